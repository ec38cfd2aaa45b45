// The host row loops of the column layer (csrc/rows.hpp) under AddressSanitizer + UndefinedBehaviorSanitizer, on buffers that end
// with the last row's field: a column of n rows at stride s is allocated at exactly (n - 1) * s + row_bytes bytes, as the last
// record of an array of structs whose field comes last.  Each result is compared with a byte-wise restatement.
// tests/test_rows_asan.py builds and runs this file; it includes nothing of the GPU.
#include "rows.hpp"
#include <cstdio>
#include <cstdlib>
#include <vector>

static unsigned long long rng_state = 0x9e3779b97f4a7c15ull;
static unsigned char rnd()
{
  rng_state = rng_state * 6364136223846793005ull + 1442695040888963407ull;
  return (unsigned char)(rng_state >> 56);
}

// exactly `bytes` bytes from malloc (so that one byte more is a finding), filled with random bytes
static unsigned char *exact(size_t bytes)
{
  unsigned char *p = static_cast<unsigned char *>(malloc(bytes));
  if(!p && bytes)
    abort();
  for(size_t i = 0; i < bytes; i++)
    p[i] = rnd();
  return p;
}

static int fail(const char *what, long long n, size_t row, long long stride)
{
  printf("FAILED: %s n=%lld row=%zu stride=%lld\n", what, n, row, stride);
  return 1;
}

static int check(long long n, size_t row, long long stride)
{
  const size_t col_bytes = n > 0 ? (size_t)(n - 1) * stride + row : 0, packed_bytes = (size_t)n * row;
  // gather
  unsigned char *col = exact(col_bytes), *packed = exact(packed_bytes);
  rows_gather(col, stride, row, n, packed);
  for(long long i = 0; i < n; i++)
    for(size_t b = 0; b < row; b++)
      if(packed[i * row + b] != col[i * stride + b])
        return fail("gather", n, row, stride);
  // scatter, without a mask and with one: bytes between the fields and rows whose bit 0 is clear keep what they held
  for(int masked = 0; masked < 2; masked++)
    {
      unsigned char *dst = exact(col_bytes), *mask = exact((size_t)n);
      std::vector<unsigned char> want(dst, dst + col_bytes);
      for(long long i = 0; i < n; i++)
        if(!masked || (mask[i] & 1))
          for(size_t b = 0; b < row; b++)
            want[i * stride + b] = packed[i * row + b];
      rows_scatter(packed, row, n, dst, stride, masked ? mask : nullptr);
      for(size_t b = 0; b < col_bytes; b++)
        if(dst[b] != want[b])
          return fail(masked ? "masked scatter" : "scatter", n, row, stride);
      free(dst);
      free(mask);
    }
  free(col);
  free(packed);
  return 0;
}

int main()
{
  const long long ns[] = {0, 1, 2, 257};
  const size_t rows[] = {1, 4, 8, 24};
  int checked = 0;
  for(long long n : ns)
    for(size_t row : rows)
      for(long long stride : {(long long)row, (long long)row + 12, (long long)(3 * row + 5)})
        {
          if(check(n, row, stride))
            return 1;
          checked++;
        }
  printf("%d cases OK\n", checked);
  return 0;
}
