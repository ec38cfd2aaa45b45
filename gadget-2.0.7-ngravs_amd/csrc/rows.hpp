// rows.hpp -- the only code that walks a caller's host memory row by row: plain byte loops, no HIP (tools/host_asan/rows_harness.cpp
// compiles this file alone).  A column is a pointer and a byte stride; row i is the row_bytes bytes at p + i * stride, and nothing
// outside these bytes is read or written -- the last row of a record array may end with its field.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstring>

// the caller's rows -> a contiguous copy
inline void rows_gather(const void *src, int64_t stride, size_t row_bytes, int64_t n, void *dst)
{
  for(int64_t i = 0; i < n; i++)
    memcpy(static_cast<unsigned char *>(dst) + i * row_bytes, static_cast<const unsigned char *>(src) + i * stride, row_bytes);
}

// a contiguous copy -> the caller's rows; with a mask (one byte per row) only the rows whose bit 0 is set
inline void rows_scatter(const void *src, size_t row_bytes, int64_t n, void *dst, int64_t stride, const unsigned char *mask = nullptr)
{
  for(int64_t i = 0; i < n; i++)
    if(!mask || (mask[i] & 1))
      memcpy(static_cast<unsigned char *>(dst) + i * stride, static_cast<const unsigned char *>(src) + i * row_bytes, row_bytes);
}
