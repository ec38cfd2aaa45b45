// columns.hip -- the strided-column transfer layer under the C ABI (columns.hpp): no arithmetic, bits in, the same bits out.
#include "columns.hpp"

// ---- device helpers: one thread per row -------------------------------------------------------------------------------------
template <class T> __global__ void k_pack_strided(const unsigned char *src, long long stride, int ncomp, long long n, T *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  const T *s = reinterpret_cast<const T *>(src + i * stride);
  for(int k = 0; k < ncomp; k++)
    dst[i * ncomp + k] = s[k];
}
// rows of the caller-order result that belong to active particles only (gravtree.c:318-341 touch nothing else); a row is
// `words` 4-byte words
__global__ void k_copy_masked(const unsigned char *__restrict__ act, long long n, int words, const unsigned int *__restrict__ src,
                              unsigned int *__restrict__ dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n || !(act[i] & 1))
    return;
  for(int k = 0; k < words; k++)
    dst[i * words + k] = src[i * words + k];
}
__global__ void k_pack_strided_f32_to_f64(const unsigned char *src, long long stride, long long n, double *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    dst[i] = (double)*reinterpret_cast<const float *>(src + i * stride);
}
// Type column: values outside 0..5 would index fsoft[] / t2g[] out of bounds; they are counted (the host path
// rejects them before the upload) and clamped
__global__ void k_pack_type(const unsigned char *src, long long stride, long long n, int *dst, int *nbad)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  int t = *reinterpret_cast<const int *>(src + i * stride);
  if(t < 0 || t >= NGRAVS_NTYPES)
    {
      atomicAdd(nbad, 1);
      t = t < 0 ? 0 : NGRAVS_NTYPES - 1;
    }
  dst[i] = t;
}
// active flag: only bit 0 is the caller's (bit 1 marks halo copies inside the engine)
__global__ void k_pack_active(const unsigned char *src, long long stride, long long n, unsigned char *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    dst[i] = src[i * stride] ? 1 : 0;
}
__global__ void k_fill_f64(double *p, long long n, double v)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    p[i] = v;
}
__global__ void k_fill_u8(unsigned char *p, long long n, unsigned char v)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    p[i] = v;
}
// Peano order -> caller order
__global__ void k_unpermute_f64(const unsigned int *idx, long long n, int ncomp, const double *src, double *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  long long j = idx[i];
  for(int k = 0; k < ncomp; k++)
    dst[j * ncomp + k] = src[i * ncomp + k];
}
__global__ void k_unpermute_i2f(const unsigned int *idx, long long n, const int *src, float *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    dst[idx[i]] = (float)src[i];
}
__global__ void k_permute_f64(const unsigned int *idx, long long n, int ncomp, const double *src, double *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  long long j = idx[i];
  for(int k = 0; k < ncomp; k++)
    dst[i * ncomp + k] = src[j * ncomp + k];
}
// Peano order <- caller order for a column that only exists for the first `lim` (own) rows: imported copies read 0
__global__ void k_permute_f64_lim(const unsigned int *idx, long long n, long long lim, int ncomp, const double *src, double *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  long long j = idx[i];
  for(int k = 0; k < ncomp; k++)
    dst[i * ncomp + k] = j < lim ? src[j * ncomp + k] : 0.0;
}
// Peano order -> caller order, own rows only
__global__ void k_unpermute_f64_lim(const unsigned int *idx, long long n, long long lim, int ncomp, const double *src, double *dst)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  long long j = idx[i];
  if(j < lim)
    for(int k = 0; k < ncomp; k++)
      dst[j * ncomp + k] = src[i * ncomp + k];
}

// ---- host side --------------------------------------------------------------------------------------------------------------
// c->host_stage is the one scratch vector of every hand-over: a resize invalidates what an earlier call returned, so each
// function below takes all the space it needs at once and is done with it when it returns
unsigned char *col_stage_rows(ngravs_ctx *c, const void *src, int64_t stride, size_t row_bytes, int64_t n, size_t total)
{
  c->host_stage.resize(total);
  rows_gather(src, stride, row_bytes, n, c->host_stage.data());
  return c->host_stage.data();
}

int col_upload(ngravs_ctx *c, const void *src, int64_t stride, size_t elem_bytes, int ncomp, int64_t n, int on_device, void *dst)
{
  const size_t row = elem_bytes * ncomp;
  const bool packed = stride == (int64_t)row;
  if(on_device)
    {
      const unsigned char *s = static_cast<const unsigned char *>(src);
      if(packed)
        HIP_TRY(c, hipMemcpyAsync(dst, src, row * n, hipMemcpyDeviceToDevice, c->stream));
      else if(elem_bytes == 8)
        hipLaunchKernelGGL(k_pack_strided<unsigned long long>, GRID1(n), 0, c->stream, s, (long long)stride, ncomp, (long long)n,
                           static_cast<unsigned long long *>(dst));
      else if(elem_bytes == 4)
        hipLaunchKernelGGL(k_pack_strided<unsigned int>, GRID1(n), 0, c->stream, s, (long long)stride, ncomp, (long long)n,
                           static_cast<unsigned int *>(dst));
      else
        {
          ngravs_report(c, NGRAVS_ERR_ARG, "strided device columns have 4- or 8-byte elements");
          return NGRAVS_ERR_ARG;
        }
      return NGRAVS_OK;
    }
  const void *h = packed ? src : col_stage_rows(c, src, stride, row, n, row * (size_t)n);
  HIP_TRY(c, hipMemcpyAsync(dst, h, row * n, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

int col_download(ngravs_ctx *c, const void *dsrc, size_t elem_bytes, int ncomp, int64_t n, void *dst, int64_t stride, int on_device,
                 const unsigned char *d_mask)
{
  const size_t row = elem_bytes * ncomp;
  if(on_device)
    {
      if((size_t)stride != row)
        {
          ngravs_report(c, NGRAVS_ERR_ARG, "device outputs must be contiguous");
          return NGRAVS_ERR_ARG;
        }
      if(d_mask)
        hipLaunchKernelGGL(k_copy_masked, GRID1(n), 0, c->stream, d_mask, (long long)n, (int)(row / 4),
                           static_cast<const unsigned int *>(dsrc), static_cast<unsigned int *>(dst));
      else
        HIP_TRY(c, hipMemcpyAsync(dst, dsrc, row * n, hipMemcpyDeviceToDevice, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      return NGRAVS_OK;
    }
  if(!d_mask && (size_t)stride == row)
    {
      HIP_TRY(c, hipMemcpyAsync(dst, dsrc, row * n, hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      return NGRAVS_OK;
    }
  // rows first, the mask behind them: one resize, so neither pointer moves
  c->host_stage.resize(row * (size_t)n + (d_mask ? (size_t)n : 0));
  unsigned char *hrows = c->host_stage.data(), *hmask = d_mask ? hrows + row * (size_t)n : nullptr;
  HIP_TRY(c, hipMemcpyAsync(hrows, dsrc, row * n, hipMemcpyDeviceToHost, c->stream));
  if(d_mask)
    HIP_TRY(c, hipMemcpyAsync(hmask, d_mask, (size_t)n, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  rows_scatter(hrows, row, n, dst, stride, hmask);
  return NGRAVS_OK;
}

int col_deliver_or_zeros(ngravs_ctx *c, const void *res, size_t bytes, void *out, int on_device)
{
  if(res)
    HIP_TRY(c, hipMemcpyAsync(out, res, bytes, on_device ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost, c->stream));
  else if(on_device)
    HIP_TRY(c, hipMemsetAsync(out, 0, bytes, c->stream));
  else
    memset(out, 0, bytes);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}
