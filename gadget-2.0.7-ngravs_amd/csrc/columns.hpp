// columns.hpp -- what every entry point of the C ABI does with a caller's column (a pointer, a byte stride, on_device): pack its
// rows into a contiguous device buffer, unpack a device result into the caller's rows, refuse with "<who>: <why>".  columns.hip
#pragma once
#include "engine.hpp"
#include "rows.hpp"

#define GRID1(n) dim3((unsigned)(((n) + 255) / 256)), dim3(256)

// a refusal of the entry point who: reported as "<who>: <why>", nothing is written
struct Refuse
{
  ngravs_ctx *c;
  const char *who;
  int operator()(int code, const std::string &why) const
  {
    ngravs_report(c, code, std::string(who) + ": " + why);
    return code;
  }
};

// n rows of ncomp elements of elem_bytes (4 or 8 on the device) -> dst, contiguous on the device.  A host column is on the device
// when the call returns (the stream is synchronised); a device column is only enqueued on c->stream.
int col_upload(ngravs_ctx *c, const void *src, int64_t stride, size_t elem_bytes, int ncomp, int64_t n, int on_device, void *dst);
// a host column packed at the front of c->host_stage, which then holds `total` >= row_bytes * n bytes: for columns that are checked
// or converted on the host before they are uploaded (from there, contiguous: col_upload does not touch the staging buffer then)
unsigned char *col_stage_rows(ngravs_ctx *c, const void *src, int64_t stride, size_t row_bytes, int64_t n, size_t total);
// dsrc, contiguous on the device -> the caller's rows, complete when the call returns; with d_mask (one byte per row, on the device)
// only the rows whose bit 0 is set.  A device destination must be contiguous: refused with NGRAVS_ERR_ARG otherwise, nothing written.
int col_download(ngravs_ctx *c, const void *dsrc, size_t elem_bytes, int ncomp, int64_t n, void *dst, int64_t stride, int on_device,
                 const unsigned char *d_mask);
// a device result column (NULL: zeros) -> the caller's contiguous array
int col_deliver_or_zeros(ngravs_ctx *c, const void *res, size_t bytes, void *out, int on_device);

// columns that are converted or checked while they are packed (device columns; set_particles_impl has the host counterparts)
__global__ void k_pack_strided_f32_to_f64(const unsigned char *src, long long stride, long long n, double *dst);
__global__ void k_pack_type(const unsigned char *src, long long stride, long long n, int *dst, int *nbad);
__global__ void k_pack_active(const unsigned char *src, long long stride, long long n, unsigned char *dst);
__global__ void k_fill_f64(double *p, long long n, double v);
__global__ void k_fill_u8(unsigned char *p, long long n, unsigned char v);
// caller order <-> Peano order (idx[i]: the caller's row of sorted row i); _lim: a column that only exists for the first lim (own) rows
__global__ void k_permute_f64(const unsigned int *idx, long long n, int ncomp, const double *src, double *dst);
__global__ void k_permute_f64_lim(const unsigned int *idx, long long n, long long lim, int ncomp, const double *src, double *dst);
__global__ void k_unpermute_f64(const unsigned int *idx, long long n, int ncomp, const double *src, double *dst);
__global__ void k_unpermute_f64_lim(const unsigned int *idx, long long n, long long lim, int ncomp, const double *src, double *dst);
__global__ void k_unpermute_i2f(const unsigned int *idx, long long n, const int *src, float *dst);
