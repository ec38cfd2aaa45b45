// time_common.hpp -- what the units that stream over ngravs_time_cols_t share (kernels_time.hip, kernels_snapshot.hip): the column
// views, the look-up of driftfac.c, and the staging of one call's columns on the device.
#pragma once
#include "engine.hpp"
#include "columns.hpp"
#include <cmath>

#define TI_BASE NGRAVS_TIMEBASE
#define TT_LEN NGRAVS_DRIFT_TABLE_LENGTH

// the columns of ngravs_time_cols_t, in its order
enum { TC_TYPE, TC_POS, TC_VEL, TC_MASS, TC_TIB, TC_TIE, TC_GA, TC_GPM, TC_VP, TC_HA, TC_ENT, TC_DTE, TC_RHO, TC_H, TC_PRES, TC_DIV, TC_MSV, TC_COUNT };
static const int tc_bytes[TC_COUNT] = {4, 24, 24, 8, 4, 4, 24, 24, 24, 24, 8, 8, 8, 8, 8, 8, 8};
static const char *const tc_name[TC_COUNT] = {"type", "pos", "vel", "mass", "ti_begstep", "ti_endstep", "grav_accel", "grav_pm", "vel_pred",
                                              "hydro_accel", "entropy", "dt_entropy", "density", "hsml", "pressure", "div_vel", "max_signal_vel"};
#define TB(k) (1u << (k))
static_assert(offsetof(ngravs_time_cols_t, n) == 16 * TC_COUNT && offsetof(ngravs_time_cols_t, max_signal_vel) == 16 * TC_MSV,
              "ngravs_time_cols_t is TC_COUNT pairs of pointer and stride");

struct TCol
{
  unsigned char *p;
  long long stride;
};
struct TCols
{
  TCol c[TC_COUNT];
  long long n;
};

__device__ inline double ldd(const TCol &c, long long i, int k = 0) { return reinterpret_cast<const double *>(c.p + i * c.stride)[k]; }
__device__ inline void sdd(const TCol &c, long long i, int k, double v) { reinterpret_cast<double *>(c.p + i * c.stride)[k] = v; }
__device__ inline int ldi(const TCol &c, long long i) { return *reinterpret_cast<const int *>(c.p + i * c.stride); }
__device__ inline void sdi(const TCol &c, long long i, int v) { *reinterpret_cast<int *>(c.p + i * c.stride) = v; }

// ---- the look-up of driftfac.c:67-174, one table ------------------------------------------------------------------------------------
// (no contraction into fused multiply-adds: a1 - logTimeBegin cancels, and host and device are to give the same bits)
__host__ __device__ inline double time_factor(const double *T, double ltb, double ltm, double tbi, int time0, int time1)
{
#pragma clang fp contract(off)
  const double a1 = ltb + time0 * tbi;
  const double a2 = ltb + time1 * tbi;
  const double u1 = (a1 - ltb) / (ltm - ltb) * TT_LEN;
  int i1 = (int)u1;
  if(i1 >= TT_LEN)
    i1 = TT_LEN - 1;
  double df1;
  if(i1 <= 1)
    df1 = u1 * T[0];
  else
    df1 = T[i1 - 1] + (T[i1] - T[i1 - 1]) * (u1 - i1);
  const double u2 = (a2 - ltb) / (ltm - ltb) * TT_LEN;
  int i2 = (int)u2;
  if(i2 >= TT_LEN)
    i2 = TT_LEN - 1;
  double df2;
  if(i2 <= 1)
    df2 = u2 * T[0];
  else
    df2 = T[i2 - 1] + (T[i2] - T[i2 - 1]) * (u2 - i2);
  return df2 - df1;
}
struct TimeTabs   // [drift | gravkick | hydrokick], TT_LEN each
{
  const double *t;
  double ltb, ltm, tbi;
  __host__ __device__ double drift(int t0, int t1) const { return time_factor(t, ltb, ltm, tbi, t0, t1); }
  __host__ __device__ double gravkick(int t0, int t1) const { return time_factor(t + TT_LEN, ltb, ltm, tbi, t0, t1); }
  __host__ __device__ double hydrokick(int t0, int t1) const { return time_factor(t + 2 * TT_LEN, ltb, ltm, tbi, t0, t1); }
};

// ---- host side ----------------------------------------------------------------------------------------------------------------------
inline size_t up256(size_t x) { return (x + 255) & ~(size_t)255; }

// The columns of one call on the device.  need: columns that must be given; gas: columns that must be given if a type-0 row exists
// (gas_ok says whether they all are); write: columns the call writes.  Device pointers are used in place; host columns are copied to
// the scratch buffer behind `scratch` bytes of the call's own and copied back by finish().
struct TimeStage
{
  ngravs_ctx *c;
  const ngravs_time_cols_t *in;
  TCols d;
  unsigned char *scratch = nullptr;
  int gas_ok = 1;
  unsigned staged = 0;

  int begin(const Refuse &refuse, unsigned need, unsigned gas, size_t scratch_bytes)
  {
    const TCol *src = reinterpret_cast<const TCol *>(in);
    const long long n = in->n;
    if(n < 0)
      return refuse(NGRAVS_ERR_ARG, "n must be >= 0");
    for(int k = 0; k < TC_COUNT; k++)
      {
        if((need & TB(k)) && n > 0 && !src[k].p)
          return refuse(NGRAVS_ERR_ARG, std::string(tc_name[k]) + " must not be NULL");
        if((gas & TB(k)) && !src[k].p)
          gas_ok = 0;
        if(((need | gas) & TB(k)) && src[k].p && src[k].stride < tc_bytes[k] && n > 1)
          return refuse(NGRAVS_ERR_ARG, std::string(tc_name[k]) + "_stride is smaller than the field");
      }
    (void)hipSetDevice(c->cfg.device);
    size_t total = up256(scratch_bytes);
    size_t off[TC_COUNT];
    d.n = n;
    for(int k = 0; k < TC_COUNT; k++)
      {
        d.c[k] = src[k];
        if(!in->on_device && ((need | gas) & TB(k)) && src[k].p)
          {
            off[k] = total;
            total += up256((size_t)n * tc_bytes[k]);
            staged |= TB(k);
          }
      }
    if(c->time_buf.ensure(total))
      return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
    scratch = c->time_buf.p;
    for(int k = 0; k < TC_COUNT; k++)
      if(staged & TB(k))
        {
          if(int rc = col_upload(c, src[k].p, src[k].stride, tc_bytes[k], 1, n, 0, c->time_buf.p + off[k]))
            return rc;
          d.c[k].p = c->time_buf.p + off[k];
          d.c[k].stride = tc_bytes[k];
        }
    return NGRAVS_OK;
  }
  // the written columns back into the caller's host arrays (device columns were written in place)
  int finish(unsigned write)
  {
    HIP_TRY(c, hipStreamSynchronize(c->stream));
    const TCol *src = reinterpret_cast<const TCol *>(in);
    const long long n = in->n;
    for(int k = 0; k < TC_COUNT; k++)
      if(staged & write & TB(k))
        if(int rc = col_download(c, d.c[k].p, tc_bytes[k], 1, n, src[k].p, src[k].stride, 0, nullptr))
          return rc;
    return NGRAVS_OK;
  }
};

inline int time_params_check(const Refuse &refuse, const ngravs_time_params_t *par)
{
  if(!par)
    return refuse(NGRAVS_ERR_ARG, "params must not be NULL");
  if(!(par->timebase_interval > 0))
    return refuse(NGRAVS_ERR_ARG, "timebase_interval must be > 0");
  if(!(par->gamma >= 1))
    return refuse(NGRAVS_ERR_ARG, "gamma must be >= 1");
  if(par->comoving && (!par->drift_table || !par->gravkick_table || !par->hydrokick_table))
    return refuse(NGRAVS_ERR_ARG, "a comoving call needs the three tables");
  if(par->comoving && (!(par->time_begin > 0) || !(par->time_max > par->time_begin)))
    return refuse(NGRAVS_ERR_ARG, "comoving: 0 < time_begin < time_max");
  return NGRAVS_OK;
}
inline TimeTabs time_host_tabs(const ngravs_time_params_t *par, const double *t)
{
  TimeTabs tt;
  tt.t = t;
  tt.ltb = log(par->time_begin);
  tt.ltm = log(par->time_max);
  tt.tbi = par->timebase_interval;
  return tt;
}
