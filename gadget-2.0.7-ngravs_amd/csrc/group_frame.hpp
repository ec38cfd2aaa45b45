// group_frame.hpp -- what k_walk_group2 (kernels_walk.hip, all modes where a piece applies) and k_eval_ring (kernels_eval.hip) share
// of a group's set-up: the XCD a wave runs on, the group's box, the wrap decisions, the constants of the fp32 reach pre-test, and how
// a group's statistics and results leave the wave.  Plain functions of their arguments; the rest stays with each kernel.
#pragma once
#include "walk_device.hpp"

// ---- group assignment of the persistent kernels ----------------------------------------------------------------------------------
// XCD-aware: the Peano order is cut into 8 contiguous segments, one per XCD (own L2), and a wave pulls groups from the segment of
// the XCD it runs on (neighbouring groups share most of their tree nodes and sources) and steals from the others when that one
// is exhausted.  Placement only affects speed.
__device__ __forceinline__ unsigned group_xcc()
{
  unsigned xcc = 0;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  return xcc & 7u;
}
// ---- the group's bounding box (wave-uniform, SGPRs) from the per-lane extremes -------------------------------------------------------
struct GroupBox
{
  double cx, cy, cz, hx, hy, hz;   // centre, half sides
  __device__ __forceinline__ double hmax() const { return fmax(hx, fmax(hy, hz)); }
};
__device__ __forceinline__ GroupBox group_box(double mnx, double mxx, double mny, double mxy, double mnz, double mxz)
{
  const double lox = wave_min(mnx), hix = wave_max(mxx);
  const double loy = wave_min(mny), hiy = wave_max(mxy);
  const double loz = wave_min(mnz), hiz = wave_max(mxz);
  return {wave_uniform(0.5 * (lox + hix)), wave_uniform(0.5 * (loy + hiy)), wave_uniform(0.5 * (loz + hiz)),
          wave_uniform(0.5 * (hix - lox)), wave_uniform(0.5 * (hiy - loy)), wave_uniform(0.5 * (hiz - loz))};
}

// ---- how a periodic group takes its images (wave-uniform by construction; read through an SGPR so that the branches on them are
// scalar branches) -------------------------------------------------------------------------------------------------------------------
// may sources be wrapped once per group, relative to the box centre (else, in a periodic run: images per pair)?
template <bool PM> __device__ __forceinline__ bool group_prewrap(int periodic, double boxhalf, double reach2, double bhmax)
{
  return __builtin_amdgcn_readfirstlane((int)(periodic && PM && (boxhalf - bhmax) * (boxhalf - bhmax) > reach2 && (boxhalf - bhmax) > 0)) != 0;
}
// A group whose whole region [box - reach, box + reach] lies inside the periodic box needs no image arithmetic at all: with
// every source inside [0, L] (src_in_box) a plain difference IS the nearest-image difference for everything within reach, and
// everything else fails the cull either way.  (Scalars, not WalkParams: handed the struct, 24 instantiations of k_walk_group2
// compile differently, one with more scratch.)
template <bool PM> __device__ __forceinline__ bool group_nowrap(int periodic, int src_in_box, double boxlen, double reach2, const GroupBox &b)
{
  bool nowrap = !periodic;
  if(PM && periodic && src_in_box)
    {
      const double rl_ = __builtin_sqrt(reach2);
      nowrap = __builtin_amdgcn_readfirstlane((int)(b.cx - b.hx - rl_ >= 0.0 && b.cx + b.hx + rl_ <= boxlen && b.cy - b.hy - rl_ >= 0.0 &&
                                                    b.cy + b.hy + rl_ <= boxlen && b.cz - b.hz - rl_ >= 0.0 &&
                                                    b.cz + b.hz + rl_ <= boxlen)) != 0;
    }
  return nowrap;
}

// ---- fp32 reach pre-test on the matrix cores (PM, no per-pair wrapping) --------------------------------------------------------------
// hit <=> |e|^2 - 2 e.t + |t|^2 - thr < 0 with entry e and target t relative to the box centre in fp32.  The threshold is widened
// by the worst-case rounding so that NO TRUE HIT IS LOST; the force loop re-tests in fp64.  e and t are fp32 roundings of
// coordinates relative to the box centre (each component <= bhmax + reach), so the true r2 moves by <= 4 rl dl; the evaluation
// itself makes <= 8 roundings of magnitudes <= M = 3 (2 bhmax + rl)^2.  (tx, ty, tz): the target relative to the box centre.
// Returns (-2 tx, -2 ty, -2 tz, |t|^2 - thr).
__device__ __forceinline__ float4 reach_pretest(double tx, double ty, double tz, double bhmax, double reach2)
{
  float4 r;
  const float tfx = (float)tx, tfy = (float)ty, tfz = (float)tz;
  r.x = -2.0f * tfx, r.y = -2.0f * tfy, r.z = -2.0f * tfz;
  const double rl = __builtin_sqrt(reach2);
  const double dl = 4.76837158203125e-07 * (bhmax + rl);   // 2^-21 x the largest relative coordinate
  const double M = 3.0 * (2.0 * bhmax + rl) * (2.0 * bhmax + rl);
  const double thr = (reach2 + 4.0 * rl * dl + 1.0e-6 * M) * (1.0 + 2e-6);
  r.w = (float)((double)tfx * tfx + (double)tfy * tfy + (double)tfz * tfz - thr);
  r.w = r.w - 1.2e-7f * __builtin_fabsf(r.w);   // the cast may have rounded up: one ulp down
  return r;
}

// ---- a group's statistics and results ------------------------------------------------------------------------------------------------
// The traversal statistics of unit ru, which the traversal kernel left behind the list lengths in gcount: read by the first group
// of the unit (grel: the group's index in the batch of g_cnt groups), wave-uniform, kept in SGPRs.  Then the group's four sums go
// to the wave's: per wave over its groups, flushed ONCE
template <int NG>
__device__ __forceinline__ void unit_stats(const int *gcount, long long grel, long long g_cnt, int SG, long long ru, int &nodes, int &batches)
{
  if(grel % SG == 0)
    {
      const long long u_cnt = (g_cnt + SG - 1) / SG;
      nodes = __builtin_amdgcn_readfirstlane(gcount[NG * u_cnt + ru]);
      batches = __builtin_amdgcn_readfirstlane(gcount[(NG + 1) * u_cnt + ru]);
    }
}
__device__ __forceinline__ void walk_stats_add(unsigned long long (&acc_st)[4], int st_entries, int st_nodes, int st_batches, int st_iters)
{
  acc_st[0] += (unsigned long long)st_entries;
  acc_st[1] += (unsigned long long)st_nodes;
  acc_st[2] += (unsigned long long)st_batches;
  acc_st[3] += (unsigned long long)st_iters;
}
// the S lanes of a target hold partial sums: added, and the first of them stores the target's result
__device__ __forceinline__ void group_store(int S, int lane, bool valid, long long ti, double &ax, double &ay, double &az, int &nint,
                                            double *r_acc, int *r_nint)
{
  if(S > 1)
    {
      for(int off = 1; off < S; off <<= 1)
        {
          ax += __shfl_xor(ax, off);
          ay += __shfl_xor(ay, off);
          az += __shfl_xor(az, off);
          nint += __shfl_xor(nint, off);
        }
    }
  if(valid && (lane & (S - 1)) == 0)
    {
      r_acc[3 * ti + 0] = ax;
      r_acc[3 * ti + 1] = ay;
      r_acc[3 * ti + 2] = az;
      r_nint[ti] = nint;
    }
}
