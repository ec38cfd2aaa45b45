// strict_walk.hpp -- the traversal of the strict-walk family: k_walk_strict / k_walk_targets (kernels_walk.hip: the force pass and
// the lattice-correction pass) and k_potential_walk / k_potential_targets (kernels_potential.hip).  One wave64 per 64 targets walks
// the tree depth-first in lock-step; every lane takes its own decision at every node.  What is here is what the walks share: the
// driver, a node's species offsets from a target, the opening criterion, the reach box of the TreePM prunes, the pseudo-node
// report and the kernels' prologues.  What a walk adds -- its interaction, its softening rule, its prune -- stays with the walk.
// Everything is compiled without contraction into fused multiply-adds, as the reference is.
#pragma once
#include "engine.hpp"
#include "walk_device.hpp"

#pragma clang fp contract(off)

// What the strict walk knows of its target (the reference's walk reads the same of P[target] or of GravDataGet[target],
// forcetree.c:1284-1313 / :1668-1695): position, ErrTolForceAcc * OldAcc, the softening length of its type (ADA: its own), its mass
// (read by the BAM laws alone) and its species
struct StrictTarget
{
  double x, y, z, aold, h, mass;
  int tg;
};

// The lock-step depth-first driver.  A lane that has dealt with a node (used it, or pruned it) while another lane wants it opened
// sits out until the walk has left that node's subtree: lane_skip = the stack depth of the node, the lane takes part only while
// sp < lane_skip.  (Depth, not particle ranges: the pseudo nodes of a multi-task tree have EMPTY ranges, which a test on particle
// indices cannot tell from "behind the subtree".)
struct StrictDfs
{
  static constexpr int NO_SKIP = 0x7fffffff;
  int *sn, *ss;   // the wave's node and slot stack in LDS
  int sp, lane_skip;

  // before each pass; a lane that is not `valid` walks along without taking part
  __device__ __forceinline__ void reset(bool valid) { lane_skip = valid ? NO_SKIP : -1; }
  __device__ __forceinline__ bool takes_part() const { return lane_skip > sp; }
  // the end of a visit, given whether this lane took part in it and whether it wants the node opened: true if some lane does
  __device__ __forceinline__ bool settle(bool took_part, bool open)
  {
    const bool wave_open = __any(open ? 1 : 0) != 0;
    if(wave_open && took_part && !open)
      lane_skip = sp + 1;   // the node goes onto the stack at depth sp + 1: this lane is done with everything below it
    return wave_open;
  }
  // visit_fn(node) -> settle(open); particle_fn(row).  Control flow is wave-uniform: node and slot live in SGPRs
  template <class V, class P> __device__ __forceinline__ void run(const TreeView &tv, V &&visit_fn, P &&particle_fn)
  {
    sp = -1;
    if(visit_fn(0))
      {
        sp = 0;
        sn[0] = 0;
        ss[0] = 0;
      }
    while(sp >= 0)
      {
        int node = __builtin_amdgcn_readfirstlane(sn[sp]);
        int slot = __builtin_amdgcn_readfirstlane(ss[sp]);
        int fl = tv.flags[node];
        if(fl & FLAG_BUCKET)
          {
            int f = tv.first[node], cnt = tv.count[node];
            if(slot >= cnt)
              {
                sp--;
                if(lane_skip > sp && lane_skip >= 0)
                  lane_skip = NO_SKIP;
                continue;
              }
            ss[sp] = slot + 1;
            particle_fn(f + slot);
            continue;
          }
        if(slot >= 8)
          {
            sp--;
            if(lane_skip > sp && lane_skip >= 0)
              lane_skip = NO_SKIP;   // the walk has left the subtree this lane sat out
            continue;
          }
        ss[sp] = slot + 1;
        int c = __builtin_amdgcn_readfirstlane(tv.child[8 * (long long)node + slot]);
        if(c == -1)
          continue;
        if(c <= -2)
          {
            particle_fn(-2 - c);
            continue;
          }
        if(visit_fn(c))
          {
            sp++;
            sn[sp] = c;
            ss[sp] = 0;
          }
      }
  }
};

// a source (particle, or one species' centre of mass: xyz of q) from the target; wrap: to the nearest image.  Returns r^2
__device__ __forceinline__ double offset_from(const double4 &q, const StrictTarget &T, const WalkParams &wp, bool wrap, double &dx, double &dy,
                                              double &dz)
{
  dx = q.x - T.x;
  dy = q.y - T.y;
  dz = q.z - T.z;
  if(wrap)
    {
      dx = nearest(dx, wp.box, wp.boxhalf);
      dy = nearest(dy, wp.box, wp.boxhalf);
      dz = nearest(dz, wp.box, wp.boxhalf);
    }
  return dx * dx + dy * dy + dz * dz;
}

// a node's moments (uniform address -> scalar loads: read by the whole wave, whoever takes part) ...
template <int NG> __device__ __forceinline__ void node_moments(const TreeView &tv, int c, double4 (&mom)[NG])
{
#pragma unroll
  for(int g = 0; g < NG; g++)
    mom[g] = tv.mom[(long long)c * NG + g];
}
// ... and what a lane that takes part makes of them: the offset of every species' centre of mass, the nearest and the farthest
// of them, the node's mass
template <int NG>
__device__ __forceinline__ void species_offsets(const double4 (&mom)[NG], const StrictTarget &T, const WalkParams &wp, bool wrap, double (&dx)[NG],
                                                double (&dy)[NG], double (&dz)[NG], double (&r2)[NG], double &r2min, double &r2max, double &summass)
{
  r2min = INFINITY, r2max = -INFINITY, summass = 0;
#pragma unroll
  for(int g = 0; g < NG; g++)
    {
      summass += mom[g].w;
      r2[g] = offset_from(mom[g], T, wp, wrap, dx[g], dy[g], dz[g]);
      if(r2[g] < r2min)
        r2min = r2[g];
      if(r2[g] > r2max)
        r2max = r2[g];
    }
}

// the opening criterion (forcetree.c:1437-1472, :2642-2670): true if the node (geo: centre and side) is to be opened
__device__ __forceinline__ bool node_opens(const double4 &geo, const StrictTarget &T, const WalkParams &wp, double r2min, double summass)
{
  const double len = geo.w;
  bool open = false;
  if(wp.use_theta)
    {
      if(len * len > r2min * wp.theta2)   // theta2 = ErrTolTheta^2
        open = true;
    }
  else
    {
      if(summass * len * len > r2min * r2min * T.aold)
        open = true;
      else if(fabs(geo.x - T.x) < 0.60 * len && fabs(geo.y - T.y) < 0.60 * len && fabs(geo.z - T.z) < 0.60 * len)   // (no NEAREST)
        open = true;
    }
  return open;
}

// the eff_dist box of the TreePM prunes (forcetree.c:1828-1862, :2990-3021): true if the node's centre is farther than eff from
// the target along some axis
__device__ __forceinline__ bool outside_reach_box(const double4 &geo, const StrictTarget &T, const WalkParams &wp, double eff)
{
  double d0 = geo.x - T.x, d1 = geo.y - T.y, d2 = geo.z - T.z;
  if(wp.periodic)
    {
      d0 = nearest(d0, wp.box, wp.boxhalf);
      d1 = nearest(d1, wp.box, wp.boxhalf);
      d2 = nearest(d2, wp.box, wp.boxhalf);
    }
  bool outside = false;
  if(d0 < -eff || d0 > eff || d1 < -eff || d1 > eff || d2 < -eff || d2 > eff)
    outside = true;
  return outside;
}

// A top leaf whose particles were not imported has no children: its mass would drop out of the sum.  The import decision covers
// what the criterion in force at the decomposition opens; the walk must not run with another one (the launcher reports bit 4)
__device__ __forceinline__ void report_pseudo(bool wave_open, int fl, int *__restrict__ err_flag)
{
  if(wave_open && (fl & FLAG_PSEUDO) && threadIdx.x % WAVE == 0)
    atomicOr(err_flag, 4);
}

// ---- kernel prologues: 256 threads = 4 waves, 64 consecutive targets per wave ----------------------------------------------------
// this wave's stacks, this lane's target index t of `count` and whether it has one; false: the wave has no target at all
__device__ __forceinline__ bool strict_wave(long long count, int *&sn, int *&ss, long long &t, bool &valid)
{
  __shared__ int st_node[4][MAX_LEVELS + 2], st_slot[4][MAX_LEVELS + 2];
  const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const long long grp = (long long)blockIdx.x * 4 + wave;
  sn = st_node[wave];
  ss = st_slot[wave];
  t = grp * WAVE + lane;
  valid = t < count;
  return grp * WAVE < count;
}
// the target that is own row ti
__device__ __forceinline__ StrictTarget own_target(const double4 *__restrict__ s_pm, const unsigned char *__restrict__ s_type,
                                                   const double *__restrict__ s_oldacc, const WalkParams &wp, long long ti, bool valid)
{
  StrictTarget T = {0, 0, 0, 0, 0, 1.0, 0};
  if(valid)
    {
      const double4 p = s_pm[ti];
      T.x = p.x;
      T.y = p.y;
      T.z = p.z;
      T.mass = p.w;
      const int ptype = s_type[ti];
      T.tg = wp.t2g[ptype];
      T.h = wp.fsoft[ptype];
      T.aold = wp.errtol_acc * s_oldacc[ti];
    }
  return T;
}
// the target that is record ord[t] of the caller's columns; me: that index
__device__ __forceinline__ StrictTarget record_target(const double *__restrict__ t_pos, const double *__restrict__ t_oldacc,
                                                      const double *__restrict__ t_mass, const int *__restrict__ t_type,
                                                      const unsigned int *__restrict__ ord, const WalkParams &wp, long long t, bool valid, long long &me)
{
  StrictTarget T = {0, 0, 0, 0, 0, 1.0, 0};
  me = 0;
  if(valid)
    {
      me = ord[t];
      T.x = t_pos[3 * me];
      T.y = t_pos[3 * me + 1];
      T.z = t_pos[3 * me + 2];
      T.mass = t_mass[me];
      const int ptype = t_type[me];
      T.tg = wp.t2g[ptype];
      T.h = wp.fsoft[ptype];
      T.aold = wp.errtol_acc * t_oldacc[me];
    }
  return T;
}

#pragma clang fp contract(fast)

// ---- host side -------------------------------------------------------------------------------------------------------------------
// the launch grid of such a kernel for n targets
static inline dim3 strict_grid(long long n) { return dim3((unsigned)(((n + WAVE - 1) / WAVE + 3) / 4)); }
