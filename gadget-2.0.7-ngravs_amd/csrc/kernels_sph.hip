// kernels_sph.hip -- SPH density and smoothing lengths of the gas particles on the device tree.
//
// Replaces (reference): density() for one task (density.c:56-441: the neighbour iteration and its final operations),
// density_evaluate (density.c:467-599) and ngb_treefind_variable (ngb.c:196-330).
//
// k_sph_density : one wave64 per 64 Peano-consecutive targets (active type-0 own rows), one target per lane, ALL rounds of the
//      smoothing-length iteration in one launch.  Per round the wave walks the tree once, depth-first, for the hull of the search
//      boxes of its unconverged lanes: a node is popped from an LDS stack, lanes 0-7 test its eight children (cube against hull,
//      nearest image in periodic runs, with the STORED side: a refit tree's cells may have grown); an overlapping child with at
//      most SPH_NLEAF particles (or a bucket) hands its particle range over, a larger one is pushed.  The type-0 particles of a
//      range are compacted into an LDS block (position, mass, velocity: 56 bytes), and once more than 64 are staged every lane
//      runs over the block with its own r2 < h2 test (density.c:531-575).  After the walk every lane applies the final operations
//      and the acceptance / bracketing rules of density.c:296-389 to its own target; Left, Right and h stay in registers.  The
//      reference repeats globally because of its export loop; the trial h of a particle depend on that particle alone, so the
//      per-lane iteration yields the same sequence.  A lane that was accepted drops out of the hull; the wave ends with its last.
//      fp64 throughout, no atomics on results (a lane owns its target).
//
// SPH hydrodynamic forces, the second half of the gas side (hydra.c:50-346 for one task, hydro_evaluate hydra.c:353-555,
// force_update_hmax forcetree.c:1134-1203, ngb_treefind_pairs ngb.c:64-185):
// k_sph_hydro_prep : one thread per particle of the sorted set: the caller's columns of a type-0 row go to Peano order together with
//      what hydro_evaluate derives from one particle alone (p/rho^2 times the dh/drho factor, both sound speeds, the Balsara
//      factors f1 / f2, the timestep as a double); rows of other types get Hsml 0 and are not read.  Counts bad rows.
// k_sph_hmax : per tree node the largest Hsml of the gas below it, bottom-up, one launch per level.
// k_sph_hydro : the same wave-per-64-targets walk (sph_hull_walk below), ONE walk: a child is opened when its
//      cube lies within max(largest h_i of the wave, hmax of the child) of the hull of the lanes' positions, the staged entry holds
//      13 doubles, and every lane applies hydra.c:416-534 to every staged source.
//
// How the four walk kernels share their text.  sph_wave_hull (the hull of a wave's lanes), sph_stage_density (the seven staged
// doubles of a density source) and sph_wave_counters (the statistics, one set of atomics per wave) serve all of them.
// sph_hull_walk is the depth-first walk as a template; k_sph_density_sums, k_sph_hydro and k_sph_hydro_sums go through it.
// sph_hydro_wave is the whole body of a hydro wave; k_sph_hydro and k_sph_hydro_sums are wrappers that hand it two functors: where
// a lane's target comes from (a row of sph_hsrc, or a record of sph_tg_in) and where its five results go (with or without
// hydra.c:320).  k_sph_density stands apart in ONE respect: it keeps an inline copy of the walk, because called through the
// template it takes 180 VGPRs instead of 164 and loses its third wave per SIMD (see sph_hull_walk); the three small helpers leave
// its registers, LDS and occupancy as they were, so it uses them.  Its per-lane acceptance rules are not merged with
// sph_density_update_one (engine.hpp) either: that function is compiled with contraction off, the kernel is not.
//
// The first guess of the smoothing lengths (ngravs_sph_hsml_guess; setup_smoothinglengths, init.c:229-247):
// k_sph_gas_cols : one thread per sorted particle: gas mass and gas flag, the inputs of two prefix scans over the Peano-ordered rows
// k_sph_hsml_guess : one lane per gas row: from the root down the cells that hold the particle, a node's gas mass and count as
//      differences of the scans, below the deepest level by halving the bucket's cell; no LDS, no scratch.
//
// The gas side in one call (ngravs_sph_accelerations): k_sph_density, then k_sph_gas_prep in the place of k_sph_hydro_prep (the
//      pressure line of density.c:305-308 and the hydro sources, a target's from the density results where they lie), k_sph_hmax,
//      k_sph_hydro, and one k_sph_scatter_cols for all columns.  The two walks are the kernels above, unchanged.
//
// Sums for targets that are NOT own rows (ngravs_sph_density_sums, ngravs_sph_hydro_sums; density_evaluate(j, 1) and
// hydro_evaluate(j, 1) of the reference, density.c:231-284, hydra.c:232-287): k_sph_density_sums and k_sph_hydro_sums at the end
//      of this file, one round over the engine's own gas for records handed in, raw sums out; k_sph_density_update is the owner's
//      side of a round.
#include "engine.hpp"
#include "walk_device.hpp"
#include <hipcub/hipcub.hpp>

#define SPH_WAVES 4        // waves per workgroup: 4 x 8.2 KB of LDS, five workgroups per CU
#define SPH_STAGE 128      // entries of a wave's staging block: processed when more than 64 are in, so a chunk of 64 always fits
#define SPH_STACK 256      // depth-first with eight children per pop: at most 7 * MAX_LEVELS + 1 = 155 pending nodes
#define SPH_NLEAF 64       // a node with at most this many particles is staged whole (one chunk)
static_assert(7 * MAX_LEVELS + 8 < SPH_STACK, "the LIFO must hold a depth-first walk of the deepest tree");
#define SPH_HWAVES 2       // k_sph_hydro: waves per workgroup: 2 x 14.0 KB of LDS, five workgroups per CU
#define SPH_HFIELDS 13     // doubles of a staged hydro source

struct SphParams
{
  int periodic;
  double box, boxhalf;
  double des, dev, minh;   // All.DesNumNgb, All.MaxNumNgbDeviation, All.MinGasHsml
};

// counters: [0] targets with hsml <= 0 or NaN, [1] targets over MAXITER rounds, [2] waves whose LIFO was full, [3] most rounds,
// [4] sum of rounds, [5] candidates tested (staged particles x unconverged lanes), [6] neighbours (r2 < h2), [7] (int) list length
#define SPH_C_BAD 0
#define SPH_C_FAILED 1
#define SPH_C_OVF 2
#define SPH_C_MAXR 3
#define SPH_C_SUMR 4
#define SPH_C_CAND 5
#define SPH_C_NGB 6
#define SPH_C_COUNT 7

struct SphLane
{
  double x, y, z, vx, vy, vz;
  double h2, hinv, hinv3, hinv4;
  double rho, wnn, dhr, divv, rx, ry, rz;
  unsigned ncand, nngb;
};

// every lane over the staged block (density.c:507-575)
__device__ __forceinline__ void sph_block(const double (*__restrict__ s)[SPH_STAGE], int cnt, bool live, const SphParams &sp, SphLane &L)
{
  if(live)
    L.ncand += (unsigned)cnt;
  for(int j = 0; j < cnt; j++)
    {
      double dx = L.x - s[0][j], dy = L.y - s[1][j], dz = L.z - s[2][j];
      if(sp.periodic)
        {
          dx = nearest(dx, sp.box, sp.boxhalf);
          dy = nearest(dy, sp.box, sp.boxhalf);
          dz = nearest(dz, sp.box, sp.boxhalf);
        }
      const double r2 = dx * dx + dy * dy + dz * dz;
      if(live && r2 < L.h2)
        {
          L.nngb++;
          const double r = sqrt(r2), u = r * L.hinv, m = s[3][j];
          double wk, dwk;
          sph_spline(u, L.hinv3, L.hinv4, &wk, &dwk);
          L.rho += m * wk;
          L.wnn += SPH_NORM_COEFF * wk / L.hinv3;
          L.dhr += -m * (3 * L.hinv * wk + u * dwk);
          if(r > 0)
            {
              const double fac = m * dwk / r;
              const double dvx = L.vx - s[4][j], dvy = L.vy - s[5][j], dvz = L.vz - s[6][j];
              L.divv -= fac * (dx * dvx + dy * dvy + dz * dvz);
              L.rx += fac * (dz * dvy - dy * dvz);
              L.ry += fac * (dx * dvz - dz * dvx);
              L.rz += fac * (dy * dvx - dx * dvy);
            }
        }
    }
}

// The hull of a wave: the box around the live lanes' x -/+ pad (pad: h for the search boxes of the density walks, ngb.c:206-210;
// 0 for the bare positions of the hydro walks), as centre and half sides, the latter a hair wider than the boxes' own rounding.
struct SphHull
{
  double cx, cy, cz, hx, hy, hz;
};
__device__ __forceinline__ SphHull sph_wave_hull(double x, double y, double z, double pad, bool live)
{
  const double BIG = 1e300;
  const double lx = wave_min(live ? x - pad : BIG), ly = wave_min(live ? y - pad : BIG), lz = wave_min(live ? z - pad : BIG);
  const double ux = wave_max(live ? x + pad : -BIG), uy = wave_max(live ? y + pad : -BIG), uz = wave_max(live ? z + pad : -BIG);
  SphHull H;
  H.cx = wave_uniform(0.5 * (lx + ux)), H.cy = wave_uniform(0.5 * (ly + uy)), H.cz = wave_uniform(0.5 * (lz + uz));
  H.hx = wave_uniform(0.5 * (ux - lx) * (1 + 1e-12)), H.hy = wave_uniform(0.5 * (uy - ly) * (1 + 1e-12));
  H.hz = wave_uniform(0.5 * (uz - lz) * (1 + 1e-12));
  return H;
}

// particle p into slot q of a density walk's staging block: position, mass, VelPred
__device__ __forceinline__ void sph_stage_density(double (*__restrict__ src)[SPH_STAGE], int q, long long p, const double4 *__restrict__ pm,
                                                  const double *__restrict__ svel)
{
  const double4 pp = pm[p];
  src[0][q] = pp.x, src[1][q] = pp.y, src[2][q] = pp.z, src[3][q] = pp.w;
  src[4][q] = svel[3 * p], src[5][q] = svel[3 * p + 1], src[6][q] = svel[3 * p + 2];
}

// statistics of a walk kernel: one set of atomics per wave.  ROUNDS: also the lanes' round counts nr (k_sph_density)
template <bool ROUNDS>
__device__ __forceinline__ void sph_wave_counters(int lane, unsigned ncand, unsigned nngb, int nr, bool ovf,
                                                  unsigned long long *__restrict__ counters)
{
  unsigned long long cand = ncand, ngb = nngb, sumr = (unsigned long long)nr;
  int maxr = nr;
  for(int off = 32; off > 0; off >>= 1)
    {
      cand += __shfl_xor(cand, off);
      ngb += __shfl_xor(ngb, off);
      if(ROUNDS)
        {
          sumr += __shfl_xor(sumr, off);
          const int o = __shfl_xor(maxr, off);
          maxr = o > maxr ? o : maxr;
        }
    }
  if(lane == 0)
    {
      atomicAdd(&counters[SPH_C_CAND], cand);
      atomicAdd(&counters[SPH_C_NGB], ngb);
      if(ROUNDS)
        {
          atomicAdd(&counters[SPH_C_SUMR], sumr);
          atomicMax(&counters[SPH_C_MAXR], (unsigned long long)maxr);
        }
      if(ovf)
        atomicAdd(&counters[SPH_C_OVF], 1ull);
    }
}

// The wave's depth-first walk of k_sph_density for a hull (centre hc, half sides hh) as a function of its own, for k_sph_hydro.
// k_sph_density keeps its inline copy: called through this template (same arithmetic, same results) the compiler gives it 180
// instead of 164 VGPRs, which costs the third wave per SIMD, and holding it to three waves spills.  A node is popped from the LDS
// stack, lanes 0-7 test its eight children (cube against hull, nearest image in periodic runs, with the STORED side: a refit
// tree's cells may have grown; widen(child) >= 0 is added to the hull's half sides for that child), an overlapping child with at
// most SPH_NLEAF particles (or a bucket) hands its particle range over, a larger one is pushed.  The type-0 particles of a range
// are compacted into the wave's staging block by put(slot, particle), and once more than 64 are staged block(count) runs every
// lane over it.  Returns false when the LIFO would overflow (nothing is written past it).
template <int STAGE, class Widen, class Put, class Block>
__device__ __forceinline__ bool sph_hull_walk(const TreeView &tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                              long long n, int periodic, double box, double boxhalf, const SphHull &H, int *stack, int lane,
                                              Widen widen, Put put, Block block)
{
  static_assert(STAGE >= 128, "a chunk of 64 must fit behind 64 staged entries");
  int top = 0, fill = 0;
  if(lane == 0)
    stack[0] = 0;   // the root is opened unconditionally
  top = 1;
  wave_sync();
  while(top > 0)
    {
      const int node = __builtin_amdgcn_readfirstlane(stack[top - 1]);
      top--;
      wave_sync();   // the slot is read before a push below reuses it
      // lanes 0-7: one child each
      int kind = 0, first = 0, count = 0, ch = -1;   // kind 1: push the child node, 2: hand its particle range over
      if(lane < 8)
        {
          ch = tv.child[8ll * node + lane];
          double cx = 0, cy = 0, cz = 0, half = 0;
          if(ch >= 0)
            {
              const double4 g = tv.geo[ch];
              cx = g.x, cy = g.y, cz = g.z, half = 0.5 * g.w;
            }
          else if(ch <= -2)
            {
              const double4 p = pm[-2 - ch];
              cx = p.x, cy = p.y, cz = p.z, half = 0;
            }
          if(ch != -1)
            {
              double dx = cx - H.cx, dy = cy - H.cy, dz = cz - H.cz;
              if(periodic)
                {
                  dx = nearest(dx, box, boxhalf);
                  dy = nearest(dy, box, boxhalf);
                  dz = nearest(dz, box, boxhalf);
                }
              const double wd = widen(ch);
              // (ngb.c:146-177 for the hull instead of one particle's box)
              if(fabs(dx) - half <= H.hx + wd && fabs(dy) - half <= H.hy + wd && fabs(dz) - half <= H.hz + wd)
                {
                  if(ch >= 0)
                    {
                      first = tv.first[ch];
                      count = tv.count[ch];
                      kind = (count <= SPH_NLEAF || (tv.flags[ch] & FLAG_BUCKET)) ? 2 : 1;
                    }
                  else
                    {
                      first = -2 - ch;
                      count = 1;
                      kind = 2;
                    }
                }
            }
        }
      const unsigned long long pmask = __ballot(kind == 1 ? 1 : 0);
      const int npush = __popcll(pmask);
      if(top + npush > SPH_STACK)   // cannot happen for a tree of at most MAX_LEVELS levels; never write past the LIFO
        return false;
      if(kind == 1)
        stack[top + lane_prefix(pmask)] = ch;
      top += npush;
      unsigned long long rmask = __ballot(kind == 2 ? 1 : 0);
      while(rmask)
        {
          const int l = __builtin_ctzll(rmask);
          rmask &= rmask - 1;
          const int f0 = __shfl(first, l), cn = __shfl(count, l);
          for(int o = 0; o < cn; o += 64)
            {
              const long long p = (long long)f0 + o + lane;
              const bool ok = o + lane < cn && p < n && type[p] == 0;   // P[p].Type > 0: not a neighbour (ngb.c:221)
              const unsigned long long m = __ballot(ok ? 1 : 0);
              if(ok)
                put(fill + lane_prefix(m), p);
              fill += __popcll(m);
              if(fill > 64)
                {
                  wave_sync();
                  block(fill);
                  wave_sync();
                  fill = 0;
                }
            }
        }
      wave_sync();   // pushes are visible before the next pop
    }
  if(fill > 0)
    {
      wave_sync();
      block(fill);
      wave_sync();
    }
  return true;
}

__global__ __launch_bounds__(64 * SPH_WAVES) void k_sph_density(TreeView tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                                                const double *__restrict__ svel, const unsigned int *__restrict__ idx,
                                                                const int *__restrict__ tlist, long long nt, long long n,
                                                                const double *__restrict__ h_in, SphParams sp, double *__restrict__ res,
                                                                int *__restrict__ row, int *__restrict__ rounds,
                                                                unsigned long long *__restrict__ counters)
{
  __shared__ double s_src[SPH_WAVES][7][SPH_STAGE];
  __shared__ int s_stack[SPH_WAVES][SPH_STACK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * SPH_WAVES + w) * 64 + lane;
  if(t - lane >= nt)   // the whole wave (no workgroup barrier anywhere below)
    return;
  double (*src)[SPH_STAGE] = s_src[w];
  int *stack = s_stack[w];
  const double BIG = 1e300;

  bool live = t < nt;
  SphLane L = {};
  double h = 0, left = 0, right = 0;
  int myrow = 0, nr = 0;
  if(live)
    {
      const int i = tlist[t];
      const double4 p = pm[i];
      L.x = p.x, L.y = p.y, L.z = p.z;
      L.vx = svel[3ll * i], L.vy = svel[3ll * i + 1], L.vz = svel[3ll * i + 2];
      myrow = (int)idx[i];
      h = h_in[myrow];
      if(!(h > 0) || !(h < BIG))
        {
          live = false;
          atomicAdd(&counters[SPH_C_BAD], 1ull);
        }
    }
  bool ovf = false;
  while(wave_any(live))
    {
      const SphHull H = sph_wave_hull(L.x, L.y, L.z, h, live);   // of the unconverged lanes' search boxes
      L.h2 = h * h;
      L.hinv = 1.0 / h;
      L.hinv3 = L.hinv * L.hinv * L.hinv;
      L.hinv4 = L.hinv3 * L.hinv;
      L.rho = L.wnn = L.dhr = L.divv = L.rx = L.ry = L.rz = 0;

      int top = 0, fill = 0;
      if(lane == 0)
        stack[0] = 0;   // the root is opened unconditionally
      top = 1;
      wave_sync();
      while(top > 0)
        {
          const int node = __builtin_amdgcn_readfirstlane(stack[top - 1]);
          top--;
          wave_sync();   // the slot is read before a push below reuses it
          // lanes 0-7: one child each
          int kind = 0, first = 0, count = 0, ch = -1;   // kind 1: push the child node, 2: hand its particle range over
          if(lane < 8)
            {
              ch = tv.child[8ll * node + lane];
              double cx = 0, cy = 0, cz = 0, half = 0;
              if(ch >= 0)
                {
                  const double4 g = tv.geo[ch];
                  cx = g.x, cy = g.y, cz = g.z, half = 0.5 * g.w;
                }
              else if(ch <= -2)
                {
                  const double4 p = pm[-2 - ch];
                  cx = p.x, cy = p.y, cz = p.z, half = 0;
                }
              if(ch != -1)
                {
                  double dx = cx - H.cx, dy = cy - H.cy, dz = cz - H.cz;
                  if(sp.periodic)
                    {
                      dx = nearest(dx, sp.box, sp.boxhalf);
                      dy = nearest(dy, sp.box, sp.boxhalf);
                      dz = nearest(dz, sp.box, sp.boxhalf);
                    }
                  // (ngb.c:272-297 for the hull instead of one particle's box)
                  if(fabs(dx) - half <= H.hx && fabs(dy) - half <= H.hy && fabs(dz) - half <= H.hz)
                    {
                      if(ch >= 0)
                        {
                          first = tv.first[ch];
                          count = tv.count[ch];
                          kind = (count <= SPH_NLEAF || (tv.flags[ch] & FLAG_BUCKET)) ? 2 : 1;
                        }
                      else
                        {
                          first = -2 - ch;
                          count = 1;
                          kind = 2;
                        }
                    }
                }
            }
          const unsigned long long pmask = __ballot(kind == 1 ? 1 : 0);
          const int npush = __popcll(pmask);
          if(top + npush > SPH_STACK)   // cannot happen for a tree of at most MAX_LEVELS levels; never write past the LIFO
            {
              ovf = true;
              break;
            }
          if(kind == 1)
            stack[top + lane_prefix(pmask)] = ch;
          top += npush;
          unsigned long long rmask = __ballot(kind == 2 ? 1 : 0);
          while(rmask)
            {
              const int l = __builtin_ctzll(rmask);
              rmask &= rmask - 1;
              const int f0 = __shfl(first, l), cn = __shfl(count, l);
              for(int o = 0; o < cn; o += 64)
                {
                  const long long p = (long long)f0 + o + lane;
                  const bool ok = o + lane < cn && p < n && type[p] == 0;   // P[p].Type > 0: not a neighbour (ngb.c:221)
                  const unsigned long long m = __ballot(ok ? 1 : 0);
                  if(ok)
                    sph_stage_density(src, fill + lane_prefix(m), p, pm, svel);
                  fill += __popcll(m);
                  if(fill > 64)
                    {
                      wave_sync();
                      sph_block(src, fill, live, sp, L);
                      wave_sync();
                      fill = 0;
                    }
                }
            }
          wave_sync();   // pushes are visible before the next pop
        }
      if(ovf)
        break;
      if(fill > 0)
        {
          wave_sync();
          sph_block(src, fill, live, sp, L);
          wave_sync();
        }

      if(live)
        {
          nr++;
          // final operations (density.c:296-303)
          const double numngb = L.wnn, rho = L.rho;
          const double dhf = 1 / (1 + h * L.dhr / (3 * rho));
          // enough neighbours? (density.c:314-389, rule for rule)
          bool redo = numngb < (sp.des - sp.dev) || (numngb > (sp.des + sp.dev) && h > 1.01 * sp.minh);
          if(redo && left > 0 && right > 0 && (right - left) < 1.0e-3 * left)
            redo = false;
          if(!redo)
            {
              res[SPH_HSML * nt + t] = h;
              res[SPH_DENSITY * nt + t] = rho;
              res[SPH_NUMNGB * nt + t] = numngb;
              res[SPH_DIVVEL * nt + t] = L.divv / rho;
              res[SPH_CURLVEL * nt + t] = sqrt(L.rx * L.rx + L.ry * L.ry + L.rz * L.rz) / rho;
              res[SPH_DHSML * nt + t] = dhf;
              row[t] = myrow;
              rounds[t] = nr;
              live = false;
            }
          else
            {
              if(numngb < (sp.des - sp.dev))
                left = fmax(h, left);
              else if(right != 0)
                {
                  if(h < right)
                    right = h;
                }
              else
                right = h;
              if(right > 0 && left > 0)
                h = pow(0.5 * (pow(left, 3) + pow(right, 3)), 1.0 / 3);
              else
                {
                  const bool newton = fabs(numngb - sp.des) < 0.5 * sp.des;
                  const double fac = 1 - (numngb - sp.des) / (3 * numngb) * dhf;
                  if(right == 0 && left > 0)
                    h *= newton ? fac : 1.26;
                  if(right > 0 && left == 0)
                    h = newton ? h * fac : h / 1.26;
                }
              if(h < sp.minh)
                h = sp.minh;
              if(nr > SPH_MAXITER)   // density.c:416: endrun(1155)
                {
                  atomicAdd(&counters[SPH_C_FAILED], 1ull);
                  live = false;
                }
            }
        }
    }
  sph_wave_counters<true>(lane, L.ncand, L.nngb, nr, ovf, counters);
}

struct SphIsTarget
{
  const unsigned char *type, *active;
  __host__ __device__ __forceinline__ bool operator()(const int &i) const { return type[i] == 0 && (active[i] & 1) != 0; }
};

static TreeView sph_tree_view(ngravs_ctx *c)
{
  TreeView tv = {};
  tv.first = c->n_first.p;
  tv.count = c->n_count.p;
  tv.child = c->n_child.p;
  tv.flags = c->n_flags.p;
  tv.geo = c->n_geo.p;
  tv.mom = c->n_mom.p;
  tv.nnodes = (int)c->nnodes;
  return tv;
}

// sph_counters on the host (waits for the stream)
static int sph_read_counters(ngravs_ctx *c, unsigned long long h[SPH_C_COUNT])
{
  HIP_TRY(c, hipMemcpyAsync(h, c->sph_counters.p, SPH_C_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

// workgroups of a kernel that gives one wave to 64 targets, waves waves per workgroup
static unsigned sph_wave_grid(long long nt, int waves)
{
  const long long nwaves = (nt + 63) / 64;
  return (unsigned)((nwaves + waves - 1) / waves);
}

// periodic, box, boxhalf of SphParams or SphHydroParams
template <class P> static void sph_set_box(const ngravs_ctx *c, P *p)
{
  p->periodic = c->cfg.periodic;
  p->box = c->cfg.box_size;
  p->boxhalf = 0.5 * c->cfg.box_size;
}

// the targets: active type-0 rows in Peano order (density.c:95, :123; hydra.c:101-105), compacted into sph_tlist as the group
// walk's list is; clears sph_counters
static int sph_targets(ngravs_ctx *c, int *count)
{
  const int n = (int)c->n;
  if(c->sph_tlist.ensure((size_t)n) || c->sph_counters.ensure(SPH_C_COUNT + 1))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, (SPH_C_COUNT + 1) * sizeof(unsigned long long), c->stream));
  int *d_cnt = reinterpret_cast<int *>(c->sph_counters.p + SPH_C_COUNT);
  hipcub::CountingInputIterator<int> iota(0);
  SphIsTarget sel = {c->s_type.p, c->s_active.p};
  size_t bytes = 0;
  HIP_TRY(c, hipcub::DeviceSelect::If(nullptr, bytes, iota, c->sph_tlist.p, d_cnt, n, sel, c->stream));
  if(c->sph_tmp.ensure(bytes))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipcub::DeviceSelect::If(c->sph_tmp.p, bytes, iota, c->sph_tlist.p, d_cnt, n, sel, c->stream));
  HIP_TRY(c, hipMemcpyAsync(count, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

// k_sph_density over the nt targets of sph_tlist (sph_res, sph_row, sph_rounds are allocated), then its counters
static int sph_density_walk(ngravs_ctx *c, double des_num_ngb, double max_dev, double min_hsml, long long nt, SphStats *st)
{
  SphParams sp;
  sph_set_box(c, &sp);
  sp.des = des_num_ngb;
  sp.dev = max_dev;
  sp.minh = min_hsml;
  hipLaunchKernelGGL(k_sph_density, dim3(sph_wave_grid(nt, SPH_WAVES)), dim3(64 * SPH_WAVES), 0, c->stream, sph_tree_view(c), c->s_pm.p,
                     c->s_type.p, c->sph_vel.p, c->s_idx.p, c->sph_tlist.p, nt, (long long)c->n, c->sph_h_in.p, sp, c->sph_res.p, c->sph_row.p,
                     c->sph_rounds.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long h[SPH_C_COUNT];
  if(int rc = sph_read_counters(c, h))
    return rc;
  st->bad_hsml = (long long)h[SPH_C_BAD];
  st->failed = (long long)h[SPH_C_FAILED];
  st->stack_ovf = (long long)h[SPH_C_OVF];
  st->max_rounds = (long long)h[SPH_C_MAXR];
  st->sum_rounds = (long long)h[SPH_C_SUMR];
  st->candidates = (long long)h[SPH_C_CAND];
  st->neighbours = (long long)h[SPH_C_NGB];
  return NGRAVS_OK;
}

int sph_density_run(ngravs_ctx *c, double des_num_ngb, double max_dev, double min_hsml, SphStats *st)
{
  memset(st, 0, sizeof(*st));
  int cnt = 0;
  if(int rc = sph_targets(c, &cnt))
    return rc;
  st->targets = cnt;
  if(cnt == 0)
    return NGRAVS_OK;
  const long long nt = cnt;
  if(c->sph_res.ensure((size_t)SPH_NRES * nt) || c->sph_row.ensure((size_t)nt) || c->sph_rounds.ensure((size_t)nt))
    return NGRAVS_ERR_NOMEM;
  return sph_density_walk(c, des_num_ngb, max_dev, min_hsml, nt, st);
}

// ---- the first guess of the smoothing lengths (setup_smoothinglengths, init.c:229-247, 3-D branch) ----------------------------
// The reference climbs its GAS-ONLY tree (ngb_treebuild -> force_treebuild(N_gas), ngb.c:408) from Father[i] while
// 10 DesNumNgb m_i > mass(no).  The masses of nested cells never decrease going up, so the same cell is found from the root:
// descend along the cells containing i while the next one holds at least two gas particles (it is a node of the gas-only tree)
// and at least 10 DesNumNgb m_i of gas.  The device tree holds all types; a node is a contiguous range of the Peano-ordered rows,
// so its gas mass and gas count are differences of two values of an inclusive scan over (type == 0 ? mass : 0) and (type == 0).
// k_sph_gas_cols   : one thread per row: the two scan inputs, shifted by one ([0] = 0); counts type-0 rows with a bad mass
// k_sph_hsml_guess : one lane per listed gas row, Peano order (neighbouring lanes follow the same path and load the same nodes)
__global__ void k_sph_gas_cols(const double4 *__restrict__ pm, const unsigned char *__restrict__ type, long long n, double *__restrict__ gm,
                               int *__restrict__ gc, unsigned long long *__restrict__ counters)
{
  const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(p == 0)
    {
      gm[0] = 0;
      gc[0] = 0;
    }
  if(p >= n)
    return;
  const bool gas = type[p] == 0;
  const double m = pm[p].w;
  if(gas && !(m > 0 && m <= 1.79769313486231570e308))
    atomicAdd(&counters[SPH_C_BAD], 1ull);
  gm[p + 1] = gas ? m : 0.0;
  gc[p + 1] = gas ? 1 : 0;
}

struct SphIsUnsetGas
{
  const unsigned char *type;
  const unsigned int *idx;
  const double *h_in;   // caller order; null: every gas row
  __host__ __device__ __forceinline__ bool operator()(const int &i) const { return type[i] == 0 && !(h_in && h_in[idx[i]] > 0); }
};

#define SPH_GUESS_SUB 30   // halvings below a bucket: 21 + 30 bits of a coordinate are exact in a double and fit a long long

__global__ void k_sph_hsml_guess(const int *__restrict__ n_first, const int *__restrict__ n_count, const int *__restrict__ n_child,
                                 const int *__restrict__ n_flags, int nnodes, const double4 *__restrict__ pm,
                                 const unsigned char *__restrict__ type, const unsigned int *__restrict__ idx, const int *__restrict__ list,
                                 long long nl, long long n, const double *__restrict__ gm, const int *__restrict__ gc, double des, double cx,
                                 double cy, double cz, double fac21, double len0, double *__restrict__ res, int *__restrict__ row)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t >= nl)
    return;
  const long long p = list[t];
  if(p < 0 || p >= n)
    return;
  const double4 me = pm[p];
  const double thr = 10 * des * me.w;   // init.c:235
  int node = 0, level = 0;
  double mass = gm[n] - gm[0];          // the root is used even when it fails the mass test (init.c:239-240)
  while(level < TREE_BITS && !(n_flags[node] & FLAG_BUCKET))
    {
      int nxt = -1;
      long long f = 0, e = 0;
      for(int k = 0; k < 8; k++)
        {
          const int ch = n_child[8ll * node + k];
          if(ch < 0 || ch >= nnodes)
            continue;   // empty, or one particle: no node of the gas-only tree either
          const long long cf = n_first[ch], ce = cf + n_count[ch];
          if(p >= cf && p < ce && cf >= 0 && ce <= n)
            nxt = ch, f = cf, e = ce;
        }
      if(nxt < 0 || gc[e] - gc[f] < 2)
        break;
      const double m = gm[e] - gm[f];
      if(!(m >= thr))
        break;
      node = nxt;
      mass = m;
      level++;
    }
  if(n_flags[node] & FLAG_BUCKET)
    {
      // below the deepest device level the reference's gas-only tree may go on: halve the cell, keep the half that holds this
      // particle, with the tree build's own cell coordinates (k_keys) extended by exact powers of two
      const long long f = n_first[node], e = f + n_count[node];
      const double ux = __dmul_rn(__dsub_rn(me.x, cx), fac21), uy = __dmul_rn(__dsub_rn(me.y, cy), fac21),
                   uz = __dmul_rn(__dsub_rn(me.z, cz), fac21);
      for(int k = 1; k <= SPH_GUESS_SUB && f >= 0 && e <= n; k++)
        {
          const double s = (double)(1ll << k);
          const long long ix = (long long)(ux * s), iy = (long long)(uy * s), iz = (long long)(uz * s);
          int cnt = 0;
          double m = 0;
          for(long long q = f; q < e; q++)
            {
              if(type[q] != 0)
                continue;
              const double4 o = pm[q];
              if((long long)(__dmul_rn(__dsub_rn(o.x, cx), fac21) * s) == ix && (long long)(__dmul_rn(__dsub_rn(o.y, cy), fac21) * s) == iy &&
                 (long long)(__dmul_rn(__dsub_rn(o.z, cz), fac21) * s) == iz)
                {
                  cnt++;
                  m += o.w;
                }
            }
          if(cnt < 2 || !(m >= thr))
            break;
          mass = m;
          level = TREE_BITS + k;
        }
    }
  res[t] = cbrt(3.0 / (4 * M_PI) * des * me.w / mass) * ldexp(len0, -level);   // init.c:246-247
  row[t] = (int)idx[p];
}

int sph_hsml_guess_run(ngravs_ctx *c, double des_num_ngb, int only_unset, long long *rows, long long *bad_mass)
{
  const long long n = c->n;
  *rows = *bad_mass = 0;
  if(c->sph_tlist.ensure((size_t)n) || c->sph_counters.ensure(SPH_C_COUNT + 1) || c->sph_gmass.ensure((size_t)n + 1) ||
     c->sph_gcount.ensure((size_t)n + 1))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, (SPH_C_COUNT + 1) * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_sph_gas_cols, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->s_pm.p, c->s_type.p, n, c->sph_gmass.p,
                     c->sph_gcount.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  int *d_cnt = reinterpret_cast<int *>(c->sph_counters.p + SPH_C_COUNT);
  hipcub::CountingInputIterator<int> iota(0);
  SphIsUnsetGas sel = {c->s_type.p, c->s_idx.p, only_unset ? c->sph_h_in.p : nullptr};
  size_t b0 = 0, b1 = 0, b2 = 0;
  HIP_TRY(c, hipcub::DeviceSelect::If(nullptr, b0, iota, c->sph_tlist.p, d_cnt, (int)n, sel, c->stream));
  HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, b1, c->sph_gmass.p + 1, c->sph_gmass.p + 1, (int)n, c->stream));
  HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(nullptr, b2, c->sph_gcount.p + 1, c->sph_gcount.p + 1, (int)n, c->stream));
  const size_t bytes = b0 > b1 ? (b0 > b2 ? b0 : b2) : (b1 > b2 ? b1 : b2);
  if(c->sph_tmp.ensure(bytes))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipcub::DeviceSelect::If(c->sph_tmp.p, b0, iota, c->sph_tlist.p, d_cnt, (int)n, sel, c->stream));
  HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(c->sph_tmp.p, b1, c->sph_gmass.p + 1, c->sph_gmass.p + 1, (int)n, c->stream));
  HIP_TRY(c, hipcub::DeviceScan::InclusiveSum(c->sph_tmp.p, b2, c->sph_gcount.p + 1, c->sph_gcount.p + 1, (int)n, c->stream));
  unsigned long long h[SPH_C_COUNT + 1];
  HIP_TRY(c, hipMemcpyAsync(h, c->sph_counters.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  *bad_mass = (long long)h[SPH_C_BAD];
  int cnt;
  memcpy(&cnt, &h[SPH_C_COUNT], sizeof(int));
  if(*bad_mass || cnt <= 0)
    return NGRAVS_OK;   // the caller refuses, or there is nothing to write
  const long long nl = cnt;
  if(c->sph_res.ensure((size_t)nl) || c->sph_row.ensure((size_t)nl))
    return NGRAVS_ERR_NOMEM;
  const double fac21 = c->dom[7] * (double)(1 << (TREE_BITS - NGRAVS_BITS_PER_DIMENSION));
  hipLaunchKernelGGL(k_sph_hsml_guess, dim3((unsigned)((nl + 255) / 256)), dim3(256), 0, c->stream, c->n_first.p, c->n_count.p, c->n_child.p,
                     c->n_flags.p, (int)c->nnodes, c->s_pm.p, c->s_type.p, c->s_idx.p, c->sph_tlist.p, nl, n, c->sph_gmass.p, c->sph_gcount.p,
                     des_num_ngb, c->dom[0], c->dom[1], c->dom[2], fac21, c->dom[6], c->sph_res.p, c->sph_row.p);
  HIP_TRY(c, hipGetLastError());
  *rows = nl;
  return NGRAVS_OK;
}

// ---- SPH hydro force --------------------------------------------------------------------------------------------------------
// counters of a hydro call: type-0 rows with a bad Hsml / Density / Pressure, waves whose LIFO was full, candidates, pairs
#define SPH_H_BADH 0
#define SPH_H_BADRHO 1
#define SPH_H_BADP 3

// One gas particle's columns of sph_hsrc from its SphP values: what hydro_evaluate derives from one particle alone.  The one place
// these expressions stand, for k_sph_hydro_prep and k_sph_gas_prep.  Counts a bad Hsml / Density / Pressure; returns whether
// the row is good.
__device__ __forceinline__ bool sph_hydro_source(double *__restrict__ hs, long long n, long long p, double vx, double vy, double vz, double h,
                                                 double rho, double pressure, double dhsml, double div, double curl, double ts,
                                                 const SphHydroParams &hp, unsigned long long *__restrict__ counters)
{
  const double BIG = 1e300;
  const double adiv = fabs(div);
  bool good = true;
  if(!(h > 0) || !(h < BIG))
    {
      atomicAdd(&counters[SPH_H_BADH], 1ull);
      good = false;
    }
  if(!(rho > 0) || !(rho < BIG))
    {
      atomicAdd(&counters[SPH_H_BADRHO], 1ull);
      good = false;
    }
  if(!(pressure >= 0) || !(pressure < BIG))
    {
      atomicAdd(&counters[SPH_H_BADP], 1ull);
      good = false;
    }
  const double por2 = pressure / (rho * rho);                 // hydra.c:441
  const double cs_j = sqrt(hp.gamma * por2 * rho);            // hydra.c:442
  const double cs_i = sqrt(hp.gamma * pressure / rho);        // hydra.c:379
  hs[SPH_HS_VX * n + p] = vx;
  hs[SPH_HS_VY * n + p] = vy;
  hs[SPH_HS_VZ * n + p] = vz;
  hs[SPH_HS_H * n + p] = h;
  hs[SPH_HS_RHO * n + p] = rho;
  hs[SPH_HS_POR2 * n + p] = por2 * dhsml;                     // hydra.c:403, :524
  hs[SPH_HS_CSJ * n + p] = cs_j;
  hs[SPH_HS_F2 * n + p] = adiv / (adiv + curl + 0.0001 * cs_j / hp.fac_mu / h);   // hydra.c:504-506
  hs[SPH_HS_TS * n + p] = ts;
  hs[SPH_HS_CSI * n + p] = cs_i;
  hs[SPH_HS_F1 * n + p] = adiv / (adiv + curl + 0.0001 * cs_i / h / hp.fac_mu);   // hydra.c:380-382
  return good;
}

__global__ void k_sph_hydro_prep(const unsigned char *__restrict__ type, const unsigned int *__restrict__ idx, long long n,
                                 const double *__restrict__ vel_in, const double *__restrict__ h_in, const double *__restrict__ col_in,
                                 const int *__restrict__ ts_in, SphHydroParams hp, double *__restrict__ hs,
                                 unsigned long long *__restrict__ counters)
{
  const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(p >= n)
    return;
  if(type[p] != 0)
    {
      hs[SPH_HS_H * n + p] = 0;   // no gas: nothing for hmax, never staged
      return;
    }
  const long long row = idx[p];
  sph_hydro_source(hs, n, p, vel_in[3 * row], vel_in[3 * row + 1], vel_in[3 * row + 2], h_in[row], col_in[row], col_in[n + row],
                   col_in[2 * n + row], col_in[3 * n + row], col_in[4 * n + row], hp.have_ts ? (double)ts_in[row] : 0.0, hp, counters);
}

// ngravs_sph_accelerations, between its two walks: the pressure line of density() (density.c:305-308) for the targets, whose
// density results are read where k_sph_density left them (res, list order, through tpos: sorted position -> list index, -1 for a
// particle that is no target), and the hydro stage's sph_hsrc for every gas particle -- a target's from those results, another
// gas particle's from the caller's columns as k_sph_hydro_prep takes them.  vel is VelPred in Peano order (sph_vel).  A bad row
// gets Hsml 0 here: the call is refused after the walk, which must not open the whole tree for an infinite length meanwhile.
__global__ void k_sph_gas_prep(const unsigned char *__restrict__ type, const unsigned int *__restrict__ idx, const int *__restrict__ tpos,
                               long long n, long long nt, const double *__restrict__ vel, const double *__restrict__ h_in,
                               const double *__restrict__ col_in, const double *__restrict__ entropy, const double *__restrict__ dt_entropy,
                               const int *__restrict__ ti_beg, const int *__restrict__ ti_end, int ti_current, SphHydroParams hp,
                               double *__restrict__ res, double *__restrict__ hs, unsigned long long *__restrict__ counters)
{
  const long long p = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(p >= n)
    return;
  if(type[p] != 0)
    {
      hs[SPH_HS_H * n + p] = 0;   // no gas: nothing for hmax, never staged
      return;
    }
  const long long row = idx[p];
  const long long t = tpos[p];
  const int beg = hp.have_ts ? ti_beg[row] : 0, end = hp.have_ts ? ti_end[row] : 0;
  double h, rho, pressure, dhsml, div, curl;
  if(t >= 0 && t < nt)
    {
      h = res[SPH_HSML * nt + t], rho = res[SPH_DENSITY * nt + t], dhsml = res[SPH_DHSML * nt + t];
      div = res[SPH_DIVVEL * nt + t], curl = res[SPH_CURLVEL * nt + t];
      // density.c:305: the midpoint by the reference's integer division
      const double dt_entr = hp.have_ts ? (double)((long long)ti_current - ((long long)beg + end) / 2) * hp.tbi : 0.0;
      pressure = (entropy[row] + (dt_entropy ? dt_entropy[row] : 0.0) * dt_entr) * pow(rho, hp.gamma);   // density.c:307-308
      res[SPH_GAS_PRESSURE * nt + t] = pressure;
    }
  else
    {
      h = h_in[row], rho = col_in[row], pressure = col_in[n + row], dhsml = col_in[2 * n + row];
      div = col_in[3 * n + row], curl = col_in[4 * n + row];
    }
  if(!sph_hydro_source(hs, n, p, vel[3 * p], vel[3 * p + 1], vel[3 * p + 2], h, rho, pressure, dhsml, div, curl,
                       hp.have_ts ? (double)(end - beg) : 0.0, hp, counters))
    hs[SPH_HS_H * n + p] = 0;
}

// sorted position -> list index of the targets (tpos is -1 everywhere before)
__global__ void k_sph_tpos(const int *__restrict__ tlist, long long nt, long long n, int *__restrict__ tpos)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t < nt && tlist[t] >= 0 && tlist[t] < n)
    tpos[tlist[t]] = (int)t;
}

// force_update_hmax (forcetree.c:1134-1203, local part): the nodes of one level from their children, the levels bottom-up
__global__ void k_sph_hmax(const int *__restrict__ n_child, const int *__restrict__ n_first, const int *__restrict__ n_count,
                           const int *__restrict__ n_flags, const double *__restrict__ sh, long long n, int node0, int nnodes_level,
                           double *__restrict__ hmax)
{
  const int t = blockIdx.x * blockDim.x + threadIdx.x;
  if(t >= nnodes_level)
    return;
  const int node = node0 + t;
  double m = 0;
  if(n_flags[node] & FLAG_BUCKET)
    {
      const long long f = n_first[node], cnt = n_count[node];
      for(long long p = f; p < f + cnt && p < n; p++)
        m = fmax(m, sh[p]);
    }
  else
    for(int k = 0; k < 8; k++)
      {
        const int ch = n_child[8ll * node + k];
        if(ch >= 0)
          m = fmax(m, hmax[ch]);
        else if(ch <= -2)
          m = fmax(m, sh[-2 - ch]);
      }
  hmax[node] = m;
}

struct SphHydroLane
{
  double x, y, z, vx, vy, vz, mass;
  double h2, hinv, hinv4, rho, por2, cs, f1, ts;
  double ax, ay, az, dte, maxsig;
  unsigned ncand, npair;
};

// every lane over the staged block (hydra.c:412-536)
__device__ __forceinline__ void sph_hydro_block(const double (*__restrict__ s)[SPH_STAGE], int cnt, bool live, const SphHydroParams &hp,
                                                SphHydroLane &L)
{
  if(live)
    L.ncand += (unsigned)cnt;
  for(int j = 0; j < cnt; j++)
    {
      double dx = L.x - s[0][j], dy = L.y - s[1][j], dz = L.z - s[2][j];
      if(hp.periodic)
        {
          dx = nearest(dx, hp.box, hp.boxhalf);
          dy = nearest(dy, hp.box, hp.boxhalf);
          dz = nearest(dz, hp.box, hp.boxhalf);
        }
      const double r2 = dx * dx + dy * dy + dz * dz;
      const double h_j = s[7][j], h_j2 = h_j * h_j;
      if(live && (r2 < L.h2 || r2 < h_j2))
        {
          const double r = sqrt(r2);
          if(r > 0)
            {
              L.npair++;
              const double m_j = s[3][j], cs_j = s[10][j];
              const double dvx = L.vx - s[4][j], dvy = L.vy - s[5][j], dvz = L.vz - s[6][j];
              const double vdotr = dx * dvx + dy * dvy + dz * dvz;
              const double vdotr2 = hp.comoving ? vdotr + hp.hubble_a2 * r2 : vdotr;
              double dwk_i = 0, dwk_j = 0;
              if(r2 < L.h2)
                {
                  const double u = r * L.hinv;
                  dwk_i = u < 0.5 ? L.hinv4 * u * (SPH_KC3 * u - SPH_KC4) : L.hinv4 * SPH_KC6 * (1.0 - u) * (1.0 - u);
                }
              if(r2 < h_j2)
                {
                  const double hinv = 1.0 / h_j, hinv4 = hinv * hinv * hinv * hinv, u = r * hinv;
                  dwk_j = u < 0.5 ? hinv4 * u * (SPH_KC3 * u - SPH_KC4) : hinv4 * SPH_KC6 * (1.0 - u) * (1.0 - u);
                }
              if(L.cs + cs_j > L.maxsig)
                L.maxsig = L.cs + cs_j;
              double visc = 0;
              if(vdotr2 < 0)   // artificial viscosity
                {
                  const double mu_ij = hp.fac_mu * vdotr2 / r;   // negative
                  const double vsig = L.cs + cs_j - 3 * mu_ij;
                  if(vsig > L.maxsig)
                    L.maxsig = vsig;
                  const double rho_ij = 0.5 * (L.rho + s[8][j]);
                  visc = 0.25 * hp.visc * vsig * (-mu_ij) / rho_ij * (L.f1 + s[11][j]);
                  if(hp.limiter)   // the viscous acceleration must not be too large
                    {
                      const double dt = fmax(L.ts, s[12][j]) * hp.tbi;
                      if(dt > 0 && (dwk_i + dwk_j) < 0)
                        {
                          const double lim = 0.5 * hp.fac_vsic_fix * vdotr2 / (0.5 * (L.mass + m_j) * (dwk_i + dwk_j) * r * dt);
                          visc = visc < lim ? visc : lim;   // dmin
                        }
                    }
                }
              const double hfc_visc = 0.5 * m_j * visc * (dwk_i + dwk_j) / r;
              const double hfc = hfc_visc + m_j * (L.por2 * dwk_i + s[9][j] * dwk_j) / r;
              L.ax -= hfc * dx;
              L.ay -= hfc * dy;
              L.az -= hfc * dz;
              L.dte += 0.5 * hfc_visc * vdotr2;
            }
        }
    }
}

// One wave of the hydro walk, the body of k_sph_hydro and k_sph_hydro_sums: the hull of the lanes' positions, ONE sph_hull_walk in
// which a child is tested against the hull widened by max(largest h_i of the wave, hmax of the child) (ngb.c:146-177), the 13
// staged doubles of a source, sph_hydro_block, the counters.  The two kernels differ in where a lane's target comes from and where
// its results go: load(t, L) fills L for target t and returns its h, store(t, L) writes the five results.
template <class Load, class Store>
__device__ __forceinline__ void sph_hydro_wave(const TreeView &tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                               const double *__restrict__ hs, const double *__restrict__ hmax, long long nt, long long n,
                                               const SphHydroParams &hp, unsigned long long *__restrict__ counters, Load load, Store store)
{
  __shared__ double s_src[SPH_HWAVES][SPH_HFIELDS][SPH_STAGE];
  __shared__ int s_stack[SPH_HWAVES][SPH_STACK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * SPH_HWAVES + w) * 64 + lane;
  if(t - lane >= nt)   // the whole wave (no workgroup barrier anywhere below)
    return;
  double (*src)[SPH_STAGE] = s_src[w];
  int *stack = s_stack[w];
  const double *sh = hs + SPH_HS_H * n;

  const bool live = t < nt;
  SphHydroLane L = {};
  double h = 0;
  if(live)
    h = load(t, L);
  const SphHull H = sph_wave_hull(L.x, L.y, L.z, 0.0, live);
  const double hw = wave_uniform(wave_max(live ? h : 0.0));
  const bool ok = sph_hull_walk<SPH_STAGE>(
    tv, pm, type, n, hp.periodic, hp.box, hp.boxhalf, H, stack, lane,
    [&](int ch) { return fmax(hw, ch >= 0 ? hmax[ch] : sh[-2 - ch]) * (1 + 1e-12); },
    [&](int q, long long p) {
      const double4 pp = pm[p];
      src[0][q] = pp.x, src[1][q] = pp.y, src[2][q] = pp.z, src[3][q] = pp.w;
      src[4][q] = hs[SPH_HS_VX * n + p], src[5][q] = hs[SPH_HS_VY * n + p], src[6][q] = hs[SPH_HS_VZ * n + p];
      src[7][q] = hs[SPH_HS_H * n + p], src[8][q] = hs[SPH_HS_RHO * n + p], src[9][q] = hs[SPH_HS_POR2 * n + p];
      src[10][q] = hs[SPH_HS_CSJ * n + p], src[11][q] = hs[SPH_HS_F2 * n + p], src[12][q] = hs[SPH_HS_TS * n + p];
    },
    [&](int cnt) { sph_hydro_block(src, cnt, live, hp, L); });
  if(live && ok)
    store(t, L);
  sph_wave_counters<false>(lane, L.ncand, L.npair, 0, !ok, counters);
}

// targets: rows of sph_hsrc by sph_tlist; results [column][nt] by list position, dt_entropy through hydra.c:320
__global__ __launch_bounds__(64 * SPH_HWAVES) void k_sph_hydro(TreeView tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                                               const double *__restrict__ hs, const double *__restrict__ hmax,
                                                               const unsigned int *__restrict__ idx, const int *__restrict__ tlist,
                                                               long long nt, long long n, SphHydroParams hp, double *__restrict__ res,
                                                               int *__restrict__ row, unsigned long long *__restrict__ counters)
{
  sph_hydro_wave(
    tv, pm, type, hs, hmax, nt, n, hp, counters,
    [&](long long t, SphHydroLane &L) {
      const int i = tlist[t];
      const double4 p = pm[i];
      L.x = p.x, L.y = p.y, L.z = p.z, L.mass = p.w;
      L.vx = hs[SPH_HS_VX * n + i], L.vy = hs[SPH_HS_VY * n + i], L.vz = hs[SPH_HS_VZ * n + i];
      const double h = hs[SPH_HS_H * n + i];
      L.h2 = h * h;
      L.hinv = 1.0 / h;
      L.hinv4 = L.hinv * L.hinv * L.hinv * L.hinv;
      L.rho = hs[SPH_HS_RHO * n + i];
      L.por2 = hs[SPH_HS_POR2 * n + i];
      L.cs = hs[SPH_HS_CSI * n + i];
      L.f1 = hs[SPH_HS_F1 * n + i];
      L.ts = hs[SPH_HS_TS * n + i];
      return h;
    },
    [&](long long t, const SphHydroLane &L) {
      // final operations (hydra.c:320)
      const double gm1 = hp.gamma - 1;
      res[SPH_HY_ACCX * nt + t] = L.ax;
      res[SPH_HY_ACCY * nt + t] = L.ay;
      res[SPH_HY_ACCZ * nt + t] = L.az;
      res[SPH_HY_DTENTR * nt + t] = L.dte * (gm1 / (hp.hubble_a2 * pow(L.rho, gm1)));
      res[SPH_HY_MAXSIG * nt + t] = L.maxsig;
      row[t] = (int)idx[tlist[t]];
    });
}

// force_update_hmax from the Hsml column of sph_hsrc
static int sph_hmax_levels(ngravs_ctx *c)
{
  const long long n = c->n;
  for(int l = c->nlevels - 1; l >= 0; l--)
    {
      const long long l0 = c->level_start[l], lc = c->level_start[l + 1] - l0;
      if(lc <= 0)
        continue;
      hipLaunchKernelGGL(k_sph_hmax, dim3((unsigned)((lc + 127) / 128)), dim3(128), 0, c->stream, c->n_child.p, c->n_first.p, c->n_count.p,
                         c->n_flags.p, c->sph_hsrc.p + SPH_HS_H * n, n, (int)l0, (int)lc, c->sph_hmax.p);
    }
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}

// k_sph_hydro over the nt targets of sph_tlist: res [SPH_HY_NRES][nt] and sph_row in list order
static int sph_hydro_walk(ngravs_ctx *c, const SphHydroParams &hp, long long nt, double *res)
{
  hipLaunchKernelGGL(k_sph_hydro, dim3(sph_wave_grid(nt, SPH_HWAVES)), dim3(64 * SPH_HWAVES), 0, c->stream, sph_tree_view(c), c->s_pm.p,
                     c->s_type.p, c->sph_hsrc.p, c->sph_hmax.p, c->s_idx.p, c->sph_tlist.p, nt, (long long)c->n, hp, res, c->sph_row.p,
                     c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}

// the stack / candidates / pairs counters of a hydro walk or a sums walk, read back (waits for the stream)
template <class Stats> static int sph_walk_counters(ngravs_ctx *c, Stats *st)
{
  unsigned long long h[SPH_C_COUNT];
  if(int rc = sph_read_counters(c, h))
    return rc;
  st->stack_ovf = (long long)h[SPH_C_OVF];
  st->candidates = (long long)h[SPH_C_CAND];
  st->pairs = (long long)h[SPH_C_NGB];
  return NGRAVS_OK;
}

// The engine's own gas as hydro sources: sph_hsrc from the caller's columns (sph_vel_in, sph_h_in, sph_col_in, sph_ts_in) by
// k_sph_hydro_prep, and the counts of its bad rows in st.  The counters are clear when this is called; sph_hmax is allocated here
// and filled by sph_hmax_levels once the caller knows the rows are good.
static int sph_hydro_sources(ngravs_ctx *c, const SphHydroParams &hp, SphHydroStats *st)
{
  const long long n = c->n;
  if(c->sph_hsrc.ensure((size_t)SPH_HS_NCOL * n) || c->sph_hmax.ensure((size_t)c->nnodes))
    return NGRAVS_ERR_NOMEM;
  hipLaunchKernelGGL(k_sph_hydro_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->s_type.p, c->s_idx.p, n, c->sph_vel_in.p,
                     c->sph_h_in.p, c->sph_col_in.p, c->sph_ts_in.p, hp, c->sph_hsrc.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long h[SPH_C_COUNT];
  if(int rc = sph_read_counters(c, h))
    return rc;
  st->bad_hsml = (long long)h[SPH_H_BADH];
  st->bad_density = (long long)h[SPH_H_BADRHO];
  st->bad_pressure = (long long)h[SPH_H_BADP];
  return NGRAVS_OK;
}

int sph_hydro_run(ngravs_ctx *c, const SphHydroParams &hp, SphHydroStats *st)
{
  memset(st, 0, sizeof(*st));
  int cnt = 0;
  if(int rc = sph_targets(c, &cnt))   // (clears the counters)
    return rc;
  st->targets = cnt;
  if(cnt == 0)
    return NGRAVS_OK;
  const long long nt = cnt;
  if(c->sph_res.ensure((size_t)SPH_HY_NRES * nt) || c->sph_row.ensure((size_t)nt))
    return NGRAVS_ERR_NOMEM;
  if(int rc = sph_hydro_sources(c, hp, st))
    return rc;
  if(st->bad_hsml || st->bad_density || st->bad_pressure)
    return NGRAVS_OK;   // the caller refuses; nothing is walked with such a column
  if(int rc = sph_hmax_levels(c))
    return rc;
  if(int rc = sph_hydro_walk(c, hp, nt, c->sph_res.p))
    return rc;
  return sph_walk_counters(c, st);
}

// ---- the gas side in one call (ngravs_sph_accelerations): density(), its pressure line, force_update_hmax(), hydro_force() ----
// One target list, no host synchronisation between the stages but the read-back of the density walk's counters (MAXITER and the
// other error flags), after which nothing runs when one is set.  sph_res holds [SPH_GAS_NRES][targets]: the density columns, the
// pressure, the hydro columns.
int sph_gas_run(ngravs_ctx *c, const SphGasParams &gp, const SphHydroParams &hp, SphStats *ds, SphHydroStats *hs, hipEvent_t ev_density,
                hipEvent_t ev_prep)
{
  memset(ds, 0, sizeof(*ds));
  memset(hs, 0, sizeof(*hs));
  const long long n = c->n;
  int cnt = 0;
  if(int rc = sph_targets(c, &cnt))   // (clears the counters)
    return rc;
  ds->targets = hs->targets = cnt;
  if(cnt == 0)
    return NGRAVS_OK;
  const long long nt = cnt;
  if(c->sph_res.ensure((size_t)SPH_GAS_NRES * nt) || c->sph_row.ensure((size_t)nt) || c->sph_rounds.ensure((size_t)nt) ||
     c->sph_tpos.ensure((size_t)n) || c->sph_hsrc.ensure((size_t)SPH_HS_NCOL * n) || c->sph_hmax.ensure((size_t)c->nnodes))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemsetAsync(c->sph_tpos.p, 0xff, sizeof(int) * n, c->stream));   // -1
  hipLaunchKernelGGL(k_sph_tpos, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, c->sph_tlist.p, nt, n, c->sph_tpos.p);
  HIP_TRY(c, hipGetLastError());
  if(int rc = sph_density_walk(c, gp.des, gp.dev, gp.minh, nt, ds))
    return rc;
  HIP_TRY(c, hipEventRecord(ev_density, c->stream));
  if(ds->bad_hsml || ds->stack_ovf || ds->failed)
    return NGRAVS_OK;   // the caller refuses; nothing of the hydro stage runs
  // the hydro stage counts in the same words
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, SPH_C_COUNT * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_sph_gas_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, c->stream, c->s_type.p, c->s_idx.p, c->sph_tpos.p, n, nt,
                     c->sph_vel.p, c->sph_h_in.p, c->sph_col_in.p, c->sph_gas_in.p, gp.have_dte ? c->sph_gas_in.p + n : nullptr,
                     c->sph_ti_in.p, c->sph_ti_in.p + n, gp.ti_current, hp, c->sph_res.p, c->sph_hsrc.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  if(int rc = sph_hmax_levels(c))
    return rc;
  HIP_TRY(c, hipEventRecord(ev_prep, c->stream));
  if(int rc = sph_hydro_walk(c, hp, nt, c->sph_res.p + SPH_GAS_HYDRO * nt))
    return rc;
  unsigned long long h[SPH_C_COUNT];
  if(int rc = sph_read_counters(c, h))
    return rc;
  hs->bad_hsml = (long long)h[SPH_H_BADH];
  hs->bad_density = (long long)h[SPH_H_BADRHO];
  hs->bad_pressure = (long long)h[SPH_H_BADP];
  hs->stack_ovf = (long long)h[SPH_C_OVF];
  hs->candidates = (long long)h[SPH_C_CAND];
  hs->pairs = (long long)h[SPH_C_NGB];
  return NGRAVS_OK;
}

__global__ void k_sph_scatter(const int *__restrict__ row, long long nt, const double *__restrict__ src, unsigned char *__restrict__ dst,
                              long long stride)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t < nt)
    *reinterpret_cast<double *>(dst + row[t] * stride) = src[t];
}

// every wanted column of sph_res [SPH_GAS_NRES][nt] in one pass
__global__ void k_sph_scatter_cols(const int *__restrict__ row, long long nt, const double *__restrict__ res, SphScatterCols cols)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t >= nt)
    return;
  const long long r = row[t];
#pragma unroll
  for(int k = 0; k < SPH_GAS_NRES; k++)
    if(cols.dst[k])
      *reinterpret_cast<double *>(cols.dst[k] + r * cols.stride[k]) = res[k * nt + t];
}

int sph_scatter_cols(ngravs_ctx *c, long long nt, const SphScatterCols &cols)
{
  hipLaunchKernelGGL(k_sph_scatter_cols, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, c->sph_row.p, nt, c->sph_res.p, cols);
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}

int sph_scatter(ngravs_ctx *c, const double *src, long long nt, double *dst, long long stride)
{
  hipLaunchKernelGGL(k_sph_scatter, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, c->sph_row.p, nt, src,
                     reinterpret_cast<unsigned char *>(dst), stride);
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}

// ---- sums for targets that are not own rows (density_evaluate(j, 1), density.c:231-284; hydro_evaluate(j, 1), hydra.c:232-287) ---
// What the reference does for a particle it imported: partial sums over the LOCAL gas, unfinalised, for the owner to add up.  A
// target is a record in sph_tg_in, not a row of the tree; the same calls serve probe points (tracers, grids).
// k_sph_tg_prep : one thread per target: refuses a bad record, and clamps the position to the domain cube for the Peano key only (a
//      foreign target may lie outside the cube of the engine's own particles).  The targets are then sorted by that key, so that
//      the 64 lanes of a wave are neighbours in space whatever the caller's order was.
// k_sph_density_sums : sph_hull_walk for the hull of the lanes' search boxes, ONE round at the given h, sph_block per staged block;
//      the seven raw sums of density.c:531-575 go to the caller's index of the target, without density.c:296-303.
// k_sph_hydro_sums : the walk of k_sph_hydro for lanes that hold the reference's hydrodata_in (hydra.c:145-162); acc[3], dt_entropy
//      BEFORE hydra.c:320 and max_signal_vel.
// k_sph_density_update : the owner's side of one round, sph_density_update_one per target.
// No workgroup barrier, no atomics on results; a push that would not fit the LIFO ends the call, and sph_tg_res is not copied out.
#define SPH_T_BADPOS 4   // counter: targets whose position is not finite, or outside [0, BoxSize] in a periodic run

__global__ void k_sph_tg_prep(const double *__restrict__ tg, long long nt, int hydro, int periodic, double box, double cx, double cy, double cz,
                              double len, double *__restrict__ clamped, unsigned int *__restrict__ iota,
                              unsigned long long *__restrict__ counters)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t >= nt)
    return;
  const double BIG = 1e300;
  const double h = tg[SPH_TG_H * nt + t];
  if(!(h > 0) || !(h < BIG))
    atomicAdd(&counters[SPH_H_BADH], 1ull);
  if(hydro)
    {
      const double rho = tg[SPH_TG_RHO * nt + t], pressure = tg[SPH_TG_P * nt + t];
      if(!(rho > 0) || !(rho < BIG))
        atomicAdd(&counters[SPH_H_BADRHO], 1ull);
      if(!(pressure >= 0) || !(pressure < BIG))
        atomicAdd(&counters[SPH_H_BADP], 1ull);
    }
  const double corner[3] = {cx, cy, cz};
  bool bad = false;
  for(int k = 0; k < 3; k++)
    {
      const double x = tg[3 * t + k];
      if(!(fabs(x) < BIG) || (periodic && !(x >= 0 && x <= box)))
        bad = true;
      // inside the cube with a cell to spare: (x - corner) * DomainFac stays below 2^TREE_BITS
      clamped[3 * t + k] = fmin(fmax(x, corner[k]), corner[k] + len * (1 - 1e-6));
    }
  if(bad)
    atomicAdd(&counters[SPH_T_BADPOS], 1ull);
  iota[t] = (unsigned int)t;
}

__global__ __launch_bounds__(64 * SPH_WAVES) void k_sph_density_sums(TreeView tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                                                     const double *__restrict__ svel, long long n, const double *__restrict__ tg,
                                                                     const unsigned int *__restrict__ ord, long long nt, SphParams sp,
                                                                     double *__restrict__ res, unsigned long long *__restrict__ counters)
{
  __shared__ double s_src[SPH_WAVES][7][SPH_STAGE];
  __shared__ int s_stack[SPH_WAVES][SPH_STACK];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const long long t = ((long long)blockIdx.x * SPH_WAVES + w) * 64 + lane;
  if(t - lane >= nt)   // the whole wave (no workgroup barrier anywhere below)
    return;
  double (*src)[SPH_STAGE] = s_src[w];
  int *stack = s_stack[w];

  const bool live = t < nt;
  SphLane L = {};
  double h = 0;
  long long me = 0;
  if(live)
    {
      me = ord[t];
      L.x = tg[3 * me], L.y = tg[3 * me + 1], L.z = tg[3 * me + 2];
      L.vx = tg[3 * nt + 3 * me], L.vy = tg[3 * nt + 3 * me + 1], L.vz = tg[3 * nt + 3 * me + 2];
      h = tg[SPH_TG_H * nt + me];
      L.h2 = h * h;
      L.hinv = 1.0 / h;
      L.hinv3 = L.hinv * L.hinv * L.hinv;
      L.hinv4 = L.hinv3 * L.hinv;
    }
  const SphHull H = sph_wave_hull(L.x, L.y, L.z, h, live);   // of the lanes' search boxes, as in k_sph_density
  const bool ok = sph_hull_walk<SPH_STAGE>(
    tv, pm, type, n, sp.periodic, sp.box, sp.boxhalf, H, stack, lane, [](int) { return 0.0; },
    [&](int q, long long p) { sph_stage_density(src, q, p, pm, svel); }, [&](int cnt) { sph_block(src, cnt, live, sp, L); });
  if(live && ok)
    {
      double *r = res + SPH_NSUMS * me;   // the caller's order; NOT passed through density.c:296-303
      r[SPH_SUM_RHO] = L.rho;
      r[SPH_SUM_NGB] = L.wnn;
      r[SPH_SUM_DHR] = L.dhr;
      r[SPH_SUM_DIV] = L.divv;
      r[SPH_SUM_ROTX] = L.rx;
      r[SPH_SUM_ROTY] = L.ry;
      r[SPH_SUM_ROTZ] = L.rz;
    }
  sph_wave_counters<false>(lane, L.ncand, L.nngb, 0, !ok, counters);
}

// targets: records of sph_tg_in in the order ord; results [nt][5] by the caller's index, dt_entropy WITHOUT hydra.c:320
__global__ __launch_bounds__(64 * SPH_HWAVES) void k_sph_hydro_sums(TreeView tv, const double4 *__restrict__ pm, const unsigned char *__restrict__ type,
                                                                    const double *__restrict__ hs, const double *__restrict__ hmax, long long n,
                                                                    const double *__restrict__ tg, const int *__restrict__ tts,
                                                                    const unsigned int *__restrict__ ord, long long nt, SphHydroParams hp,
                                                                    double *__restrict__ res, unsigned long long *__restrict__ counters)
{
  sph_hydro_wave(
    tv, pm, type, hs, hmax, nt, n, hp, counters,
    [&](long long t, SphHydroLane &L) {
      // hydrodata_in (hydra.c:145-162), and what hydro_evaluate derives from it (hydra.c:379, :403)
      const long long me = ord[t];
      L.x = tg[3 * me], L.y = tg[3 * me + 1], L.z = tg[3 * me + 2];
      L.vx = tg[3 * nt + 3 * me], L.vy = tg[3 * nt + 3 * me + 1], L.vz = tg[3 * nt + 3 * me + 2];
      const double h = tg[SPH_TG_H * nt + me];
      L.mass = tg[SPH_TG_MASS * nt + me];
      L.h2 = h * h;
      L.hinv = 1.0 / h;
      L.hinv4 = L.hinv * L.hinv * L.hinv * L.hinv;
      L.rho = tg[SPH_TG_RHO * nt + me];
      const double pressure = tg[SPH_TG_P * nt + me];
      const double por2 = pressure / (L.rho * L.rho);
      L.por2 = por2 * tg[SPH_TG_DHSML * nt + me];
      L.cs = sqrt(hp.gamma * pressure / L.rho);
      L.f1 = tg[SPH_TG_F1 * nt + me];
      L.ts = tts ? (double)tts[me] : 0.0;
      return h;
    },
    [&](long long t, const SphHydroLane &L) {
      double *r = res + SPH_HY_NRES * (long long)ord[t];
      r[SPH_HY_ACCX] = L.ax;
      r[SPH_HY_ACCY] = L.ay;
      r[SPH_HY_ACCZ] = L.az;
      r[SPH_HY_DTENTR] = L.dte;
      r[SPH_HY_MAXSIG] = L.maxsig;
    });
}

// refuses bad targets (st says which), else leaves the caller's indices in Peano order in sph_tg_ord + nt
static int sph_targets_order(ngravs_ctx *c, long long nt, int hydro, SphSumsStats *st, bool *good)
{
  *good = false;
  double *clamped = c->sph_tg_in.p + (hydro ? SPH_TG_NCOL : SPH_TG_H + 1) * nt;
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, (SPH_C_COUNT + 1) * sizeof(unsigned long long), c->stream));
  hipLaunchKernelGGL(k_sph_tg_prep, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, c->sph_tg_in.p, nt, hydro, c->cfg.periodic,
                     c->cfg.box_size, c->dom[0], c->dom[1], c->dom[2], c->dom[6], clamped, c->sph_tg_ord.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long h[SPH_C_COUNT];
  if(int rc = sph_read_counters(c, h))
    return rc;
  st->bad_hsml = (long long)h[SPH_H_BADH];
  st->bad_density = (long long)h[SPH_H_BADRHO];
  st->bad_pressure = (long long)h[SPH_H_BADP];
  st->bad_pos = (long long)h[SPH_T_BADPOS];
  if(st->bad_hsml || st->bad_density || st->bad_pressure || st->bad_pos)
    return NGRAVS_OK;   // the caller refuses; nothing is walked for such a target
  const double fac21 = c->dom[7] * (double)(1 << (TREE_BITS - NGRAVS_BITS_PER_DIMENSION));
  if(int rc = dom_keys_only(c, clamped, nt, c->dom, fac21, TREE_BITS, reinterpret_cast<long long *>(c->sph_tg_key.p)))
    return rc;
  size_t bytes = 0;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(nullptr, bytes, c->sph_tg_key.p, c->sph_tg_key.p + nt, c->sph_tg_ord.p, c->sph_tg_ord.p + nt,
                                                (int)nt, 0, 3 * TREE_BITS, c->stream));
  if(c->sph_tmp.ensure(bytes))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipcub::DeviceRadixSort::SortPairs(c->sph_tmp.p, bytes, c->sph_tg_key.p, c->sph_tg_key.p + nt, c->sph_tg_ord.p,
                                                c->sph_tg_ord.p + nt, (int)nt, 0, 3 * TREE_BITS, c->stream));
  *good = true;
  return NGRAVS_OK;
}

int sph_density_sums_run(ngravs_ctx *c, long long nt, SphSumsStats *st)
{
  memset(st, 0, sizeof(*st));
  if(c->sph_counters.ensure(SPH_C_COUNT + 1) || c->sph_tg_key.ensure(2 * (size_t)nt) || c->sph_tg_ord.ensure(2 * (size_t)nt) ||
     c->sph_tg_res.ensure((size_t)SPH_NSUMS * nt))
    return NGRAVS_ERR_NOMEM;
  bool good;
  if(int rc = sph_targets_order(c, nt, 0, st, &good))
    return rc;
  if(!good)
    return NGRAVS_OK;
  SphParams sp = {};
  sph_set_box(c, &sp);
  hipLaunchKernelGGL(k_sph_density_sums, dim3(sph_wave_grid(nt, SPH_WAVES)), dim3(64 * SPH_WAVES), 0, c->stream, sph_tree_view(c), c->s_pm.p,
                     c->s_type.p, c->sph_vel.p, (long long)c->n, c->sph_tg_in.p, c->sph_tg_ord.p + nt, nt, sp, c->sph_tg_res.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  return sph_walk_counters(c, st);
}

int sph_hydro_sums_run(ngravs_ctx *c, const SphHydroParams &hp, long long nt, int have_tts, SphSumsStats *st, SphHydroStats *own)
{
  memset(st, 0, sizeof(*st));
  memset(own, 0, sizeof(*own));
  if(c->sph_counters.ensure(SPH_C_COUNT + 1) || c->sph_tg_key.ensure(2 * (size_t)nt) || c->sph_tg_ord.ensure(2 * (size_t)nt) ||
     c->sph_tg_res.ensure((size_t)SPH_HY_NRES * nt))
    return NGRAVS_ERR_NOMEM;
  // the engine's own gas first, as sph_hydro_run prepares it
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, (SPH_C_COUNT + 1) * sizeof(unsigned long long), c->stream));
  if(int rc = sph_hydro_sources(c, hp, own))
    return rc;
  if(own->bad_hsml || own->bad_density || own->bad_pressure)
    return NGRAVS_OK;   // the caller refuses; nothing is walked with such a column
  bool good;
  if(int rc = sph_targets_order(c, nt, 1, st, &good))   // (clears the counters)
    return rc;
  if(!good)
    return NGRAVS_OK;
  if(int rc = sph_hmax_levels(c))
    return rc;
  hipLaunchKernelGGL(k_sph_hydro_sums, dim3(sph_wave_grid(nt, SPH_HWAVES)), dim3(64 * SPH_HWAVES), 0, c->stream, sph_tree_view(c), c->s_pm.p,
                     c->s_type.p, c->sph_hsrc.p, c->sph_hmax.p, (long long)c->n, c->sph_tg_in.p, have_tts ? c->sph_tg_ts.p : nullptr,
                     c->sph_tg_ord.p + nt, nt, hp, c->sph_tg_res.p, c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  return sph_walk_counters(c, st);
}

__global__ void k_sph_density_update(long long n, const double *__restrict__ sums, double *__restrict__ h, double *__restrict__ left,
                                     double *__restrict__ right, int *__restrict__ rounds, double des, double dev, double minh,
                                     int *__restrict__ accepted, SphScatterCols out, unsigned long long *__restrict__ failed)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t >= n)
    return;
  double o[SPH_NRES];
  const int r = sph_density_update_one(sums + SPH_NSUMS * t, des, dev, minh, &h[t], &left[t], &right[t], &rounds[t], o);
  accepted[t] = r == 0;
  if(r == 0)
    {
#pragma unroll
      for(int k = 0; k < SPH_NRES; k++)
        if(out.dst[k])
          reinterpret_cast<double *>(out.dst[k])[t] = o[k];
    }
  else if(r == 2)
    atomicAdd(failed, 1ull);
}

int sph_density_update_device(long long n, const double *sums, double *h, double *left, double *right, int *rounds, double des, double dev,
                              double minh, int *accepted, double *const out[SPH_NRES], long long *failed)
{
  *failed = 0;
  DevBuf<unsigned long long> failed_buf;
  if(failed_buf.ensure(1))
    return NGRAVS_ERR_NOMEM;
  unsigned long long *d_failed = failed_buf.p;
  SphScatterCols cols = {};
  for(int k = 0; k < SPH_NRES; k++)
    cols.dst[k] = reinterpret_cast<unsigned char *>(out[k]);
  unsigned long long f = 0;
  hipError_t e = hipMemsetAsync(d_failed, 0, sizeof(unsigned long long), 0);
  if(e == hipSuccess)
    {
      hipLaunchKernelGGL(k_sph_density_update, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, 0, n, sums, h, left, right, rounds, des, dev, minh,
                         accepted, cols, d_failed);
      e = hipGetLastError();
    }
  if(e == hipSuccess)
    e = hipMemcpy(&f, d_failed, sizeof(f), hipMemcpyDeviceToHost);   // (waits for the kernel)
  if(e != hipSuccess)
    return NGRAVS_ERR_NO_DEVICE;
  *failed = (long long)f;
  return NGRAVS_OK;
}
