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
#include "engine.hpp"
#include "walk_device.hpp"
#include <hipcub/hipcub.hpp>

#define SPH_WAVES 4        // waves per workgroup: 4 x 8.2 KB of LDS, five workgroups per CU
#define SPH_STAGE 128      // entries of a wave's staging block: processed when more than 64 are in, so a chunk of 64 always fits
#define SPH_STACK 256      // depth-first with eight children per pop: at most 7 * MAX_LEVELS + 1 = 155 pending nodes
#define SPH_NLEAF 64       // a node with at most this many particles is staged whole (one chunk)
static_assert(7 * MAX_LEVELS + 8 < SPH_STACK, "the LIFO must hold a depth-first walk of the deepest tree");

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
      // the hull of the unconverged lanes' search boxes (ngb.c:206-210), a hair wider than the boxes' own rounding
      const double lx = wave_min(live ? L.x - h : BIG), ly = wave_min(live ? L.y - h : BIG), lz = wave_min(live ? L.z - h : BIG);
      const double ux = wave_max(live ? L.x + h : -BIG), uy = wave_max(live ? L.y + h : -BIG), uz = wave_max(live ? L.z + h : -BIG);
      const double hcx = wave_uniform(0.5 * (lx + ux)), hcy = wave_uniform(0.5 * (ly + uy)), hcz = wave_uniform(0.5 * (lz + uz));
      const double hhx = wave_uniform(0.5 * (ux - lx) * (1 + 1e-12)), hhy = wave_uniform(0.5 * (uy - ly) * (1 + 1e-12)),
                   hhz = wave_uniform(0.5 * (uz - lz) * (1 + 1e-12));
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
                  double dx = cx - hcx, dy = cy - hcy, dz = cz - hcz;
                  if(sp.periodic)
                    {
                      dx = nearest(dx, sp.box, sp.boxhalf);
                      dy = nearest(dy, sp.box, sp.boxhalf);
                      dz = nearest(dz, sp.box, sp.boxhalf);
                    }
                  // (ngb.c:272-297 for the hull instead of one particle's box)
                  if(fabs(dx) - half <= hhx && fabs(dy) - half <= hhy && fabs(dz) - half <= hhz)
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
                    {
                      const int q = fill + lane_prefix(m);
                      const double4 pp = pm[p];
                      src[0][q] = pp.x, src[1][q] = pp.y, src[2][q] = pp.z, src[3][q] = pp.w;
                      src[4][q] = svel[3 * p], src[5][q] = svel[3 * p + 1], src[6][q] = svel[3 * p + 2];
                    }
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
  // statistics: one set of atomics per wave
  unsigned long long cand = L.ncand, ngb = L.nngb, sumr = (unsigned long long)nr;
  int maxr = nr;
  for(int off = 32; off > 0; off >>= 1)
    {
      cand += __shfl_xor(cand, off);
      ngb += __shfl_xor(ngb, off);
      sumr += __shfl_xor(sumr, off);
      const int o = __shfl_xor(maxr, off);
      maxr = o > maxr ? o : maxr;
    }
  if(lane == 0)
    {
      atomicAdd(&counters[SPH_C_CAND], cand);
      atomicAdd(&counters[SPH_C_NGB], ngb);
      atomicAdd(&counters[SPH_C_SUMR], sumr);
      atomicMax(&counters[SPH_C_MAXR], (unsigned long long)maxr);
      if(ovf)
        atomicAdd(&counters[SPH_C_OVF], 1ull);
    }
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

int sph_density_run(ngravs_ctx *c, double des_num_ngb, double max_dev, double min_hsml, SphStats *st)
{
  memset(st, 0, sizeof(*st));
  const int n = (int)c->n;
  if(c->sph_tlist.ensure((size_t)n) || c->sph_counters.ensure(SPH_C_COUNT + 1))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemsetAsync(c->sph_counters.p, 0, (SPH_C_COUNT + 1) * sizeof(unsigned long long), c->stream));
  // the targets: active type-0 rows in Peano order (density.c:95, :123), compacted as the group walk's list is
  int *d_cnt = reinterpret_cast<int *>(c->sph_counters.p + SPH_C_COUNT);
  hipcub::CountingInputIterator<int> iota(0);
  SphIsTarget sel = {c->s_type.p, c->s_active.p};
  size_t bytes = 0;
  HIP_TRY(c, hipcub::DeviceSelect::If(nullptr, bytes, iota, c->sph_tlist.p, d_cnt, n, sel, c->stream));
  if(c->sph_tmp.ensure(bytes))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipcub::DeviceSelect::If(c->sph_tmp.p, bytes, iota, c->sph_tlist.p, d_cnt, n, sel, c->stream));
  int cnt = 0;
  HIP_TRY(c, hipMemcpyAsync(&cnt, d_cnt, sizeof(int), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  st->targets = cnt;
  if(cnt == 0)
    return NGRAVS_OK;
  const long long nt = cnt;
  if(c->sph_res.ensure((size_t)SPH_NRES * nt) || c->sph_row.ensure((size_t)nt) || c->sph_rounds.ensure((size_t)nt))
    return NGRAVS_ERR_NOMEM;
  SphParams sp;
  sp.periodic = c->cfg.periodic;
  sp.box = c->cfg.box_size;
  sp.boxhalf = 0.5 * c->cfg.box_size;
  sp.des = des_num_ngb;
  sp.dev = max_dev;
  sp.minh = min_hsml;
  const long long nwaves = (nt + 63) / 64;
  const unsigned nb = (unsigned)((nwaves + SPH_WAVES - 1) / SPH_WAVES);
  hipLaunchKernelGGL(k_sph_density, dim3(nb), dim3(64 * SPH_WAVES), 0, c->stream, sph_tree_view(c), c->s_pm.p, c->s_type.p, c->sph_vel.p,
                     c->s_idx.p, c->sph_tlist.p, nt, (long long)c->n, c->sph_h_in.p, sp, c->sph_res.p, c->sph_row.p, c->sph_rounds.p,
                     c->sph_counters.p);
  HIP_TRY(c, hipGetLastError());
  unsigned long long h[SPH_C_COUNT];
  HIP_TRY(c, hipMemcpyAsync(h, c->sph_counters.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  st->bad_hsml = (long long)h[SPH_C_BAD];
  st->failed = (long long)h[SPH_C_FAILED];
  st->stack_ovf = (long long)h[SPH_C_OVF];
  st->max_rounds = (long long)h[SPH_C_MAXR];
  st->sum_rounds = (long long)h[SPH_C_SUMR];
  st->candidates = (long long)h[SPH_C_CAND];
  st->neighbours = (long long)h[SPH_C_NGB];
  return NGRAVS_OK;
}

__global__ void k_sph_scatter(const int *__restrict__ row, long long nt, const double *__restrict__ src, unsigned char *__restrict__ dst,
                              long long stride)
{
  const long long t = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(t < nt)
    *reinterpret_cast<double *>(dst + row[t] * stride) = src[t];
}

int sph_scatter(ngravs_ctx *c, const double *src, long long nt, double *dst, long long stride)
{
  hipLaunchKernelGGL(k_sph_scatter, dim3((unsigned)((nt + 255) / 256)), dim3(256), 0, c->stream, c->sph_row.p, nt, src,
                     reinterpret_cast<unsigned char *>(dst), stride);
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}
