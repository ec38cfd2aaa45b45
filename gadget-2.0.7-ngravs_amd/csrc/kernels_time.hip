// kernels_time.hip -- time integration for one task: the stations of the reference's main loop (run.c:32-65) around the forces.
//
//   find_next_sync_point_and_drift   run.c:151-234       time_next_sync_point, time_move_particles
//   move_particles, do_box_wrapping  predict.c:31-133    k_move
//   find_dt_displacement_constraint  timestep.c:587-665  k_disp_sums + time_dt_displacement (host)
//   advance_and_find_timesteps       timestep.c:24-413   k_advance_decide, k_advance_apply
//   get_timestep                     timestep.c:427-576  k_advance_decide
//   init_drift_table, get_*_factor   driftfac.c:26-212   time_tables (host), time_factor (host and device)
//   compute_global_quantities_of_system  global.c:22-198 k_global_sums + k_global_final, time_global_finish (host)
//   energy_statistics                run.c:413-433       time_energy_line (host)
//
// Streaming kernels over the caller's own columns (pointer + byte stride per field, any layout): every byte is read once and written
// once per call, no intermediate column.  The calls keep no state: the context lends its stream, its fatal handler and one scratch
// buffer (counters, the decided steps, the tables, device copies of host columns).
#include "time_common.hpp"

struct TimeCounters
{
  int min_ti;
  unsigned flags;             // TF_*
  unsigned long long count;   // rows on the sync point / rows advanced
  long long row888, row818;   // lowest failing row of each fatal case
};
#define TF_BAD_TYPE 1u
#define TF_GAS_MISSING 2u
#define TF_ABOVE_MIN 4u

// ---- reductions: per wave by shuffles, per block through LDS, then one atomic (or one partial) per block ---------------------------
template <class T, class Op> __device__ inline T wave_reduce(T v, Op op)
{
  for(int o = 32; o > 0; o >>= 1)
    v = op(v, __shfl_xor(v, o));
  return v;
}
// the block's value in thread 0 (256 threads = 4 waves)
template <class T, class Op> __device__ inline T block_reduce(T v, Op op, T *lds4)
{
  v = wave_reduce(v, op);
  __syncthreads();
  if((threadIdx.x & 63) == 0)
    lds4[threadIdx.x >> 6] = v;
  __syncthreads();
  return op(op(lds4[0], lds4[1]), op(lds4[2], lds4[3]));
}
struct OpMin
{
  template <class T> __device__ T operator()(T a, T b) const { return a < b ? a : b; }
};
struct OpAdd
{
  template <class T> __device__ T operator()(T a, T b) const { return a + b; }
};
struct OpOr
{
  template <class T> __device__ T operator()(T a, T b) const { return a | b; }
};

#define TIME_BLOCK 256
#define TIME_MAX_GRID 1024
static unsigned time_grid(long long n)
{
  long long g = (n + TIME_BLOCK - 1) / TIME_BLOCK;
  return (unsigned)(g < 1 ? 1 : (g > TIME_MAX_GRID ? TIME_MAX_GRID : g));
}

// type in 0..5 in every row, and no type-0 row when a gas column is missing
__global__ __launch_bounds__(TIME_BLOCK) void k_time_check(TCol type, long long n, int gas_ok, TimeCounters *cnt)
{
  __shared__ unsigned lds[4];
  unsigned f = 0;
  for(long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TIME_BLOCK)
    {
      const int t = ldi(type, i);
      if(t < 0 || t >= NGRAVS_NTYPES)
        f |= TF_BAD_TYPE;
      if(t == 0 && !gas_ok)
        f |= TF_GAS_MISSING;
    }
  f = block_reduce(f, OpOr(), lds);
  if(threadIdx.x == 0 && f)
    atomicOr(&cnt->flags, f);
}

// ---- the sync point (run.c:161-191) --------------------------------------------------------------------------------------------------
__global__ __launch_bounds__(TIME_BLOCK) void k_sync_min(TCol tie, long long n, TimeCounters *cnt)
{
  __shared__ int lds[4];
  int m = 0x7fffffff;
  for(long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TIME_BLOCK)
    {
      const int t = ldi(tie, i);
      m = t < m ? t : m;
    }
  m = block_reduce(m, OpMin(), lds);
  if(threadIdx.x == 0)
    atomicMin(&cnt->min_ti, m);
}
__global__ __launch_bounds__(TIME_BLOCK) void k_sync_count(TCol tie, long long n, int pm_ti_endstep, TimeCounters *cnt)
{
  __shared__ unsigned long long lds[4];
  __shared__ unsigned ldsf[4];
  const int mn = cnt->min_ti;
  const int next = (pm_ti_endstep >= 0 && mn >= pm_ti_endstep) ? pm_ti_endstep : mn;
  unsigned long long k = 0;
  unsigned f = 0;
  for(long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TIME_BLOCK)
    {
      const int t = ldi(tie, i);
      k += t == next;
      if(t > mn)
        f = TF_ABOVE_MIN;
    }
  k = block_reduce(k, OpAdd(), lds);
  f = block_reduce(f, OpOr(), ldsf);
  if(threadIdx.x == 0)
    {
      if(k)
        atomicAdd(&cnt->count, k);
      if(f)
        atomicOr(&cnt->flags, f);
    }
}

// ---- the displacement sums (timestep.c:606-612): one partial of 18 numbers per block, added up in block order -----------------------
__global__ __launch_bounds__(TIME_BLOCK) void k_disp_sums(TCol type, TCol vel, TCol mass, long long n, double *partial, TimeCounters *cnt)
{
  __shared__ double lds[4];
  __shared__ unsigned ldsf[4];
  double v2[NGRAVS_NTYPES], mn[NGRAVS_NTYPES], ct[NGRAVS_NTYPES];
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    v2[t] = 0, mn[t] = 1.0e30, ct[t] = 0;
  unsigned f = 0;
  for(long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x; i < n; i += (long long)gridDim.x * TIME_BLOCK)
    {
      const int ty = ldi(type, i);
      const double x = ldd(vel, i, 0), y = ldd(vel, i, 1), z = ldd(vel, i, 2), m = ldd(mass, i);
      const double s = x * x + y * y + z * z;
      if(ty < 0 || ty >= NGRAVS_NTYPES)
        f = TF_BAD_TYPE;
#pragma unroll
      for(int t = 0; t < NGRAVS_NTYPES; t++)
        if(ty == t)
          {
            v2[t] += s;
            if(mn[t] > m)
              mn[t] = m;
            ct[t] += 1;
          }
    }
#pragma unroll
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    {
      const double a = block_reduce(v2[t], OpAdd(), lds);
      const double b = block_reduce(mn[t], OpMin(), lds);
      const double c = block_reduce(ct[t], OpAdd(), lds);
      if(threadIdx.x == 0)
        {
          partial[blockIdx.x * 18 + t] = a;
          partial[blockIdx.x * 18 + 6 + t] = b;
          partial[blockIdx.x * 18 + 12 + t] = c;
        }
    }
  f = block_reduce(f, OpOr(), ldsf);
  if(threadIdx.x == 0 && f)
    atomicOr(&cnt->flags, f);
}
__global__ void k_disp_final(const double *partial, int nblocks, double *out)
{
  const int k = threadIdx.x;
  if(k >= 18)
    return;
  double v = partial[k];
  for(int b = 1; b < nblocks; b++)
    {
      const double w = partial[b * 18 + k];
      v = (k >= 6 && k < 12) ? (w < v ? w : v) : v + w;
    }
  out[k] = v;
}

// ---- compute_global_quantities_of_system (global.c:52-114): 13 sums per type, one partial of 78 numbers per block ------------------
#define GQ_NK 13                        // mass, kinetic, internal, potential, momentum[3], angular momentum[3], mass x position[3]
#define GQ_NSUMS NGRAVS_GLOBAL_NSUMS    // GQ_NK per type
#define GQ_SPLIT 8                      // k_global_final: runs of TIME_MAX_GRID / GQ_SPLIT blocks
static_assert(GQ_NSUMS == GQ_NK * NGRAVS_NTYPES && TIME_MAX_GRID % GQ_SPLIT == 0 && GQ_NSUMS * GQ_SPLIT <= 1024, "k_global_final is one block");
struct GlobalParams
{
  TimeTabs tabs;
  double tbi, dt_pm, a1, a2, a3, gm1;   // dt_pm: the long-range half-step prediction (global.c:79-84), once per call on the host
  int ti_current, comoving, mesh, isotherm;
};
// A row's type is data, and 78 accumulators per lane are not to live in registers: they live in LDS as acc[k][type][lane], 64 lanes
// wide, 39 KiB for the block.  The block's four waves share the 64 lane columns and take turns on them with a barrier between the
// turns, so a cell is only ever touched by the one thread whose turn it is, and it sees its rows in the order (trip, wave) that the
// grid alone fixes.  Adding a row's terms is a read-add-write of 13 cells without a bank conflict (consecutive lanes, consecutive
// cells).  At the end each cell column is added up over the lanes by the shuffle tree, and the block stores its 78 numbers: no
// floating-point atomic anywhere, the same bits on every call with the same columns.  (Four blocks fill a CU's LDS: the launch bound
// asks for the four waves per SIMD that go with them.)
__global__ __launch_bounds__(TIME_BLOCK, 4) void k_global_sums(TCols c, TCol pot, GlobalParams p, int gas_ok, double *__restrict__ partial,
                                                            TimeCounters *cnt)
{
  __shared__ double acc[GQ_NSUMS * 64];
  __shared__ unsigned ldsf[4];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  for(int e = threadIdx.x; e < GQ_NSUMS * 64; e += TIME_BLOCK)
    acc[e] = 0;
  unsigned f = 0;
  const long long n = c.n;
  // (the trip count is the block's, not the thread's: there are barriers inside)
  for(long long base = blockIdx.x * (long long)TIME_BLOCK; base < n; base += (long long)gridDim.x * TIME_BLOCK)
    {
      const long long i = base + threadIdx.x;
      int ty = -1;   // no row, or a row that is refused
      double t[GQ_NK];
      if(i < n)
        {
          const int ty0 = ldi(c.c[TC_TYPE], i);
          if(ty0 < 0 || ty0 >= NGRAVS_NTYPES)
            f |= TF_BAD_TYPE;
          else if(ty0 == 0 && !gas_ok)
            f |= TF_GAS_MISSING;
          else
            {
              ty = ty0;
              const bool gas = ty == 0;
              const double m = ldd(c.c[TC_MASS], i);
              const int beg = ldi(c.c[TC_TIB], i), mid = (beg + ldi(c.c[TC_TIE], i)) / 2;
              const double dt_entr = (p.ti_current - mid) * p.tbi;   // global.c:58-68
              double dt_gravkick = dt_entr, dt_hydrokick = dt_entr;
              if(p.comoving)
                {
                  dt_gravkick = p.tabs.gravkick(beg, p.ti_current) - p.tabs.gravkick(beg, mid);
                  if(gas)
                    dt_hydrokick = p.tabs.hydrokick(beg, p.ti_current) - p.tabs.hydrokick(beg, mid);
                }
              double pos[3], vel[3];
              for(int j = 0; j < 3; j++)   // global.c:70-88
                {
                  pos[j] = ldd(c.c[TC_POS], i, j);
                  vel[j] = ldd(c.c[TC_VEL], i, j) + ldd(c.c[TC_GA], i, j) * dt_gravkick;
                  if(gas)
                    vel[j] += ldd(c.c[TC_HA], i, j) * dt_hydrokick;
                  if(p.mesh)
                    vel[j] += ldd(c.c[TC_GPM], i, j) * p.dt_pm;
                }
              t[0] = m;
              t[1] = 0.5 * m * (vel[0] * vel[0] + vel[1] * vel[1] + vel[2] * vel[2]) / p.a2;
              t[2] = 0;
              if(gas)   // global.c:76-77, 93-101
                {
                  const double entr = ldd(c.c[TC_ENT], i) + ldd(c.c[TC_DTE], i) * dt_entr;
                  t[2] = m * (p.isotherm ? entr : entr / p.gm1 * pow(ldd(c.c[TC_RHO], i) / p.a3, p.gm1));
                }
              t[3] = pot.p ? 0.5 * m * ldd(pot, i) / p.a1 : 0.0;
              for(int j = 0; j < 3; j++)
                {
                  t[4 + j] = m * vel[j];
                  t[10 + j] = m * pos[j];
                }
              t[7] = m * (pos[1] * vel[2] - pos[2] * vel[1]);
              t[8] = m * (pos[2] * vel[0] - pos[0] * vel[2]);
              t[9] = m * (pos[0] * vel[1] - pos[1] * vel[0]);
            }
        }
      for(int w = 0; w < TIME_BLOCK / 64; w++)
        {
          __syncthreads();
          if(w == wave && ty >= 0)
            {
              double *cell = acc + ty * 64 + lane;
#pragma unroll
              for(int k = 0; k < GQ_NK; k++)
                cell[k * NGRAVS_NTYPES * 64] += t[k];
            }
        }
    }
  __syncthreads();
  for(int e = wave; e < GQ_NSUMS; e += TIME_BLOCK / 64)
    {
      const double v = wave_reduce(acc[e * 64 + lane], OpAdd());
      if(lane == 0)
        partial[blockIdx.x * (long long)GQ_NSUMS + (e % NGRAVS_NTYPES) * GQ_NK + e / NGRAVS_NTYPES] = v;   // [type][k], as the caller gets it
    }
  f = block_reduce(f, OpOr(), ldsf);
  if(threadIdx.x == 0 && f)
    atomicOr(&cnt->flags, f);
}
// One block.  Thread (run, e) adds entry e of the blocks of its run in block order, then thread (0, e) adds the runs in their order:
// for up to TIME_MAX_GRID / GQ_SPLIT blocks that is the plain sum in block order, and always an order that the grid alone fixes.
__global__ __launch_bounds__(GQ_NSUMS *GQ_SPLIT) void k_global_final(const double *__restrict__ partial, int nblocks, double *__restrict__ out)
{
  __shared__ double runs[GQ_SPLIT * GQ_NSUMS];
  const int e = threadIdx.x % GQ_NSUMS, run = threadIdx.x / GQ_NSUMS;
  const int b0 = run * (TIME_MAX_GRID / GQ_SPLIT);
  const int b1 = b0 + TIME_MAX_GRID / GQ_SPLIT < nblocks ? b0 + TIME_MAX_GRID / GQ_SPLIT : nblocks;
  double v = 0;
  for(int b = b0; b < b1; b++)
    v += partial[b * GQ_NSUMS + e];
  runs[run * GQ_NSUMS + e] = v;
  __syncthreads();
  if(run == 0)
    {
      for(int r = 1; r < GQ_SPLIT; r++)
        v += runs[r * GQ_NSUMS + e];
      out[e] = v;
    }
}

// ---- move_particles (predict.c:31-76) and do_box_wrapping (predict.c:124-132) -------------------------------------------------------
struct MoveParams
{
  double dt_drift, dt_gravkick, dt_hydrokick;
  double tbi, min_gas_hsml, gamma, box;
  int time1, mesh, wrap;
};
// the two while loops of predict.c:127-131.  A coordinate that sixty-four steps do not bring home (or that no step moves: infinite,
// or beyond 2^53 boxes) is not looped over for ever: it is folded by floor, NaN and infinity are left as they are
__device__ inline double box_wrap(double x, double box)
{
  int guard = 0;
  while(x < 0 && guard++ < 64)
    x += box;
  while(x >= box && guard++ < 128)
    x -= box;
  if((x < 0 || x >= box) && isfinite(x))
    {
      x -= floor(x / box) * box;
      if(x >= box || x < 0)
        x = 0;
    }
  return x;
}
// WIDE: pos and vel are contiguous [n][3] and 16-byte aligned: the block's 256 rows are 768 consecutive doubles, moved as 384 double2
template <bool WIDE> __global__ __launch_bounds__(TIME_BLOCK) void k_move(TCols c, MoveParams p)
{
  const long long n = c.n;
  const long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x;
  if(WIDE)
    {
      const long long n3 = 3 * n;
      double *pos = reinterpret_cast<double *>(c.c[TC_POS].p);
      const double *vel = reinterpret_cast<const double *>(c.c[TC_VEL].p);
      for(int j = threadIdx.x; j < 3 * TIME_BLOCK / 2; j += TIME_BLOCK)
        {
          const long long e = blockIdx.x * (long long)(3 * TIME_BLOCK) + 2 * j;
          if(e + 1 < n3)
            {
              double2 x = *reinterpret_cast<const double2 *>(pos + e);
              const double2 v = *reinterpret_cast<const double2 *>(vel + e);
              x.x += v.x * p.dt_drift;
              x.y += v.y * p.dt_drift;
              if(p.wrap)
                x.x = box_wrap(x.x, p.box), x.y = box_wrap(x.y, p.box);
              *reinterpret_cast<double2 *>(pos + e) = x;
            }
          else if(e < n3)
            {
              double x = pos[e] + vel[e] * p.dt_drift;
              pos[e] = p.wrap ? box_wrap(x, p.box) : x;
            }
        }
    }
  if(i >= n)
    return;
  if(!WIDE)
    for(int j = 0; j < 3; j++)
      {
        double x = ldd(c.c[TC_POS], i, j) + ldd(c.c[TC_VEL], i, j) * p.dt_drift;
        sdd(c.c[TC_POS], i, j, p.wrap ? box_wrap(x, p.box) : x);
      }
  if(ldi(c.c[TC_TYPE], i) != 0)
    return;
  for(int j = 0; j < 3; j++)
    {
      double g = ldd(c.c[TC_GA], i, j);
      if(p.mesh)
        g += ldd(c.c[TC_GPM], i, j);
      sdd(c.c[TC_VP], i, j, ldd(c.c[TC_VP], i, j) + (g * p.dt_gravkick + ldd(c.c[TC_HA], i, j) * p.dt_hydrokick));
    }
  const double div = ldd(c.c[TC_DIV], i);
  const double rho = ldd(c.c[TC_RHO], i) * exp(-div * p.dt_drift);
  double h = ldd(c.c[TC_H], i) * exp(0.333333333333 * div * p.dt_drift);
  if(h < p.min_gas_hsml)
    h = p.min_gas_hsml;
  const double dt_entr = (p.time1 - (ldi(c.c[TC_TIB], i) + ldi(c.c[TC_TIE], i)) / 2) * p.tbi;
  sdd(c.c[TC_RHO], i, 0, rho);
  sdd(c.c[TC_H], i, 0, h);
  sdd(c.c[TC_PRES], i, 0, (ldd(c.c[TC_ENT], i) + ldd(c.c[TC_DTE], i) * dt_entr) * pow(rho, p.gamma));
}

// ---- advance_and_find_timesteps (timestep.c:24-413) ---------------------------------------------------------------------------------
struct AdvParams
{
  TimeTabs tabs;
  double fac1, fac2, fac3, hubble_a, atime, a3inv;   // timestep.c:48-61
  double soft[NGRAVS_NTYPES];                        // All.SofteningTable[]
  double eta, courant, scale, max_dt, min_dt, dt_disp, tbi, gamma, min_egy_spec;
  double dt_gravkickB;                               // timestep.c:70-76, with the PM step as it was on entry
  // the long-range kick (timestep.c:351-408), decided on the host
  double pm_dt_gravkick, pm_dt_gravkickB;
  int ti_current, comoving, mesh, adaptive, synchronization, stop, long_range;
};

// get_timestep (timestep.c:427-576) and the rules of timestep.c:190-253 for the rows on the sync point: step[i] = the new ti_step, or
// -1 for a row that is not advanced.  Writes nothing else; the lowest failing row of each fatal case goes to the counters.
__global__ __launch_bounds__(TIME_BLOCK) void k_advance_decide(TCols c, AdvParams p, int gas_ok, int *__restrict__ step, TimeCounters *cnt)
{
  __shared__ unsigned long long lds[4];
  __shared__ unsigned ldsf[4];
  const long long n = c.n;
  const long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x;
  unsigned f = 0;
  unsigned long long kicked = 0;
  if(i < n)
    {
      const int ty = ldi(c.c[TC_TYPE], i);
      int ti_step = -1;
      if(ty < 0 || ty >= NGRAVS_NTYPES)
        f |= TF_BAD_TYPE;
      else if(ty == 0 && !gas_ok)
        f |= TF_GAS_MISSING;
      else if(ldi(c.c[TC_TIE], i) == p.ti_current)
        {
          const int beg = ldi(c.c[TC_TIB], i), end = p.ti_current;
          double a[3];
          for(int j = 0; j < 3; j++)
            {
              a[j] = p.fac1 * ldd(c.c[TC_GA], i, j);
              if(p.mesh)
                a[j] += p.fac1 * ldd(c.c[TC_GPM], i, j);
              if(ty == 0)
                a[j] += p.fac2 * ldd(c.c[TC_HA], i, j);
            }
          double ac = sqrt(a[0] * a[0] + a[1] * a[1] + a[2] * a[2]);
          if(ac == 0)
            ac = 1.0e-30;
          ac *= p.scale;
          double dt = sqrt(2 * p.eta * p.atime * p.soft[ty] / ac);
          if(ty == 0)
            {
              const double h = ldd(c.c[TC_H], i), msv = ldd(c.c[TC_MSV], i);
              if(p.adaptive)
                dt = sqrt(2 * p.eta * p.atime * h / 2.8 / ac);
              const double dt_courant = p.comoving ? 2 * p.courant * p.atime * h / (p.fac3 * msv) : 2 * p.courant * h / msv;
              if(dt_courant < dt)
                dt = dt_courant;
            }
          dt *= p.hubble_a;
          if(dt >= p.max_dt)
            dt = p.max_dt;
          if(dt >= p.dt_disp)
            dt = p.dt_disp;
          bool ok = true;
          if(dt < p.min_dt)
            {
              if(p.stop)
                {
                  atomicMin(&cnt->row888, i);
                  ok = false;
                }
              dt = p.min_dt;
            }
          // ti_step = dt / Timebase_interval in (0, TIMEBASE), else endrun(818): decided on the quotient, which an int need not hold
          const double q = dt / p.tbi;
          if(ok && !(q >= 1.0 && q < (double)TI_BASE))
            {
              atomicMin(&cnt->row818, i);
              ok = false;
            }
          if(ok)
            {
              ti_step = 1 << (31 - __clz((int)q));   // the power-of-two floor (timestep.c:190-194)
              if(p.synchronization && ti_step > end - beg && ((TI_BASE - end) % ti_step) > 0)
                ti_step = end - beg;
              if(p.ti_current == TI_BASE)
                ti_step = 0;
              if(TI_BASE - p.ti_current < ti_step)
                ti_step = TI_BASE - p.ti_current;
              kicked = 1;
            }
        }
      step[i] = ti_step;
    }
  kicked = block_reduce(kicked, OpAdd(), lds);
  f = block_reduce(f, OpOr(), ldsf);
  if(threadIdx.x == 0)
    {
      if(kicked)
        atomicAdd(&cnt->count, kicked);
      if(f)
        atomicOr(&cnt->flags, f);
    }
}

// the kicks of timestep.c:255-326 for the rows k_advance_decide gave a step, then the long-range kick of timestep.c:384-407 for all rows
__global__ __launch_bounds__(TIME_BLOCK) void k_advance_apply(TCols c, AdvParams p, const int *__restrict__ step)
{
  const long long i = blockIdx.x * (long long)TIME_BLOCK + threadIdx.x;
  if(i >= c.n)
    return;
  const int ti_step = step[i];
  if(ti_step < 0 && !p.long_range)
    return;
  const int ty = ldi(c.c[TC_TYPE], i);
  double vel[3], ga[3], ha[3] = {0, 0, 0}, gpm[3] = {0, 0, 0}, vp[3];
  int beg = 0, end = 0;
  const bool gas = ty == 0;
  for(int j = 0; j < 3; j++)
    vel[j] = ldd(c.c[TC_VEL], i, j);
  if(p.mesh && (gas || p.long_range))
    for(int j = 0; j < 3; j++)
      gpm[j] = ldd(c.c[TC_GPM], i, j);
  if(ti_step >= 0 || gas)
    {
      for(int j = 0; j < 3; j++)
        ga[j] = ldd(c.c[TC_GA], i, j);
      beg = ldi(c.c[TC_TIB], i), end = ldi(c.c[TC_TIE], i);
      if(gas)
        for(int j = 0; j < 3; j++)
          ha[j] = ldd(c.c[TC_HA], i, j);
    }
  bool vp_new = false;
  if(ti_step >= 0)
    {
      const int tstart = (beg + end) / 2;        // midpoint of the old step
      const int tend = end + ti_step / 2;        // midpoint of the new step
      double dt_entr, dt_gravkick, dt_hydrokick, dt_gravkick2, dt_hydrokick2;
      if(p.comoving)
        {
          dt_entr = (tend - tstart) * p.tbi;
          dt_gravkick = p.tabs.gravkick(tstart, tend);
          dt_hydrokick = p.tabs.hydrokick(tstart, tend);
          dt_gravkick2 = p.tabs.gravkick(end, tend);
          dt_hydrokick2 = p.tabs.hydrokick(end, tend);
        }
      else
        {
          dt_entr = dt_gravkick = dt_hydrokick = (tend - tstart) * p.tbi;
          dt_gravkick2 = dt_hydrokick2 = (tend - end) * p.tbi;
        }
      beg = end;
      end = beg + ti_step;
      sdi(c.c[TC_TIB], i, beg);
      sdi(c.c[TC_TIE], i, end);
      for(int j = 0; j < 3; j++)
        vel[j] += ga[j] * dt_gravkick;
      if(gas)
        {
          for(int j = 0; j < 3; j++)
            {
              vel[j] += ha[j] * dt_hydrokick;
              vp[j] = vel[j] - dt_gravkick2 * ga[j] - dt_hydrokick2 * ha[j];
              if(p.mesh)
                vp[j] += gpm[j] * p.dt_gravkickB;
            }
          vp_new = true;
          double ent = ldd(c.c[TC_ENT], i), dte = ldd(c.c[TC_DTE], i);
          // cooling takes at most half of the entropy
          if(dte * dt_entr > -0.5 * ent)
            ent += dte * dt_entr;
          else
            ent *= 0.5;
          if(p.min_egy_spec != 0)
            {
              const double minentropy = p.min_egy_spec * (p.gamma - 1) / pow(ldd(c.c[TC_RHO], i) * p.a3inv, p.gamma - 1);
              if(ent < minentropy)
                {
                  ent = minentropy;
                  dte = 0;
                }
            }
          // no over-cooling in the prediction over the first half of the new step
          dt_entr = ti_step / 2 * p.tbi;
          if(ent + dte * dt_entr < 0.5 * ent)
            dte = -0.5 * ent / dt_entr;
          sdd(c.c[TC_ENT], i, 0, ent);
          sdd(c.c[TC_DTE], i, 0, dte);
        }
    }
  if(p.long_range)
    {
      for(int j = 0; j < 3; j++)
        vel[j] += gpm[j] * p.pm_dt_gravkick;
      if(gas)
        {
          double dt_gravkickA, dt_hydrokick;
          if(p.comoving)
            {
              dt_gravkickA = p.tabs.gravkick(beg, p.ti_current) - p.tabs.gravkick(beg, (beg + end) / 2);
              dt_hydrokick = p.tabs.hydrokick(beg, p.ti_current) - p.tabs.hydrokick(beg, (beg + end) / 2);
            }
          else
            dt_gravkickA = dt_hydrokick = (p.ti_current - (beg + end) / 2) * p.tbi;
          for(int j = 0; j < 3; j++)
            vp[j] = vel[j] + ga[j] * dt_gravkickA + ha[j] * dt_hydrokick + gpm[j] * p.pm_dt_gravkickB;
          vp_new = true;
        }
    }
  for(int j = 0; j < 3; j++)
    sdd(c.c[TC_VEL], i, j, vel[j]);
  if(vp_new)
    for(int j = 0; j < 3; j++)
      sdd(c.c[TC_VP], i, j, vp[j]);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static int time_read_counters(ngravs_ctx *c, const TimeCounters *dev, TimeCounters *h)
{
  HIP_TRY(c, hipMemcpyAsync(h, dev, sizeof(TimeCounters), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}
static int time_clear_counters(ngravs_ctx *c, TimeCounters *dev)
{
  TimeCounters z;
  z.min_ti = 0x7fffffff;
  z.flags = 0;
  z.count = 0;
  z.row888 = z.row818 = 0x7fffffffffffffffll;
  HIP_TRY(c, hipMemcpyAsync(dev, &z, sizeof z, hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));   // (z is on the stack)
  return NGRAVS_OK;
}
static int time_flags_outcome(const Refuse &refuse, unsigned flags)
{
  if(flags & TF_BAD_TYPE)
    return refuse(NGRAVS_ERR_ARG, "a type outside 0..5");
  if(flags & TF_GAS_MISSING)
    return refuse(NGRAVS_ERR_ARG, "there is a type-0 row, but not every gas column of this call was given");
  return NGRAVS_OK;
}
// -- the tables (driftfac.c:26-60, integrands :179-212) --
static void gauss_legendre(int n, double *x, double *w)
{
  for(int i = 0; i < n; i++)
    {
      double z = cos(M_PI * (i + 0.75) / (n + 0.5)), pp = 1;
      for(int it = 0; it < 100; it++)
        {
          double p1 = 1, p2 = 0;
          for(int j = 0; j < n; j++)
            {
              const double p3 = p2;
              p2 = p1;
              p1 = ((2.0 * j + 1.0) * z * p2 - j * p3) / (j + 1);
            }
          pp = n * (z * p1 - p2) / (z * z - 1);
          const double z1 = z;
          z = z1 - p1 / pp;
          if(fabs(z - z1) < 1e-16)
            break;
        }
      x[i] = z;
      w[i] = 2 / ((1 - z * z) * pp * pp);
    }
}
int time_tables(const ngravs_time_params_t *par, int rule, double *drift, double *gravkick, double *hydrokick)
{
  if(!(par->time_begin > 0) || !(par->time_max > par->time_begin) || !(par->hubble > 0) || !(par->gamma >= 1) || (rule != 0 && rule != 1))
    return NGRAVS_ERR_ARG;
  enum { NQ = 12 };
  double x[NQ], w[NQ];
  gauss_legendre(NQ, x, w);
  const double ltb = log(par->time_begin), ltm = log(par->time_max);
  const int panels = rule == 0 ? 1 : 2;
  double sum[3] = {0, 0, 0};
  for(int i = 0; i < TT_LEN; i++)
    {
      const double l0 = ltb + ((ltm - ltb) / TT_LEN) * i, l1 = ltb + ((ltm - ltb) / TT_LEN) * (i + 1);
      for(int q = 0; q < panels; q++)
        {
          const double a = l0 + (l1 - l0) * q / panels, b = l0 + (l1 - l0) * (q + 1) / panels;
          double s[3] = {0, 0, 0};
          for(int k = 0; k < NQ; k++)
            {
              const double aa = exp(0.5 * (a + b) + 0.5 * (b - a) * x[k]);
              double h = par->omega0 / (aa * aa * aa) + (1 - par->omega0 - par->omega_lambda) / (aa * aa) + par->omega_lambda;
              h = par->hubble * sqrt(h);
              // da = a d(log a)
              s[0] += w[k] * aa / (h * aa * aa * aa);
              s[1] += w[k] * aa / (h * aa * aa);
              s[2] += w[k] * aa / (h * pow(aa, 3 * (par->gamma - 1)) * aa);
            }
          for(int t = 0; t < 3; t++)
            sum[t] += 0.5 * (b - a) * s[t];
        }
      drift[i] = sum[0];
      gravkick[i] = sum[1];
      hydrokick[i] = sum[2];
    }
  return NGRAVS_OK;
}
int time_factors(const ngravs_time_params_t *par, int ti0, int ti1, double out[3])
{
  if(!par->drift_table || !par->gravkick_table || !par->hydrokick_table || !(par->time_begin > 0) || !(par->time_max > par->time_begin) ||
     !(par->timebase_interval > 0))
    return NGRAVS_ERR_ARG;
  const double ltb = log(par->time_begin), ltm = log(par->time_max);
  out[0] = time_factor(par->drift_table, ltb, ltm, par->timebase_interval, ti0, ti1);
  out[1] = time_factor(par->gravkick_table, ltb, ltm, par->timebase_interval, ti0, ti1);
  out[2] = time_factor(par->hydrokick_table, ltb, ltm, par->timebase_interval, ti0, ti1);
  return NGRAVS_OK;
}

static double time_hubble_a(const ngravs_time_params_t *par, double a)
{
  const double h = par->omega0 / (a * a * a) + (1 - par->omega0 - par->omega_lambda) / (a * a) + par->omega_lambda;
  return par->hubble * sqrt(h);
}

// find_dt_displacement_constraint after its sums (timestep.c:595-659)
int time_dt_displacement(const ngravs_time_params_t *par, const double sums[18], double G, double asmth, double time, double *out)
{
  double dt_displacement = par->max_size_timestep;
  if(par->comoving)
    {
      if(!(time > 0) || !(G > 0) || !(par->hubble > 0))
        return NGRAVS_ERR_ARG;
      const double hfac = time_hubble_a(par, time) * time * time;
      for(int type = 0; type < 6; type++)
        if(sums[12 + type] > 0)
          {
            const double min_mass = sums[6 + type], v_sum = sums[type], count_sum = sums[12 + type];
            double dmean;
            if(type == 0)
              dmean = pow(min_mass / (par->omega_baryon * 3 * par->hubble * par->hubble / (8 * M_PI * G)), 1.0 / 3);
            else
              dmean = pow(min_mass / ((par->omega0 - par->omega_baryon) * 3 * par->hubble * par->hubble / (8 * M_PI * G)), 1.0 / 3);
            double dt = par->max_rms_displacement_fac * hfac * dmean / sqrt(v_sum / count_sum);
            if(asmth > 0 && asmth < dmean)
              dt = par->max_rms_displacement_fac * hfac * asmth / sqrt(v_sum / count_sum);
            if(dt < dt_displacement)
              dt_displacement = dt;
          }
    }
  *out = dt_displacement;
  return NGRAVS_OK;
}

int time_next_sync_point(ngravs_ctx *c, const ngravs_time_cols_t *cols, int pm_ti_endstep, ngravs_sync_t *out)
{
  const Refuse refuse = {c, "ngravs_next_sync_point"};
  if(!cols || !out)
    return refuse(NGRAVS_ERR_ARG, "cols and out must not be NULL");
  if(cols->n <= 0)
    return refuse(NGRAVS_ERR_ARG, "n must be > 0: there is no minimum of no rows");
  TimeStage st = {c, cols};
  int rc;
  if((rc = st.begin(refuse, TB(TC_TIE), 0, sizeof(TimeCounters))))
    return rc;
  TimeCounters *cnt = reinterpret_cast<TimeCounters *>(st.scratch), h;
  if((rc = time_clear_counters(c, cnt)))
    return rc;
  const long long n = cols->n;
  hipLaunchKernelGGL(k_sync_min, dim3(time_grid(n)), dim3(TIME_BLOCK), 0, c->stream, st.d.c[TC_TIE], n, cnt);
  hipLaunchKernelGGL(k_sync_count, dim3(time_grid(n)), dim3(TIME_BLOCK), 0, c->stream, st.d.c[TC_TIE], n, pm_ti_endstep, cnt);
  HIP_TRY(c, hipGetLastError());
  if((rc = time_read_counters(c, cnt, &h)))
    return rc;
  const bool pm_rule = pm_ti_endstep >= 0 && h.min_ti >= pm_ti_endstep;
  out->ti_next = pm_rule ? pm_ti_endstep : h.min_ti;
  out->full_step = pm_rule || !(h.flags & TF_ABOVE_MIN);
  out->n_active = (int64_t)h.count;
  return NGRAVS_OK;
}

int time_displacement_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, double sums[18])
{
  const Refuse refuse = {c, "ngravs_displacement_sums"};
  if(!cols || !sums)
    return refuse(NGRAVS_ERR_ARG, "cols and sums must not be NULL");
  const size_t off_part = up256(sizeof(TimeCounters)), off_out = off_part + up256(sizeof(double) * 18 * TIME_MAX_GRID);
  TimeStage st = {c, cols};
  int rc;
  if((rc = st.begin(refuse, TB(TC_TYPE) | TB(TC_VEL) | TB(TC_MASS), 0, off_out + 256)))
    return rc;
  TimeCounters *cnt = reinterpret_cast<TimeCounters *>(st.scratch), h;
  double *partial = reinterpret_cast<double *>(st.scratch + off_part), *dout = reinterpret_cast<double *>(st.scratch + off_out);
  if((rc = time_clear_counters(c, cnt)))
    return rc;
  const long long n = cols->n;
  const unsigned grid = time_grid(n);
  hipLaunchKernelGGL(k_disp_sums, dim3(grid), dim3(TIME_BLOCK), 0, c->stream, st.d.c[TC_TYPE], st.d.c[TC_VEL], st.d.c[TC_MASS], n, partial, cnt);
  hipLaunchKernelGGL(k_disp_final, dim3(1), dim3(64), 0, c->stream, partial, (int)grid, dout);
  HIP_TRY(c, hipGetLastError());
  double hs[18];
  HIP_TRY(c, hipMemcpyAsync(hs, dout, sizeof hs, hipMemcpyDeviceToHost, c->stream));
  if((rc = time_read_counters(c, cnt, &h)) || (rc = time_flags_outcome(refuse, h.flags)))
    return rc;
  memcpy(sums, hs, sizeof hs);
  return NGRAVS_OK;
}

// compute_global_quantities_of_system up to its MPI_Reduce (global.c:32-114): the task's 78 sums
int time_global_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int ti_current, const int32_t *pm_ti,
                     const double *potential, int64_t potential_stride, double sums[GQ_NSUMS])
{
  const Refuse refuse = {c, "ngravs_global_sums"};
  if(!cols || !sums)
    return refuse(NGRAVS_ERR_ARG, "cols and sums must not be NULL");
  int rc;
  if((rc = time_params_check(refuse, par)))
    return rc;
  const int mesh = c->cfg.pmgrid > 0;
  if(mesh && !pm_ti)
    return refuse(NGRAVS_ERR_ARG, "a configuration with a mesh needs pm_ti");
  if(ti_current < 0 || ti_current > TI_BASE)
    return refuse(NGRAVS_ERR_ARG, "ti_current outside the integer time line");
  if(mesh && (pm_ti[0] < 0 || pm_ti[1] < pm_ti[0] || pm_ti[1] > TI_BASE))
    return refuse(NGRAVS_ERR_ARG, "pm_ti is not a step on the integer time line");
  const long long n = cols->n;
  if(potential && potential_stride < (int64_t)sizeof(double) && n > 1)
    return refuse(NGRAVS_ERR_ARG, "potential_stride is smaller than the field");
  const bool pot_staged = potential && !cols->on_device;
  const size_t off_tab = up256(sizeof(TimeCounters)), off_part = off_tab + up256(sizeof(double) * 3 * TT_LEN),
               off_out = off_part + up256(sizeof(double) * GQ_NSUMS * TIME_MAX_GRID), off_pot = off_out + up256(sizeof(double) * GQ_NSUMS);
  TimeStage st = {c, cols};
  if((rc = st.begin(refuse, TB(TC_TYPE) | TB(TC_POS) | TB(TC_VEL) | TB(TC_MASS) | TB(TC_TIB) | TB(TC_TIE) | TB(TC_GA) | (mesh ? TB(TC_GPM) : 0),
                    TB(TC_HA) | TB(TC_ENT) | TB(TC_DTE) | TB(TC_RHO), off_pot + (pot_staged ? sizeof(double) * (size_t)n : 0))))
    return rc;
  if(n == 0)   // a task that owns no rows
    {
      memset(sums, 0, sizeof(double) * GQ_NSUMS);
      return NGRAVS_OK;
    }
  TimeCounters *cnt = reinterpret_cast<TimeCounters *>(st.scratch), h;
  double *dtab = reinterpret_cast<double *>(st.scratch + off_tab), *partial = reinterpret_cast<double *>(st.scratch + off_part),
         *dout = reinterpret_cast<double *>(st.scratch + off_out);
  TCol pot = {nullptr, 0};
  if(pot_staged)
    {
      if((rc = col_upload(c, potential, potential_stride, sizeof(double), 1, n, 0, st.scratch + off_pot)))
        return rc;
      pot.p = st.scratch + off_pot, pot.stride = sizeof(double);
    }
  else if(potential)
    pot.p = reinterpret_cast<unsigned char *>(const_cast<double *>(potential)), pot.stride = potential_stride;

  GlobalParams p;
  memset(&p, 0, sizeof p);
  p.tabs = time_host_tabs(par, dtab);
  p.tbi = par->timebase_interval;
  p.a1 = p.a2 = p.a3 = 1;
  p.gm1 = par->gamma - 1;
  p.isotherm = par->gamma == 1;
  p.ti_current = ti_current;
  p.comoving = par->comoving != 0;
  p.mesh = mesh;
  if(par->comoving)
    {
      const double *tab[3] = {par->drift_table, par->gravkick_table, par->hydrokick_table};
      for(int k = 0; k < 3; k++)
        if((rc = col_upload(c, tab[k], sizeof(double), sizeof(double), 1, TT_LEN, 0, dtab + k * TT_LEN)))
          return rc;
      const double time = par->time_begin * exp(ti_current * par->timebase_interval);   // All.Time (run.c:231-234)
      p.a1 = time, p.a2 = time * time, p.a3 = time * time * time;
    }
  if(mesh)   // global.c:79-84
    {
      const TimeTabs hg = time_host_tabs(par, par->gravkick_table);
      const int pmb = pm_ti[0], mid = (pm_ti[0] + pm_ti[1]) / 2;
      if(par->comoving)
        p.dt_pm = time_factor(hg.t, hg.ltb, hg.ltm, hg.tbi, pmb, ti_current) - time_factor(hg.t, hg.ltb, hg.ltm, hg.tbi, pmb, mid);
      else
        p.dt_pm = (ti_current - mid) * par->timebase_interval;
    }
  if((rc = time_clear_counters(c, cnt)))
    return rc;
  const unsigned grid = time_grid(n);
  hipLaunchKernelGGL(k_global_sums, dim3(grid), dim3(TIME_BLOCK), 0, c->stream, st.d, pot, p, st.gas_ok, partial, cnt);
  hipLaunchKernelGGL(k_global_final, dim3(1), dim3(GQ_NSUMS * GQ_SPLIT), 0, c->stream, partial, (int)grid, dout);
  HIP_TRY(c, hipGetLastError());
  double hs[GQ_NSUMS];
  HIP_TRY(c, hipMemcpyAsync(hs, dout, sizeof hs, hipMemcpyDeviceToHost, c->stream));
  if((rc = time_read_counters(c, cnt, &h)) || (rc = time_flags_outcome(refuse, h.flags)))
    return rc;
  memcpy(sums, hs, sizeof hs);
  return NGRAVS_OK;
}

// compute_global_quantities_of_system after its MPI_Reduce (global.c:130-194), in the reference's order of operations
int time_global_finish(const double sums[GQ_NSUMS], ngravs_sysstate_t *out)
{
#pragma clang fp contract(off)
  ngravs_sysstate_t s;
  memset(&s, 0, sizeof s);
  for(int i = 0; i < 6; i++)
    {
      const double *t = sums + GQ_NK * i;
      s.MassComp[i] = t[0], s.EnergyKinComp[i] = t[1], s.EnergyIntComp[i] = t[2], s.EnergyPotComp[i] = t[3];
      for(int j = 0; j < 3; j++)
        s.MomentumComp[i][j] = t[4 + j], s.AngMomentumComp[i][j] = t[7 + j], s.CenterOfMassComp[i][j] = t[10 + j];
      s.EnergyTotComp[i] = s.EnergyKinComp[i] + s.EnergyPotComp[i] + s.EnergyIntComp[i];
    }
  for(int i = 0; i < 6; i++)
    {
      s.Mass += s.MassComp[i];
      s.EnergyKin += s.EnergyKinComp[i];
      s.EnergyPot += s.EnergyPotComp[i];
      s.EnergyInt += s.EnergyIntComp[i];
      s.EnergyTot += s.EnergyTotComp[i];
      for(int j = 0; j < 3; j++)
        {
          s.Momentum[j] += s.MomentumComp[i][j];
          s.AngMomentum[j] += s.AngMomentumComp[i][j];
          s.CenterOfMass[j] += s.CenterOfMassComp[i][j];
        }
    }
  for(int i = 0; i < 6; i++)
    for(int j = 0; j < 3; j++)
      if(s.MassComp[i] > 0)
        s.CenterOfMassComp[i][j] /= s.MassComp[i];
  for(int j = 0; j < 3; j++)
    if(s.Mass > 0)
      s.CenterOfMass[j] /= s.Mass;
  for(int i = 0; i < 6; i++)
    {
      for(int j = 0; j < 3; j++)
        {
          s.CenterOfMassComp[i][3] += s.CenterOfMassComp[i][j] * s.CenterOfMassComp[i][j];
          s.MomentumComp[i][3] += s.MomentumComp[i][j] * s.MomentumComp[i][j];
          s.AngMomentumComp[i][3] += s.AngMomentumComp[i][j] * s.AngMomentumComp[i][j];
        }
      s.CenterOfMassComp[i][3] = sqrt(s.CenterOfMassComp[i][3]);
      s.MomentumComp[i][3] = sqrt(s.MomentumComp[i][3]);
      s.AngMomentumComp[i][3] = sqrt(s.AngMomentumComp[i][3]);
    }
  for(int j = 0; j < 3; j++)
    {
      s.CenterOfMass[3] += s.CenterOfMass[j] * s.CenterOfMass[j];
      s.Momentum[3] += s.Momentum[j] * s.Momentum[j];
      s.AngMomentum[3] += s.AngMomentum[j] * s.AngMomentum[j];
    }
  s.CenterOfMass[3] = sqrt(s.CenterOfMass[3]);
  s.Momentum[3] = sqrt(s.Momentum[3]);
  s.AngMomentum[3] = sqrt(s.AngMomentum[3]);
  *out = s;
  return NGRAVS_OK;
}

// the energy.txt line of energy_statistics (run.c:419-429): 28 fields and a newline; the length, or NGRAVS_ERR_ARG for a short buffer
int time_energy_line(const ngravs_sysstate_t *s, double time, char *buf, int64_t len)
{
  double v[28] = {time, s->EnergyInt, s->EnergyPot, s->EnergyKin};
  for(int i = 0; i < 6; i++)
    {
      v[4 + 3 * i] = s->EnergyIntComp[i], v[5 + 3 * i] = s->EnergyPotComp[i], v[6 + 3 * i] = s->EnergyKinComp[i];
      v[22 + i] = s->MassComp[i];
    }
  char line[28 * 32];
  int at = 0;
  for(int k = 0; k < 28; k++)
    at += snprintf(line + at, sizeof line - at, k ? " %g" : "%g", v[k]);
  line[at++] = '\n';
  if(len < at + 1)
    return NGRAVS_ERR_ARG;
  memcpy(buf, line, at);
  buf[at] = 0;
  return at;
}

static const unsigned TIME_GAS_MOVE =TB(TC_GA) | TB(TC_VP) | TB(TC_HA) | TB(TC_ENT) | TB(TC_DTE) | TB(TC_RHO) | TB(TC_H) | TB(TC_PRES) | TB(TC_DIV) |
                                      TB(TC_TIB) | TB(TC_TIE);
static const unsigned TIME_GAS_ADVANCE = TB(TC_VP) | TB(TC_HA) | TB(TC_ENT) | TB(TC_DTE) | TB(TC_RHO) | TB(TC_H) | TB(TC_MSV);

int time_move_particles(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int time0, int time1, int wrap)
{
  const Refuse refuse = {c, "ngravs_move_particles"};
  if(!cols)
    return refuse(NGRAVS_ERR_ARG, "cols must not be NULL");
  int rc;
  if((rc = time_params_check(refuse, par)))
    return rc;
  if(time1 < time0)
    return refuse(NGRAVS_ERR_ARG, "time1 < time0");
  if(!(par->min_gas_hsml >= 0))
    return refuse(NGRAVS_ERR_ARG, "min_gas_hsml must be >= 0");
  const int mesh = c->cfg.pmgrid > 0;
  MoveParams p;
  if(par->comoving)
    {
      double f[3];
      if((rc = time_factors(par, time0, time1, f)))
        return rc;
      p.dt_drift = f[0], p.dt_gravkick = f[1], p.dt_hydrokick = f[2];
    }
  else
    p.dt_drift = p.dt_gravkick = p.dt_hydrokick = (time1 - time0) * par->timebase_interval;
  p.tbi = par->timebase_interval;
  p.min_gas_hsml = par->min_gas_hsml;
  p.gamma = par->gamma;
  p.box = c->cfg.box_size;
  p.time1 = time1;
  p.mesh = mesh;
  p.wrap = wrap && c->cfg.periodic && c->cfg.box_size > 0;
  TimeStage st = {c, cols};
  if((rc = st.begin(refuse, TB(TC_TYPE) | TB(TC_POS) | TB(TC_VEL), TIME_GAS_MOVE | (mesh ? TB(TC_GPM) : 0), sizeof(TimeCounters))))
    return rc;
  const long long n = cols->n;
  if(n == 0)
    return NGRAVS_OK;
  TimeCounters *cnt = reinterpret_cast<TimeCounters *>(st.scratch), h;
  if((rc = time_clear_counters(c, cnt)))
    return rc;
  hipLaunchKernelGGL(k_time_check, dim3(time_grid(n)), dim3(TIME_BLOCK), 0, c->stream, st.d.c[TC_TYPE], n, st.gas_ok, cnt);
  HIP_TRY(c, hipGetLastError());
  if((rc = time_read_counters(c, cnt, &h)) || (rc = time_flags_outcome(refuse, h.flags)))
    return rc;
  const TCol &cp = st.d.c[TC_POS], &cv = st.d.c[TC_VEL];
  const bool wide = cp.stride == 24 && cv.stride == 24 && (((uintptr_t)cp.p | (uintptr_t)cv.p) & 15) == 0;
  const dim3 grid((unsigned)((n + TIME_BLOCK - 1) / TIME_BLOCK));
  if(wide)
    hipLaunchKernelGGL(k_move<true>, grid, dim3(TIME_BLOCK), 0, c->stream, st.d, p);
  else
    hipLaunchKernelGGL(k_move<false>, grid, dim3(TIME_BLOCK), 0, c->stream, st.d, p);
  HIP_TRY(c, hipGetLastError());
  return st.finish(TB(TC_POS) | TB(TC_VP) | TB(TC_RHO) | TB(TC_H) | TB(TC_PRES));
}

int time_advance(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int ti_current, double dt_displacement,
                 int32_t *pm_ti, int64_t *n_kicked)
{
  const Refuse refuse = {c, "ngravs_advance_and_find_timesteps"};
  if(!cols)
    return refuse(NGRAVS_ERR_ARG, "cols must not be NULL");
  int rc;
  if((rc = time_params_check(refuse, par)))
    return rc;
  const int mesh = c->cfg.pmgrid > 0;
  if(mesh && !pm_ti)
    return refuse(NGRAVS_ERR_ARG, "a configuration with a mesh needs pm_ti");
  if(ti_current < 0 || ti_current > TI_BASE)
    return refuse(NGRAVS_ERR_ARG, "ti_current outside the integer time line");
  if(!(dt_displacement >= 0) || !(par->max_size_timestep >= 0) || !(par->min_size_timestep >= 0))
    return refuse(NGRAVS_ERR_ARG, "dt_displacement, max_size_timestep and min_size_timestep must be >= 0");
  if(mesh && (pm_ti[0] < 0 || pm_ti[1] < pm_ti[0] || pm_ti[1] > TI_BASE))
    return refuse(NGRAVS_ERR_ARG, "pm_ti is not a step on the integer time line");
  const long long n = cols->n;
  const size_t off_tab = up256(sizeof(TimeCounters)), off_step = off_tab + up256(sizeof(double) * 3 * TT_LEN);
  TimeStage st = {c, cols};
  if((rc = st.begin(refuse, TB(TC_TYPE) | TB(TC_VEL) | TB(TC_TIB) | TB(TC_TIE) | TB(TC_GA) | (mesh ? TB(TC_GPM) : 0), TIME_GAS_ADVANCE,
                    off_step + sizeof(int) * (size_t)(n > 0 ? n : 1))))
    return rc;
  TimeCounters *cnt = reinterpret_cast<TimeCounters *>(st.scratch), h;
  double *dtab = reinterpret_cast<double *>(st.scratch + off_tab);
  int *step = reinterpret_cast<int *>(st.scratch + off_step);

  AdvParams p;
  memset(&p, 0, sizeof p);
  p.tabs = time_host_tabs(par, dtab);
  if(par->comoving)
    {
      const double *tab[3] = {par->drift_table, par->gravkick_table, par->hydrokick_table};
      for(int k = 0; k < 3; k++)
        if((rc = col_upload(c, tab[k], sizeof(double), sizeof(double), 1, TT_LEN, 0, dtab + k * TT_LEN)))
          return rc;
      const double time = par->time_begin * exp(ti_current * par->timebase_interval);   // All.Time (run.c:231-234)
      p.fac1 = 1 / (time * time);
      p.fac2 = 1 / pow(time, 3 * par->gamma - 2);
      p.fac3 = pow(time, 3 * (1 - par->gamma) / 2.0);
      p.hubble_a = time_hubble_a(par, time);
      p.a3inv = 1 / (time * time * time);
      p.atime = time;
    }
  else
    p.fac1 = p.fac2 = p.fac3 = p.hubble_a = p.a3inv = p.atime = 1;
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    p.soft[t] = c->cfg.force_softening[t] / 2.8;
  p.eta = par->err_tol_int_accuracy;
  p.courant = par->courant_fac;
  p.scale = par->timestep_scale != 0 ? par->timestep_scale : 1.0;
  p.max_dt = par->max_size_timestep;
  p.min_dt = par->min_size_timestep;
  p.dt_disp = dt_displacement;
  p.tbi = par->timebase_interval;
  p.gamma = par->gamma;
  p.min_egy_spec = par->min_egy_spec;
  p.ti_current = ti_current;
  p.comoving = par->comoving != 0;
  p.mesh = mesh;
  p.adaptive = par->adaptive_gravsoft != 0;
  p.synchronization = par->synchronization != 0;
  p.stop = par->stop_below_min_timestep != 0;
  // the host's side of the tables: the same function on the caller's arrays
  const TimeTabs hg = time_host_tabs(par, par->gravkick_table);
  auto gravkick = [&](int t0, int t1) { return time_factor(hg.t, hg.ltb, hg.ltm, hg.tbi, t0, t1); };
  int pm_new[2] = {0, 0};
  if(mesh)
    {
      const int pmb = pm_ti[0], pme = pm_ti[1];
      if(par->comoving)   // timestep.c:70-76
        p.dt_gravkickB = gravkick(pmb, ti_current) - gravkick(pmb, (pmb + pme) / 2);
      else
        p.dt_gravkickB = (ti_current - (pmb + pme) / 2) * par->timebase_interval;
      if(pme == ti_current)   // timestep.c:351-383
        {
          p.long_range = 1;
          int ti_step = TI_BASE;
          while(ti_step > 0 && ti_step > dt_displacement / par->timebase_interval)
            ti_step >>= 1;
          if(ti_step > pme - pmb && ((TI_BASE - pme) % (ti_step > 0 ? ti_step : 1)) > 0)
            ti_step = pme - pmb;
          if(ti_current == TI_BASE)
            ti_step = 0;
          const int tstart = (pmb + pme) / 2, tend = pme + ti_step / 2;
          p.pm_dt_gravkick = par->comoving ? gravkick(tstart, tend) : (tend - tstart) * par->timebase_interval;
          pm_new[0] = pme;
          pm_new[1] = pme + ti_step;
          if(par->comoving)
            p.pm_dt_gravkickB = -gravkick(pm_new[0], (pm_new[0] + pm_new[1]) / 2);
          else
            p.pm_dt_gravkickB = -((pm_new[0] + pm_new[1]) / 2 - pm_new[0]) * par->timebase_interval;
        }
    }
  if(n_kicked)
    *n_kicked = 0;
  if(n > 0)
    {
      if((rc = time_clear_counters(c, cnt)))
        return rc;
      const dim3 grid((unsigned)((n + TIME_BLOCK - 1) / TIME_BLOCK));
      hipLaunchKernelGGL(k_advance_decide, grid, dim3(TIME_BLOCK), 0, c->stream, st.d, p, st.gas_ok, step, cnt);
      HIP_TRY(c, hipGetLastError());
      if((rc = time_read_counters(c, cnt, &h)) || (rc = time_flags_outcome(refuse, h.flags)))
        return rc;
      const long long none = 0x7fffffffffffffffll;
      if(h.row888 != none || h.row818 != none)
        {
          // the reference stops at the first failing row of its loop
          char msg[200];
          if(h.row888 < h.row818)
            {
              snprintf(msg, sizeof msg, "ngravs_advance_and_find_timesteps: timestep wants to be below the limit MinSizeTimestep, row %lld", h.row888);
              ngravs_report(c, 888, msg);
            }
          else
            {
              snprintf(msg, sizeof msg, "ngravs_advance_and_find_timesteps: a timestep outside (0, TIMEBASE) on the integer timeline, row %lld",
                       h.row818);
              ngravs_report(c, 818, msg);
            }
          return NGRAVS_ERR_STATE;
        }
      if(h.count > 0 || p.long_range)
        {
          hipLaunchKernelGGL(k_advance_apply, grid, dim3(TIME_BLOCK), 0, c->stream, st.d, p, step);
          HIP_TRY(c, hipGetLastError());
        }
      if((rc = st.finish(TB(TC_VEL) | TB(TC_TIB) | TB(TC_TIE) | TB(TC_VP) | TB(TC_ENT) | TB(TC_DTE))))
        return rc;
      if(n_kicked)
        *n_kicked = (int64_t)h.count;
    }
  if(p.long_range)
    pm_ti[0] = pm_new[0], pm_ti[1] = pm_new[1];
  return NGRAVS_OK;
}
