// kernels_snapshot.hip -- the reference's output station for one task: savepositions() (io.c:33-989) and find_next_outputtime()
// (run.c:244-361).
//
//   the file order (fill_write_buffer's pindex scan, io.c:178-206)   k_snap_count, k_snap_scan, k_snap_scatter -> order[n]
//   fill_write_buffer (io.c:129-357)                                 k_snap_scalar<BLOCK>, k_snap_vector<BLOCK>
//   get_particles_in_block (io.c:465-523)                            snap_segments (host)
//   the header (io.c:720-761), the framing (io.c:796-844, 965-969)   snapshot_header, snapshot_write (host)
//   find_next_outputtime (run.c:244-361)                             snapshot_next_outputtime (host)
//
// The file order is a stable six-way partition of the rows by type, kept in the context as a gather permutation (order[dest] =
// source row), so that every block kernel writes its output coalesced and gathers its rows.  The block kernels round to float where
// the reference assigns to its float buffer: after EACH statement of fill_write_buffer, and nothing is contracted into a fused
// multiply-add (the reference is built with -ffp-contract=off).
#include "time_common.hpp"
#include <cstdio>

#define SNAP_BLOCK 256
#define SNAP_WAVES (SNAP_BLOCK / 64)
#define SNAP_MAX_GRID 1024
#define SNAP_NT NGRAVS_NTYPES
#define SNAP_WRAP_LIMIT 1024.0   // a periodic position beyond that many box lengths is refused: at most 1025 trips of the wrap loops

// snap_tmp: counts[6][G] | base[6][G] | npart[6] | flags
struct SnapPlanBufs
{
  int *counts, *base, *npart;
  unsigned *flags;
};
#define SF_BAD_TYPE 1u
#define SF_BAD_POS 2u

// ---- the file order --------------------------------------------------------------------------------------------------------------
// Block b owns the chunks [b * cpb, (b + 1) * cpb) of SNAP_BLOCK rows: a CONTIGUOUS range, so that the rows of one type keep their
// order across the trips of a block and across blocks.  The counts of a wave are popcounts of one ballot per type.
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_count(TCol type, long long n, long long cpb, SnapPlanBufs pb)
{
  __shared__ int lds[SNAP_WAVES][SNAP_NT + 1];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int cnt[SNAP_NT] = {0, 0, 0, 0, 0, 0};
  int bad = 0;
  const long long c0 = blockIdx.x * cpb;
  for(long long ch = c0; ch < c0 + cpb; ch++)
    {
      const long long i = ch * SNAP_BLOCK + threadIdx.x;
      if(ch * SNAP_BLOCK >= n)
        break;
      const int t = i < n ? ldi(type, i) : -1;
      bad |= i < n && (t < 0 || t >= SNAP_NT);
#pragma unroll
      for(int k = 0; k < SNAP_NT; k++)
        cnt[k] += __popcll(__ballot(t == k));
    }
  bad = __any(bad);
  if(lane == 0)
    {
      for(int k = 0; k < SNAP_NT; k++)
        lds[wave][k] = cnt[k];
      lds[wave][SNAP_NT] = bad;
    }
  __syncthreads();
  if(threadIdx.x <= SNAP_NT)
    {
      int s = 0;
      for(int w = 0; w < SNAP_WAVES; w++)
        s += lds[w][threadIdx.x];
      if(threadIdx.x < SNAP_NT)
        pb.counts[threadIdx.x * gridDim.x + blockIdx.x] = s;
      else if(s)
        atomicOr(pb.flags, SF_BAD_TYPE);   // (a flag, not a sum: the order it is set in does not matter)
    }
}
// the exclusive scan of the counts in (type, block) order: one block of SNAP_MAX_GRID threads, thread b holds block b's count
__global__ __launch_bounds__(SNAP_MAX_GRID) void k_snap_scan(int G, SnapPlanBufs pb)
{
  __shared__ int wsum[SNAP_MAX_GRID / 64];
  __shared__ int running;
  const int b = threadIdx.x, lane = b & 63, wave = b >> 6;
  if(b == 0)
    running = 0;
  __syncthreads();
  for(int t = 0; t < SNAP_NT; t++)
    {
      const int v = b < G ? pb.counts[t * G + b] : 0;
      int s = v;   // inclusive scan within the wave
      for(int o = 1; o < 64; o <<= 1)
        {
          const int u = __shfl_up(s, o);
          if(lane >= o)
            s += u;
        }
      if(lane == 63)
        wsum[wave] = s;
      __syncthreads();
      int before = 0, total = 0;
      for(int w = 0; w < SNAP_MAX_GRID / 64; w++)
        {
          before += w < wave ? wsum[w] : 0;
          total += wsum[w];
        }
      const int run = running;
      if(b < G)
        pb.base[t * G + b] = run + before + s - v;
      __syncthreads();
      if(b == 0)
        {
          pb.npart[t] = total;
          running = run + total;
        }
      __syncthreads();
    }
}
// A row's place: the base of its (type, block), the rows of its type in the block's earlier chunks, those in the chunk's earlier
// waves (per-wave counts in LDS), and those in lower lanes of its wave (the ballot mask below its lane).
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_scatter(TCol type, long long n, long long cpb, SnapPlanBufs pb, int *__restrict__ order)
{
  __shared__ int lds[2][SNAP_WAVES][SNAP_NT];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const unsigned long long below = lane ? (~0ull >> (64 - lane)) : 0ull;
  int run[SNAP_NT];
#pragma unroll
  for(int k = 0; k < SNAP_NT; k++)
    run[k] = pb.base[k * gridDim.x + blockIdx.x];
  const long long c0 = blockIdx.x * cpb;
  int buf = 0;
  for(long long ch = c0; ch < c0 + cpb; ch++, buf ^= 1)   // (two LDS buffers: one barrier per chunk)
    {
      if(ch * SNAP_BLOCK >= n)
        break;
      const long long i = ch * SNAP_BLOCK + threadIdx.x;
      const int t = i < n ? ldi(type, i) : -1;
      int rank = 0, mine = -1;
#pragma unroll
      for(int k = 0; k < SNAP_NT; k++)
        {
          const unsigned long long m = __ballot(t == k);
          if(lane == 0)
            lds[buf][wave][k] = __popcll(m);
          if(t == k)
            rank = __popcll(m & below), mine = k;
        }
      __syncthreads();
      int dest = 0;
#pragma unroll
      for(int k = 0; k < SNAP_NT; k++)
        {
          int before = 0, total = 0;
#pragma unroll
          for(int w = 0; w < SNAP_WAVES; w++)
            {
              const int cw = lds[buf][w][k];
              before += w < wave ? cw : 0;
              total += cw;
            }
          if(mine == k)
            dest = run[k] + before + rank;
          run[k] += total;
        }
      if(mine >= 0 && dest >= 0 && dest < n)   // (the plan is refused when a type is outside 0..5; the bound is for the store alone)
        order[dest] = (int)i;
    }
}

// ---- fill_write_buffer (io.c:129-357) ------------------------------------------------------------------------------------------------
enum { B_POS, B_VEL, B_ID, B_MASS, B_U, B_RHO, B_HSML, B_POT, B_ACCE, B_ENDT, B_TSTP, B_COUNT };
static_assert(B_COUNT == NGRAVS_SNAP_NBLOCKS && B_TSTP == NGRAVS_SNAP_TSTP && B_POS == NGRAVS_SNAP_POS, "enum iofields");
static const char snap_label[B_COUNT][5] = {"POS ", "VEL ", "ID  ", "MASS", "U   ", "RHO ", "HSML", "POT ", "ACCE", "ENDT", "TSTP"};
static const char *const snap_name[B_COUNT] = {"POS", "VEL", "ID", "MASS", "U", "RHO", "HSML", "POT", "ACCE", "ENDT", "TSTP"};
static bool snap_is_vector(int b) { return b == B_POS || b == B_VEL || b == B_ACCE; }

struct SnapParams
{
  TimeTabs tabs;
  double tbi, dt_pm, a3inv, sqrt_a3inv, fac1, fac2, gm1, min_egy, box;
  int ti_current, comoving, mesh, isotherm, periodic;
  long long ngas;   // rows of type 0: the first ngas places of the file order
};
// a block's elements in the file order: up to six runs (one per type that the block holds)
struct SnapSegs
{
  int nseg;
  long long dst0[SNAP_NT], src0[SNAP_NT], len[SNAP_NT];
  __device__ long long place(long long e) const
  {
    long long o = -1;
    for(int s = 0; s < nseg; s++)
      if(e >= dst0[s] && e < dst0[s] + len[s])
        o = src0[s] + (e - dst0[s]);
    return o;
  }
};

// io.c:183-201 on the float; the trip bound is never reached by a row that k_snap_pos_check let pass
__device__ inline float snap_wrap(float fp, double box)
{
#pragma clang fp contract(off)
  for(int trip = 0; trip < 1025 && fp < 0; trip++)
    fp = (float)(fp + box);
  for(int trip = 0; trip < 1025 && fp >= box; trip++)
    fp = (float)(fp - box);
  return fp;
}
// io.c:213-228: the two kick factors of a row, as in k_global_sums
__device__ inline void snap_kicks(const TCols &c, const SnapParams &p, long long i, bool gas, double &dt_gravkick, double &dt_hydrokick)
{
#pragma clang fp contract(off)
  const int beg = ldi(c.c[TC_TIB], i), mid = (beg + ldi(c.c[TC_TIE], i)) / 2;
  dt_gravkick = dt_hydrokick = (p.ti_current - mid) * p.tbi;
  if(p.comoving)
    {
      dt_gravkick = p.tabs.gravkick(beg, p.ti_current) - p.tabs.gravkick(beg, mid);
      if(gas)
        dt_hydrokick = p.tabs.hydrokick(beg, p.ti_current) - p.tabs.hydrokick(beg, mid);
    }
}
template <int BLOCK> __device__ inline void snap_vector_row(const TCols &c, const SnapParams &p, long long i, bool gas, float fp[3])
{
#pragma clang fp contract(off)
  if(BLOCK == B_POS)
    {
      for(int k = 0; k < 3; k++)
        {
          fp[k] = (float)ldd(c.c[TC_POS], i, k);
          if(p.periodic)
            fp[k] = snap_wrap(fp[k], p.box);
        }
    }
  else if(BLOCK == B_VEL)
    {
      double dt_gravkick, dt_hydrokick;
      snap_kicks(c, p, i, gas, dt_gravkick, dt_hydrokick);
      for(int k = 0; k < 3; k++)
        {
          fp[k] = (float)(ldd(c.c[TC_VEL], i, k) + ldd(c.c[TC_GA], i, k) * dt_gravkick);
          if(gas)
            fp[k] = (float)(fp[k] + ldd(c.c[TC_HA], i, k) * dt_hydrokick);
          if(p.mesh)
            fp[k] = (float)(fp[k] + ldd(c.c[TC_GPM], i, k) * p.dt_pm);
          fp[k] = (float)(fp[k] * p.sqrt_a3inv);
        }
    }
  else   // B_ACCE
    {
      for(int k = 0; k < 3; k++)
        {
          fp[k] = (float)(p.fac1 * ldd(c.c[TC_GA], i, k));
          if(p.mesh)
            fp[k] = (float)(fp[k] + p.fac1 * ldd(c.c[TC_GPM], i, k));
          if(gas)
            fp[k] = (float)(fp[k] + p.fac2 * ldd(c.c[TC_HA], i, k));
        }
    }
}
// the element's 4 bytes on disk
template <int BLOCK> __device__ inline unsigned snap_scalar_row(const TCols &c, const TCol &extra, const SnapParams &p, long long i)
{
#pragma clang fp contract(off)
  float f = 0;
  if(BLOCK == B_ID)
    return (unsigned)ldi(extra, i);
  else if(BLOCK == B_MASS)
    f = (float)ldd(c.c[TC_MASS], i);
  else if(BLOCK == B_U)
    {
      const double entr = ldd(c.c[TC_ENT], i);
      if(p.isotherm)
        f = (float)entr;
      else
        {
          const double u = entr / p.gm1 * pow(ldd(c.c[TC_RHO], i) * p.a3inv, p.gm1);
          f = (float)(p.min_egy > u ? p.min_egy : u);   // dmax (system.c)
        }
    }
  else if(BLOCK == B_RHO)
    f = (float)ldd(c.c[TC_RHO], i);
  else if(BLOCK == B_HSML)
    f = (float)ldd(c.c[TC_H], i);
  else if(BLOCK == B_POT)
    f = (float)ldd(extra, i);
  else if(BLOCK == B_ENDT)
    f = (float)ldd(c.c[TC_DTE], i);
  else   // B_TSTP
    f = (float)((ldi(c.c[TC_TIE], i) - ldi(c.c[TC_TIB], i)) * p.tbi);
  return __float_as_uint(f);
}

// out[e - first] for the elements e of [first, first + count) of the block
template <int BLOCK>
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_scalar(TCols c, TCol extra, SnapParams p, SnapSegs sg, const int *__restrict__ order, long long first,
                                                            long long count, unsigned *__restrict__ out)
{
  for(long long j = blockIdx.x * (long long)SNAP_BLOCK + threadIdx.x; j < count; j += (long long)gridDim.x * SNAP_BLOCK)
    {
      const long long o = sg.place(first + j);
      if(o < 0 || o >= c.n)
        continue;
      const long long i = order[o];
      if(i < 0 || i >= c.n)
        continue;
      out[j] = snap_scalar_row<BLOCK>(c, extra, p, i);
    }
}
// A thread takes four consecutive elements: twelve floats, three 16-byte stores where the quad is whole and `aligned` says that
// out + 12 * (a multiple of four) is a multiple of 16 bytes; single floats otherwise.
template <int BLOCK>
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_vector(TCols c, SnapParams p, SnapSegs sg, const int *__restrict__ order, long long first, long long count,
                                                            float *__restrict__ out, int aligned)
{
  const long long quads = (count + 3) / 4;
  for(long long q = blockIdx.x * (long long)SNAP_BLOCK + threadIdx.x; q < quads; q += (long long)gridDim.x * SNAP_BLOCK)
    {
      float v[12];
      bool ok[4];
      for(int r = 0; r < 4; r++)
        {
          const long long j = 4 * q + r;
          ok[r] = false;
          v[3 * r] = v[3 * r + 1] = v[3 * r + 2] = 0;
          if(j >= count)
            continue;
          const long long o = sg.place(first + j);
          if(o < 0 || o >= c.n)
            continue;
          const long long i = order[o];
          if(i < 0 || i >= c.n)
            continue;
          ok[r] = true;
          snap_vector_row<BLOCK>(c, p, i, o < p.ngas, v + 3 * r);
        }
      if(aligned && ok[0] && ok[1] && ok[2] && ok[3])
        {
          float4 *dst = reinterpret_cast<float4 *>(out + 12 * q);
          dst[0] = make_float4(v[0], v[1], v[2], v[3]);
          dst[1] = make_float4(v[4], v[5], v[6], v[7]);
          dst[2] = make_float4(v[8], v[9], v[10], v[11]);
        }
      else
        for(int r = 0; r < 4; r++)
          if(ok[r])
            for(int k = 0; k < 3; k++)
              out[12 * q + 3 * r + k] = v[3 * r + k];
    }
}
// the refusal of the periodic POS block: a coordinate that is not finite or at least SNAP_WRAP_LIMIT box lengths away
__global__ __launch_bounds__(SNAP_BLOCK) void k_snap_pos_check(TCols c, SnapParams p, SnapSegs sg, const int *__restrict__ order, long long first, long long count,
                                                               unsigned *flags)
{
  int bad = 0;
  for(long long j = blockIdx.x * (long long)SNAP_BLOCK + threadIdx.x; j < count; j += (long long)gridDim.x * SNAP_BLOCK)
    {
      const long long o = sg.place(first + j);
      if(o < 0 || o >= c.n)
        continue;
      const long long i = order[o];
      if(i < 0 || i >= c.n)
        continue;
      for(int k = 0; k < 3; k++)
        {
          const double x = ldd(c.c[TC_POS], i, k);
          bad |= !(fabs(x) < SNAP_WRAP_LIMIT * p.box);   // (NaN and the infinities fail the comparison)
        }
    }
  if(__any(bad) && (threadIdx.x & 63) == 0)
    atomicOr(flags, SF_BAD_POS);
}

// ---- host side ----------------------------------------------------------------------------------------------------------------------
static unsigned snap_grid(long long n)
{
  long long g = (n + SNAP_BLOCK - 1) / SNAP_BLOCK;
  return (unsigned)(g < 1 ? 1 : (g > SNAP_MAX_GRID ? SNAP_MAX_GRID : g));
}
static SnapPlanBufs snap_plan_bufs(ngravs_ctx *c)
{
  SnapPlanBufs pb;
  pb.counts = c->snap_tmp.p;
  pb.base = pb.counts + SNAP_NT * SNAP_MAX_GRID;
  pb.npart = pb.base + SNAP_NT * SNAP_MAX_GRID;
  pb.flags = reinterpret_cast<unsigned *>(pb.npart + 8);
  return pb;
}

// the order for the device column `type` of n rows into the context; the earlier plan is gone whatever the outcome
static int snap_plan_device(ngravs_ctx *c, const Refuse &refuse, TCol type, long long n, int64_t npart[6])
{
  c->snap_n = -1;
  if(n > 0x7fffffffll)
    return refuse(NGRAVS_ERR_ARG, "n does not fit the int32 order");
  if(c->snap_tmp.ensure(2 * SNAP_NT * SNAP_MAX_GRID + 16) || c->snap_order.ensure((size_t)(n > 0 ? n : 1)))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  int hn[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  if(n > 0)
    {
      const SnapPlanBufs pb = snap_plan_bufs(c);
      const long long chunks = (n + SNAP_BLOCK - 1) / SNAP_BLOCK;
      const unsigned G = snap_grid(n);
      const long long cpb = (chunks + G - 1) / G;
      HIP_TRY(c, hipMemsetAsync(pb.flags, 0, sizeof(unsigned), c->stream));
      hipLaunchKernelGGL(k_snap_count, dim3(G), dim3(SNAP_BLOCK), 0, c->stream, type, n, cpb, pb);
      hipLaunchKernelGGL(k_snap_scan, dim3(1), dim3(SNAP_MAX_GRID), 0, c->stream, (int)G, pb);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipMemcpyAsync(hn, pb.npart, sizeof(int) * 7, hipMemcpyDeviceToHost, c->stream));   // npart[6], pad, flags
      HIP_TRY(c, hipMemcpyAsync(hn + 7, pb.flags, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if(hn[7] & SF_BAD_TYPE)
        return refuse(NGRAVS_ERR_ARG, "a type outside 0..5");
      hipLaunchKernelGGL(k_snap_scatter, dim3(G), dim3(SNAP_BLOCK), 0, c->stream, type, n, cpb, pb, c->snap_order.p);
      HIP_TRY(c, hipGetLastError());
      HIP_TRY(c, hipStreamSynchronize(c->stream));
    }
  for(int t = 0; t < SNAP_NT; t++)
    c->snap_npart[t] = npart[t] = hn[t];
  c->snap_n = n;
  return NGRAVS_OK;
}

int snapshot_plan(ngravs_ctx *c, const ngravs_time_cols_t *cols, int64_t npart[6])
{
  const Refuse refuse = {c, "ngravs_snapshot_plan"};
  if(!cols || !npart)
    return refuse(NGRAVS_ERR_ARG, "cols and npart must not be NULL");
  c->snap_n = -1;
  TimeStage st = {c, cols};
  int rc;
  if((rc = st.begin(refuse, TB(TC_TYPE), 0, 256)))
    return rc;
  return snap_plan_device(c, refuse, st.d.c[TC_TYPE], cols->n, npart);
}

// get_particles_in_block (io.c:465-523): the block's runs in the file order; returns its number of elements
static long long snap_segments(const int64_t npart[6], const double mass_table[6], int block, SnapSegs *sg)
{
  long long off[SNAP_NT + 1] = {0};
  for(int t = 0; t < SNAP_NT; t++)
    off[t + 1] = off[t] + npart[t];
  SnapSegs s;
  memset(&s, 0, sizeof s);
  long long total = 0;
  for(int t = 0; t < SNAP_NT; t++)
    {
      bool in = npart[t] > 0;
      if(block == B_MASS)
        in = in && mass_table[t] == 0;
      if(block == B_U || block == B_RHO || block == B_HSML || block == B_ENDT)
        in = in && t == 0;
      if(!in)
        continue;
      s.dst0[s.nseg] = total, s.src0[s.nseg] = off[t], s.len[s.nseg] = npart[t];
      s.nseg++;
      total += npart[t];
    }
  if(sg)
    *sg = s;
  return total;
}

int snapshot_block_count(ngravs_ctx *c, const ngravs_snapshot_t *snap, int block, int64_t *count, int32_t *bytes_per_element)
{
  const Refuse refuse = {c, "ngravs_snapshot_block_count"};
  if(!snap || !count)
    return refuse(NGRAVS_ERR_ARG, "snap and count must not be NULL");
  if(block < 0 || block >= B_COUNT)
    return refuse(NGRAVS_ERR_ARG, "no such block");
  if(c->snap_n < 0)
    return refuse(NGRAVS_ERR_STATE, "no plan: call ngravs_snapshot_plan first");
  *count = snap_segments(c->snap_npart, snap->mass_table, block, nullptr);
  if(bytes_per_element)
    *bytes_per_element = snap_is_vector(block) ? 12 : 4;
  return NGRAVS_OK;
}

// which columns of ngravs_time_cols_t a block reads: every row / only with gas
static void snap_block_columns(int block, int mesh, unsigned *need, unsigned *gas)
{
  *need = *gas = 0;
  switch(block)
    {
    case B_POS: *need = TB(TC_POS); break;
    case B_VEL: *need = TB(TC_VEL) | TB(TC_GA) | TB(TC_TIB) | TB(TC_TIE) | (mesh ? TB(TC_GPM) : 0), *gas = TB(TC_HA); break;
    case B_MASS: *need = TB(TC_MASS); break;
    case B_U: *gas = TB(TC_ENT) | TB(TC_RHO); break;
    case B_RHO: *gas = TB(TC_RHO); break;
    case B_HSML: *gas = TB(TC_H); break;
    case B_ACCE: *need = TB(TC_GA) | (mesh ? TB(TC_GPM) : 0), *gas = TB(TC_HA); break;
    case B_ENDT: *gas = TB(TC_DTE); break;
    case B_TSTP: *need = TB(TC_TIB) | TB(TC_TIE); break;
    default: break;   // ID, POT: columns of ngravs_snapshot_t
    }
}

// what a call checks before it touches the device
static int snap_check_args(ngravs_ctx *c, const Refuse &refuse, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap)
{
  if(!cols || !snap)
    return refuse(NGRAVS_ERR_ARG, "cols and snap must not be NULL");
  if(int rc = time_params_check(refuse, par))
    return rc;
  const int mesh = c->cfg.pmgrid > 0;
  if(mesh && !snap->pm_ti)
    return refuse(NGRAVS_ERR_ARG, "a configuration with a mesh needs pm_ti");
  if(snap->ti_current < 0 || snap->ti_current > TI_BASE)
    return refuse(NGRAVS_ERR_ARG, "ti_current outside the integer time line");
  if(mesh && (snap->pm_ti[0] < 0 || snap->pm_ti[1] < snap->pm_ti[0] || snap->pm_ti[1] > TI_BASE))
    return refuse(NGRAVS_ERR_ARG, "pm_ti is not a step on the integer time line");
  if(c->cfg.periodic && !(c->cfg.box_size > 0))
    return refuse(NGRAVS_ERR_ARG, "a periodic configuration needs box_size > 0");
  return NGRAVS_OK;
}
// a block that is asked for and whose column is missing
static int snap_check_block(ngravs_ctx *c, const Refuse &refuse, const ngravs_time_cols_t *cols, const ngravs_snapshot_t *snap, int block)
{
  const TCol *src = reinterpret_cast<const TCol *>(cols);
  unsigned need, gas;
  snap_block_columns(block, c->cfg.pmgrid > 0, &need, &gas);
  const long long n = cols->n;
  for(int k = 0; k < TC_COUNT; k++)
    {
      const bool wanted = (need & TB(k)) || ((gas & TB(k)) && c->snap_npart[0] > 0);
      if(wanted && n > 0 && !src[k].p)
        return refuse(NGRAVS_ERR_ARG, std::string("block ") + snap_name[block] + ": the column " + tc_name[k] + " is missing" +
                                          ((gas & TB(k)) ? " (there are type-0 rows)" : ""));
      if(wanted && src[k].p && src[k].stride < tc_bytes[k] && n > 1)
        return refuse(NGRAVS_ERR_ARG, std::string(tc_name[k]) + "_stride is smaller than the field");
    }
  if(block == B_ID && n > 0 && (!snap->ids || (snap->ids_stride < 4 && n > 1)))
    return refuse(NGRAVS_ERR_ARG, "block ID: the column ids is missing, or its stride is smaller than the field");
  if(block == B_POT && n > 0 && (!snap->potential || (snap->potential_stride < 8 && n > 1)))
    return refuse(NGRAVS_ERR_ARG, "block POT: the column potential is missing, or its stride is smaller than the field");
  return NGRAVS_OK;
}

static int snap_params(ngravs_ctx *c, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, double *dtab, bool tables, SnapParams *out)
{
  SnapParams p;
  memset(&p, 0, sizeof p);
  p.tabs = time_host_tabs(par, dtab);
  p.tbi = par->timebase_interval;
  p.a3inv = p.sqrt_a3inv = p.fac1 = p.fac2 = 1;   // io.c:149-156
  p.gm1 = par->gamma - 1;
  p.isotherm = par->gamma == 1;
  p.min_egy = par->min_egy_spec;
  p.box = c->cfg.box_size;
  p.periodic = c->cfg.periodic != 0;
  p.ti_current = snap->ti_current;
  p.comoving = par->comoving != 0;
  p.mesh = c->cfg.pmgrid > 0;
  p.ngas = c->snap_npart[0];
  if(par->comoving)
    {
      if(tables)
        {
          const double *tab[3] = {par->drift_table, par->gravkick_table, par->hydrokick_table};
          for(int k = 0; k < 3; k++)
            if(int rc = col_upload(c, tab[k], sizeof(double), sizeof(double), 1, TT_LEN, 0, dtab + k * TT_LEN))
              return rc;
        }
      const double time = par->time_begin * exp(snap->ti_current * par->timebase_interval);   // All.Time (run.c:212-213)
      p.a3inv = 1 / (time * time * time);
      p.fac1 = 1 / (time * time);
      p.fac2 = 1 / pow(time, 3 * par->gamma - 2);
    }
  p.sqrt_a3inv = sqrt(p.a3inv);
  if(p.mesh)   // io.c:158-166
    {
      const TimeTabs hg = time_host_tabs(par, par->gravkick_table);
      const int pmb = snap->pm_ti[0], mid = (snap->pm_ti[0] + snap->pm_ti[1]) / 2;
      if(par->comoving)
        p.dt_pm = time_factor(hg.t, hg.ltb, hg.ltm, hg.tbi, pmb, snap->ti_current) - time_factor(hg.t, hg.ltb, hg.ltm, hg.tbi, pmb, mid);
      else
        p.dt_pm = (snap->ti_current - mid) * par->timebase_interval;
    }
  *out = p;
  return NGRAVS_OK;
}

// the elements [first, first + count) of a block into dout (device, 4 or 12 bytes each); the arguments were checked
static void snap_launch(ngravs_ctx *c, const TCols &d, TCol extra, const SnapParams &p, const SnapSegs &sg, int block, long long first, long long count,
                        void *dout)
{
  if(count <= 0)
    return;
  const int *order = c->snap_order.p;
  unsigned *u = static_cast<unsigned *>(dout);
  float *f = static_cast<float *>(dout);
  const int aligned = ((uintptr_t)dout & 15) == 0;
  const dim3 gs(snap_grid(count)), gv(snap_grid((count + 3) / 4)), bl(SNAP_BLOCK);
#define SNAP_SCALAR(B) hipLaunchKernelGGL(k_snap_scalar<B>, gs, bl, 0, c->stream, d, extra, p, sg, order, first, count, u)
#define SNAP_VECTOR(B) hipLaunchKernelGGL(k_snap_vector<B>, gv, bl, 0, c->stream, d, p, sg, order, first, count, f, aligned)
  switch(block)
    {
    case B_POS: SNAP_VECTOR(B_POS); break;
    case B_VEL: SNAP_VECTOR(B_VEL); break;
    case B_ACCE: SNAP_VECTOR(B_ACCE); break;
    case B_ID: SNAP_SCALAR(B_ID); break;
    case B_MASS: SNAP_SCALAR(B_MASS); break;
    case B_U: SNAP_SCALAR(B_U); break;
    case B_RHO: SNAP_SCALAR(B_RHO); break;
    case B_HSML: SNAP_SCALAR(B_HSML); break;
    case B_POT: SNAP_SCALAR(B_POT); break;
    case B_ENDT: SNAP_SCALAR(B_ENDT); break;
    default: SNAP_SCALAR(B_TSTP); break;
    }
#undef SNAP_SCALAR
#undef SNAP_VECTOR
}
// the refusal of a periodic POS range (nothing is written then)
static int snap_pos_check(ngravs_ctx *c, const Refuse &refuse, const TCols &d, const SnapParams &p, const SnapSegs &sg, long long first, long long count,
                          unsigned *dflags)
{
  if(!p.periodic || count <= 0)
    return NGRAVS_OK;
  unsigned h = 0;
  HIP_TRY(c, hipMemsetAsync(dflags, 0, sizeof(unsigned), c->stream));
  hipLaunchKernelGGL(k_snap_pos_check, dim3(snap_grid(count)), dim3(SNAP_BLOCK), 0, c->stream, d, p, sg, c->snap_order.p, first, count, dflags);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(&h, dflags, sizeof h, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  if(h & SF_BAD_POS)
    return refuse(NGRAVS_ERR_ARG, "block POS: a periodic position that is not finite or 1024 box lengths away or more");
  return NGRAVS_OK;
}

// the scratch of one call behind the staged columns: flags | tables | out | ids | potential
struct SnapScratch
{
  size_t off_tab, off_out, off_ids, off_pot, total;
  SnapScratch(size_t out_bytes, size_t ids_bytes, size_t pot_bytes)
  {
    off_tab = 256;
    off_out = off_tab + up256(sizeof(double) * 3 * TT_LEN);
    off_ids = off_out + up256(out_bytes);
    off_pot = off_ids + up256(ids_bytes);
    total = off_pot + up256(pot_bytes);
  }
};
// the ids / potential column of ngravs_snapshot_t on the device
static int snap_extra(ngravs_ctx *c, const ngravs_time_cols_t *cols, const void *p, int64_t stride, size_t bytes, unsigned char *stage, TCol *out)
{
  out->p = nullptr, out->stride = 0;
  if(!p || cols->n <= 0)
    return NGRAVS_OK;
  if(cols->on_device)
    {
      out->p = static_cast<unsigned char *>(const_cast<void *>(p)), out->stride = stride;
      return NGRAVS_OK;
    }
  if(int rc = col_upload(c, p, stride, bytes, 1, cols->n, 0, stage))
    return rc;
  out->p = stage, out->stride = (long long)bytes;
  return NGRAVS_OK;
}

int snapshot_block(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, int block,
                   int64_t first, int64_t count, void *out, int out_on_device)
{
  const Refuse refuse = {c, "ngravs_snapshot_block"};
  int rc;
  if((rc = snap_check_args(c, refuse, cols, par, snap)))
    return rc;
  if(block < 0 || block >= B_COUNT)
    return refuse(NGRAVS_ERR_ARG, "no such block");
  if(c->snap_n < 0)
    return refuse(NGRAVS_ERR_STATE, "no plan: call ngravs_snapshot_plan first");
  if(cols->n != c->snap_n)
    return refuse(NGRAVS_ERR_STATE, "n is not the plan's");
  SnapSegs sg;
  const long long total = snap_segments(c->snap_npart, snap->mass_table, block, &sg);
  if(first < 0 || count < 0 || first > total || count > total - first)
    return refuse(NGRAVS_ERR_ARG, std::string("the range is outside the block ") + snap_name[block]);
  if(count > 0 && !out)
    return refuse(NGRAVS_ERR_ARG, "out must not be NULL");
  if((rc = snap_check_block(c, refuse, cols, snap, block)))
    return rc;
  if(count == 0)
    return NGRAVS_OK;
  const size_t el = snap_is_vector(block) ? 12 : 4;
  const bool host_cols = !cols->on_device;
  const SnapScratch sc(out_on_device ? 0 : el * (size_t)count, host_cols && block == B_ID ? 4 * (size_t)cols->n : 0,
                       host_cols && block == B_POT ? 8 * (size_t)cols->n : 0);
  unsigned need, gas;
  snap_block_columns(block, c->cfg.pmgrid > 0, &need, &gas);
  TimeStage st = {c, cols};
  if((rc = st.begin(refuse, need, c->snap_npart[0] > 0 ? gas : 0, sc.total)))
    return rc;
  SnapParams p;
  if((rc = snap_params(c, par, snap, reinterpret_cast<double *>(st.scratch + sc.off_tab), block == B_VEL, &p)))
    return rc;
  TCol extra = {nullptr, 0};
  if(block == B_ID && (rc = snap_extra(c, cols, snap->ids, snap->ids_stride, 4, st.scratch + sc.off_ids, &extra)))
    return rc;
  if(block == B_POT && (rc = snap_extra(c, cols, snap->potential, snap->potential_stride, 8, st.scratch + sc.off_pot, &extra)))
    return rc;
  if(block == B_POS && (rc = snap_pos_check(c, refuse, st.d, p, sg, first, count, reinterpret_cast<unsigned *>(st.scratch))))
    return rc;
  void *dout = out_on_device ? out : static_cast<void *>(st.scratch + sc.off_out);
  snap_launch(c, st.d, extra, p, sg, block, first, count, dout);
  HIP_TRY(c, hipGetLastError());
  if(!out_on_device)
    return col_download(c, dout, 4, (int)(el / 4), count, out, (int64_t)el, 0, nullptr);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

// ---- the header (io.c:720-761), field for field -------------------------------------------------------------------------------------
struct SnapHeader   // struct io_header, allvars.h
{
  int npart[6];
  double mass[6];
  double time, redshift;
  int flag_sfr, flag_feedback;
  unsigned npartTotal[6];
  int flag_cooling, num_files;
  double BoxSize, Omega0, OmegaLambda, HubbleParam;
  int flag_stellarage, flag_metals;
  unsigned npartTotalHighWord[6];
  int flag_entropy_instead_u;
  char fill[60];
};
static_assert(sizeof(SnapHeader) == 256, "io_header is 256 bytes");

int snapshot_header(const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, const int64_t npart[6], const int64_t npart_total[6],
                    int num_files, double time, unsigned char out[256])
{
  SnapHeader h;
  memset(&h, 0, sizeof h);
  for(int n = 0; n < 6; n++)
    {
      h.npart[n] = (int)npart[n];
      h.npartTotal[n] = (unsigned)npart_total[n];
      h.npartTotalHighWord[n] = (unsigned)(npart_total[n] >> 32);
      h.mass[n] = snap->mass_table[n];
    }
  h.time = time;
  h.redshift = par->comoving ? 1.0 / time - 1 : 0;
  h.num_files = num_files;
  h.BoxSize = snap->box_size;
  h.Omega0 = par->omega0;
  h.OmegaLambda = par->omega_lambda;
  h.HubbleParam = snap->hubble_param;
  memcpy(out, &h, sizeof h);
  return NGRAVS_OK;
}

// ---- the file (write_file, io.c:672-989, for one task and one file) -----------------------------------------------------------------
static bool snap_fwrite(const void *p, size_t bytes, FILE *fd) { return bytes == 0 || fwrite(p, bytes, 1, fd) == 1; }
static bool snap_label_record(const char *label, int next, FILE *fd)   // io.c:796-803, 832-839
{
  const int blksize = sizeof(int) + 4 * sizeof(char);
  return snap_fwrite(&blksize, 4, fd) && snap_fwrite(label, 4, fd) && snap_fwrite(&next, 4, fd) && snap_fwrite(&blksize, 4, fd);
}

int snapshot_write(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                   uint32_t blocks_mask, int snap_format, int64_t buffer_bytes, const char *path)
{
  const Refuse refuse = {c, "ngravs_snapshot_write"};
  int rc;
  if(!path)
    return refuse(NGRAVS_ERR_ARG, "path must not be NULL");
  if(snap_format == 3)
    return refuse(NGRAVS_ERR_ARG, "snap_format 3: the library has no HDF5 support");
  if(snap_format != 1 && snap_format != 2)
    return refuse(NGRAVS_ERR_ARG, "unsupported file format (snap_format must be 1 or 2)");
  if((rc = snap_check_args(c, refuse, cols, par, snap)))
    return rc;
  if(buffer_bytes < 0 || (buffer_bytes > 0 && buffer_bytes < 12))
    return refuse(NGRAVS_ERR_ARG, "buffer_bytes holds no element");
  if(buffer_bytes == 0)
    buffer_bytes = 64ll << 20;
  c->snap_n = -1;
  const long long n = cols->n;
  if(n < 0)
    return refuse(NGRAVS_ERR_ARG, "n must be >= 0");
  // blockpresent (io.c:532-556): the first seven always, the others by the mask
  const uint32_t mask = blocks_mask | 0x7f;
  const TCol *src = reinterpret_cast<const TCol *>(cols);
  if(n > 0 && !src[TC_TYPE].p)
    return refuse(NGRAVS_ERR_ARG, "type must not be NULL");
  // every column of every present block on the device, once; which gas columns are needed is known after the plan, so a gas column
  // that is given is staged, and a missing one is refused below when there is gas
  const int mesh = c->cfg.pmgrid > 0;
  unsigned need = TB(TC_TYPE), gas = 0;
  for(int b = 0; b < B_COUNT; b++)
    if(mask & (1u << b))
      {
        unsigned nb, gb;
        snap_block_columns(b, mesh, &nb, &gb);
        need |= nb, gas |= gb;
      }
  unsigned given_need = 0;
  for(int k = 0; k < TC_COUNT; k++)
    if((need & TB(k)) && (src[k].p || k == TC_TYPE))
      given_need |= TB(k);
  const bool host_cols = !cols->on_device;
  const SnapScratch sc((size_t)buffer_bytes, host_cols && snap->ids ? 4 * (size_t)n : 0,
                       host_cols && (mask & (1u << B_POT)) && snap->potential ? 8 * (size_t)n : 0);
  TimeStage st = {c, cols};
  if((rc = st.begin(refuse, given_need, gas, sc.total)))
    return rc;
  int64_t npart[6];
  if((rc = snap_plan_device(c, refuse, st.d.c[TC_TYPE], n, npart)))
    return rc;
  for(int b = 0; b < B_COUNT; b++)
    if((mask & (1u << b)) && snap_segments(npart, snap->mass_table, b, nullptr) > 0 && (rc = snap_check_block(c, refuse, cols, snap, b)))
      return rc;
  SnapParams p;
  if((rc = snap_params(c, par, snap, reinterpret_cast<double *>(st.scratch + sc.off_tab), true, &p)))
    return rc;
  TCol ids, pot;
  if((rc = snap_extra(c, cols, snap->ids, snap->ids_stride, 4, st.scratch + sc.off_ids, &ids)))
    return rc;
  if((rc = snap_extra(c, cols, (mask & (1u << B_POT)) ? snap->potential : nullptr, snap->potential_stride, 8, st.scratch + sc.off_pot, &pot)))
    return rc;
  SnapSegs sg;
  const long long nall = snap_segments(npart, snap->mass_table, B_POS, &sg);
  if((rc = snap_pos_check(c, refuse, st.d, p, sg, 0, nall, reinterpret_cast<unsigned *>(st.scratch))))
    return rc;
  for(int b = 0; b < B_COUNT; b++)
    if((mask & (1u << b)) && snap_segments(npart, snap->mass_table, b, nullptr) * (snap_is_vector(b) ? 12 : 4) > 0x7fffffffll)
      return refuse(NGRAVS_ERR_ARG, std::string("block ") + snap_name[b] + " does not fit the int record length of the file format");

  // nothing is refused from here on: the file is opened
  FILE *fd = fopen(path, "w");
  if(!fd)
    return refuse(NGRAVS_ERR_ARG, std::string("can't open file `") + path + "' for writing snapshot");   // endrun(123)
  std::vector<unsigned char> hbuf((size_t)buffer_bytes);
  unsigned char header[256];
  const double time = par->comoving ? par->time_begin * exp(snap->ti_current * par->timebase_interval)
                                    : par->time_begin + snap->ti_current * par->timebase_interval;
  snapshot_header(par, snap, npart, npart, 1, time, header);
  bool ok = true;
  int blksize = 256;
  if(snap_format == 2)
    ok = ok && snap_label_record("HEAD", 256 + 2 * (int)sizeof(int), fd);
  ok = ok && snap_fwrite(&blksize, 4, fd) && snap_fwrite(header, 256, fd) && snap_fwrite(&blksize, 4, fd);
  for(int b = 0; b < B_COUNT && ok; b++)
    {
      if(!(mask & (1u << b)))
        continue;
      const long long total = snap_segments(npart, snap->mass_table, b, &sg);
      if(total <= 0)
        continue;
      const long long el = snap_is_vector(b) ? 12 : 4, maxlen = buffer_bytes / el;
      if(snap_format == 2)
        ok = ok && snap_label_record(snap_label[b], (int)(total * el) + 2 * (int)sizeof(int), fd);
      blksize = (int)(total * el);
      ok = ok && snap_fwrite(&blksize, 4, fd);
      for(long long first = 0; first < total && ok; first += maxlen)
        {
          const long long pc = total - first < maxlen ? total - first : maxlen;
          snap_launch(c, st.d, b == B_ID ? ids : pot, p, sg, b, first, pc, st.scratch + sc.off_out);
          if((rc = col_download(c, st.scratch + sc.off_out, 4, (int)(el / 4), pc, hbuf.data(), el, 0, nullptr)))
            {
              fclose(fd);
              return rc;
            }
          ok = ok && snap_fwrite(hbuf.data(), (size_t)(pc * el), fd);
        }
      ok = ok && snap_fwrite(&blksize, 4, fd);
    }
  ok = (fclose(fd) == 0) && ok;
  if(!ok)
    return refuse(NGRAVS_ERR_ARG, std::string("I/O error while writing `") + path + "'");   // my_fwrite: endrun(777)
  return NGRAVS_OK;
}

// ---- find_next_outputtime (run.c:244-361) ---------------------------------------------------------------------------------------------
int snapshot_next_outputtime(const ngravs_time_params_t *par, const ngravs_output_rule_t *rule, int ti_curr, int32_t *ti_next_out)
{
  const Refuse refuse = {nullptr, "ngravs_find_next_outputtime"};
  if(!par || !rule || !ti_next_out)
    return refuse(NGRAVS_ERR_ARG, "a NULL argument");
  if(!(par->timebase_interval > 0))
    return refuse(NGRAVS_ERR_ARG, "timebase_interval must be > 0");
  if(par->comoving && !(par->time_begin > 0))
    return refuse(NGRAVS_ERR_ARG, "comoving: time_begin must be > 0");
  int ti, ti_next = -1, iter = 0;
  double time;
  if(rule->output_list_on)
    {
      if(rule->output_list_length > 0 && !rule->output_list_times)
        return refuse(NGRAVS_ERR_ARG, "output_list_times must not be NULL");
      for(int i = 0; i < rule->output_list_length; i++)
        {
          time = rule->output_list_times[i];
          if(time >= par->time_begin && time <= par->time_max)
            {
              if(par->comoving)
                ti = (int)(log(time / par->time_begin) / par->timebase_interval);
              else
                ti = (int)((time - par->time_begin) / par->timebase_interval);
              if(ti >= ti_curr)
                {
                  if(ti_next == -1)
                    ti_next = ti;
                  if(ti_next > ti)
                    ti_next = ti;
                }
            }
        }
    }
  else
    {
      if(par->comoving ? !(rule->time_bet_snapshot > 1.0) : !(rule->time_bet_snapshot > 0.0))
        return refuse(NGRAVS_ERR_ARG, par->comoving ? "TimeBetSnapshot > 1.0 required for your simulation (endrun 13123)"
                                                    : "TimeBetSnapshot > 0.0 required for your simulation (endrun 13123)");
      time = rule->time_of_first_snapshot;
      while(time < par->time_begin)
        {
          if(par->comoving)
            time *= rule->time_bet_snapshot;
          else
            time += rule->time_bet_snapshot;
          iter++;
          if(iter > 1000000)
            return refuse(NGRAVS_ERR_ARG, "Can't determine next output time (endrun 110)");
        }
      while(time <= par->time_max)
        {
          if(par->comoving)
            ti = (int)(log(time / par->time_begin) / par->timebase_interval);
          else
            ti = (int)((time - par->time_begin) / par->timebase_interval);
          if(ti >= ti_curr)
            {
              ti_next = ti;
              break;
            }
          if(par->comoving)
            time *= rule->time_bet_snapshot;
          else
            time += rule->time_bet_snapshot;
          iter++;
          if(iter > 1000000)
            return refuse(NGRAVS_ERR_ARG, "Can't determine next output time (endrun 111)");
        }
    }
  if(ti_next == -1)
    ti_next = 2 * TI_BASE;   // this will prevent any further output
  *ti_next_out = ti_next;
  return NGRAVS_OK;
}
