// engine.hpp -- internal state of libngravs_hip.so (not part of the C ABI).
//
// Data layout in HBM (all SoA, fp64 as the reference's -DDOUBLEPRECISION build):
//   input columns, caller's order : in_pos[3n] in_mass[n] in_type[n] in_oldacc[n] in_active[n]
//   Peano-sorted particle columns : s_pm[n] = double4{x,y,z,mass}  s_type[n] u8  s_oldacc[n]
//                                   s_active[n] u8  s_key[n] u64 (21 bits/dim)  s_idx[n] u32
//   tree (breadth-first, level-contiguous): n_first/n_count (particle range), n_child[8*nodes]
//       (>=0 node, -1 empty, <=-2 particle -2-p), n_geo = double4{cx,cy,cz,len},
//       n_mom[nodes*NG] = double4{sx,sy,sz,mass}, n_flags (reference bitflags bits 2-5, FLAG_*), n_level
//   results, Peano order          : r_acc[3n] r_nint[n] r_pm[3n] r_oldacc[n]
#pragma once
#include <hip/hip_runtime.h>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <utility>
#include <vector>
#include "../../include/ngravs_host.h"
#include "devbuf.hpp"

#define NG_MAX NGRAVS_MAX_GRAVS
#define NTAB NGRAVS_NTAB
#define TREE_BITS NGRAVS_TREE_BITS
// n_flags bits beyond the reference's bitflags 2-5 (max-softening type, mixed softening)
#define FLAG_BUCKET 64     // bit 6: the node holds its particles directly (deepest level)
#define FLAG_PSEUDO 128    // bit 7: top-level cell whose particles live on another task: global monopoles, no children
#define FLAG_PARTIAL 256   // bit 8: the cell contains particles that are not on this task (never handed over as a leaf)
// bits 9-24: source species (type_to_grav & 3) of up to 8 particles, 2 bits each, written by k_moments for the group walk.
//   range-coded node (FLAG_BUCKET, or at most FLAG_SPECIES_SLOTS particles and not FLAG_PARTIAL): field q = particle first + q
//   any other node: field q = the particle in child slot q (child <= -2)
#define FLAG_SPECIES_SHIFT 9
#define FLAG_SPECIES_SLOTS 8
#define FLAG_SPECIES_MASK (0xffff << FLAG_SPECIES_SHIFT)
#define MAX_LEVELS (TREE_BITS + 1)

struct ngravs_ctx;

#define HIP_TRY(ctx, expr)                                                                        \
  do                                                                                              \
    {                                                                                             \
      hipError_t e__ = (expr);                                                                    \
      if(e__ != hipSuccess)                                                                       \
        {                                                                                         \
          ngravs_report(ctx, NGRAVS_ERR_NO_DEVICE, std::string(#expr) + ": " + hipGetErrorString(e__)); \
          return NGRAVS_ERR_NO_DEVICE;                                                            \
        }                                                                                         \
    }                                                                                             \
  while(0)

void ngravs_report(ngravs_ctx *ctx, int code, const std::string &msg);

// User-defined laws (ngravs_create_with_laws; user_laws.cpp builds the tables, DESIGN.md "User-defined force laws").
// Every table is a run of sub-intervals with a degree-7 polynomial in t in [-1, 1] each (UL_NC coefficients, Horner order
// c[7] .. c[0]).  r-space force of registry entry k: g(r) = r^2 accel(1, 1, r^2, r, 1) over the octaves [2^(e-1), 2^e),
// e = e_lo .. e_lo + n_oct - 1, S sub-intervals of the mantissa each: coef + (k * n_oct + o) * S * UL_NC.  Spline of entry k
// for the i-th distinct softening h[i]: spline(1, 1, h, u h, 1) over u in [0, 1), Ss sub-intervals: spl + ((k * nh + i) * Ss) * UL_NC.
#define UL_NC 8
struct UserTabs
{
  const double *coef, *spl;
  int e_lo, n_oct, S;
  int nh, Ss;
  double h[NGRAVS_NTYPES];
};
__host__ __device__ inline double ul_poly(const double *c, double t)
{
  double v = c[7];
  for(int j = 6; j >= 0; j--)
    v = v * t + c[j];
  return v;
}
// g(r) of entry k: octave and mantissa by frexp (v_frexp_exp_i32_f64 / v_frexp_mant_f64), clamped to the table's ends
__host__ __device__ inline double ul_g(const UserTabs &u, int k, double r)
{
  int e;
  (void)frexp(r, &e);
  int o = e - u.e_lo;
  const double m = ldexp(r, -(u.e_lo + (o < 0 ? 0 : (o >= u.n_oct ? u.n_oct - 1 : o))));   // [0.5, 1) inside the table
  double s = (m - 0.5) * (2 * u.S);
  // outside the table (or r = 0 / NaN) the value at its nearer end: no extrapolated polynomial
  s = o < 0 ? 0.0 : (o >= u.n_oct ? (double)u.S : s);
  o = o < 0 ? 0 : (o >= u.n_oct ? u.n_oct - 1 : o);
  s = s >= 0 ? (s <= u.S ? s : (double)u.S) : 0.0;
  int j = (int)s;
  j = j >= u.S ? u.S - 1 : j;
  return ul_poly(u.coef + ((size_t)(k * u.n_oct + o) * u.S + j) * UL_NC, 2 * (s - j) - 1);
}
__host__ __device__ inline double ul_spline(const UserTabs &u, int k, double h, double r)
{
  if(u.nh == 0)   // no positive softening: r < h never holds (a NaN pair of h = 0 gets no table read)
    return 0.0;
  int i = 0;
  for(int q = 1; q < u.nh; q++)
    if(fabs(u.h[q] - h) < fabs(u.h[i] - h))
      i = q;
  double s = r / h * u.Ss;
  s = s >= 0 ? (s <= u.Ss ? s : (double)u.Ss) : 0.0;   // (NaN -> 0)
  int j = (int)s;
  j = j >= u.Ss ? u.Ss - 1 : j;
  return ul_poly(u.spl + ((size_t)(k * u.nh + i) * u.Ss + j) * UL_NC, 2 * (s - j) - 1);
}

// The model's potential companions (ngravs_create_with_potentials) as the potential walk reads them: the tables of UserTabs with
// p(r) = r pot(1, 1, 0, r, 1) in the place of g(r) and pot_spline(1, 1, h, u h, 1) in the place of the force spline, one table per
// distinct function; kp / ks [target][source]: the table of the pair's pot / pot_spline, -1 for a pair without an entry (cN / cS)
struct PotUser
{
  UserTabs ut;
  int kp[NG_MAX][NG_MAX], ks[NG_MAX][NG_MAX];
};

// constants every kernel needs, passed by value (fits kernarg / SGPRs)
struct WalkParams
{
  int ng, periodic, pm, use_theta;
  int nleaf;                // group walk: an opened node with <= nleaf particles hands over its particles directly (0: only buckets)
  int exact_reach;          // group walk: exact fp64 reach test instead of the packed-fp32 pre-test (ngravs_set_tuning)
  double box, boxhalf;
  double theta2;            // ErrTolTheta^2
  double errtol_acc;        // ErrTolForceAcc
  double rcut, rcut2, asmthfac, utor2wpi, reach2;   // TreePM constants (forcetree.c:1708-1711)
  double ym;                // YUKAWA_IMASS / BoxSize (ngravs.c:859)
  double bam_eps;           // BAM_EPSILON (ngravs.c:45-47)
  double fac_intp;          // 2*NGRAVS_EN/BoxSize: lattice-table lookup scale (forcetree.c:3737)
  double fsoft[NGRAVS_NTYPES];
  int t2g[NGRAVS_NTYPES];
  unsigned t2g_packed;   // the same map, 2 bits per type (register-resident lookups)
  // law coefficients [target][source]: accel = m*(cN/r2 + cY*exp(-r ym)(ym/r + 1/r2)); spline = cS*plummer
  double cN[NG_MAX][NG_MAX], cY[NG_MAX][NG_MAX], cS[NG_MAX][NG_MAX];
  // TreePM short-range tables as the evaluation kernel stages them: identical tables of the symmetric wiring are stored once
  int ntab_lds;                 // distinct tables
  int tab_slot[NG_MAX * NG_MAX];   // [target * ng + source] -> slot
  int slot_src[NG_MAX * NG_MAX];   // slot -> a [target * ng + source] index that holds it
  // Yukawa factor through the table bins: exp(-ym r) = E[tab] * P5(-ym (r - tab/asmthfac)), E[tab] = exp(-ym tab/asmthfac)
  // appended to the table buffer (valid while ym * bin width is small, else 0 and exp() is evaluated in full)
  int exp_tab;
  double inv_asmthfac;
  double ec[4];   // (ym / asmthfac)^k / k!, k = 1..4: the polynomial in the bin fraction
  int src_in_box;   // every particle (and so every node centre of mass) lies inside [0, BoxSize]: groups away from the faces skip the image arithmetic
  // the BAM / NGRAVS_ACCUMULATOR family in the group walk (tree-only wirings): law ids [target][source] and the flag that one is wired
  int bam;
  int law_accel[NG_MAX][NG_MAX], law_spline[NG_MAX][NG_MAX];
  // user-defined laws (tree-only wirings with a user id: then bam = 1 too, which selects the variant that evaluates law ids)
  int user;
  UserTabs ut;
};

struct TreeView
{
  const int *first, *count, *child, *flags;
  const int *npart;        // particles per species below a node (NGRAVS_ACCUMULATOR, allvars.h:645-648); null unless a BAM law is wired
  const double4 *geo, *mom;
  // node head of the group walk: {flags, first, count, float bits of mass_lo} per node, mass_lo = the sum of the node's species
  // masses rounded toward zero to float.  Null unless the tree is a freshly built single-task tree (ngravs_ctx::head_valid) and
  // the tuning walk_head is on: the walk then reads flags, first and count from their own arrays and always fetches the moments
  const int4 *head;
  double head_eps;         // slack of the head's distance bound: 2^-40 x the largest coordinate magnitude of the domain
  int nnodes;
  // start table of the group walk (TreePM only): node index of every cell of one complete tree level, [ix][iy][iz]
  const int *ltab;
  int ltab_level;          // 0: none, walks start at the root
  double ltab_corner[3], ltab_cl;
  // adaptive softening for gas (ngravs_set_gas_softening; read by the ADA instantiations alone, null otherwise)
  const double *soft;      // per sorted particle: Hsml of a type-0 row, fsoft[type] of any other
  const double *maxsoft;   // per node: the largest of them below it (0: empty node)
};

// The counters of a walk (ngravs_ctx::walk_counters): cleared in front of a walk, bumped by its kernels, read by the host after it
struct WalkCounters
{
  int reserved0;
  int err;               // error flag of the walk kernels: 1 a list overflowed, 2 the LIFO, 4 a top leaf that was not imported
  int overflowed;        // split walk: groups in walk_ovf (their lists or LIFO outgrew their region) ...
  int overflowed_lifo;   // ... of them by the LIFO
  int unopened;          // top leaves the walk wanted opened but had to use as monopoles
  int reserved1[3];
  int xcd_next[8];       // the next group of each XCD's segment (the persistent kernels' group assignment; cleared between batches)
  unsigned long long stats[4];   // pool entries, nodes tested, traversal batches, force-loop slots per lane: sums over the groups
  int ntargets;          // length of the compacted target list (walk_tlist)
  int reserved2;
  unsigned long long head[2];    // node head: nodes opened without their moments, nodes that passed its test
  int reserved3[2];
};
static_assert(sizeof(WalkCounters) == 32 * sizeof(int), "WalkCounters: 32 ints");
static_assert(offsetof(WalkCounters, err) == 4 && offsetof(WalkCounters, overflowed) == 8 && offsetof(WalkCounters, overflowed_lifo) == 12 &&
                  offsetof(WalkCounters, unopened) == 16 && offsetof(WalkCounters, xcd_next) == 32 && offsetof(WalkCounters, stats) == 64 &&
                  offsetof(WalkCounters, ntargets) == 96 && offsetof(WalkCounters, head) == 104,
              "WalkCounters: the layout the kernels and the host agree on");

// LDS of the group walk's evaluating kernels: what a workgroup may use, and the block every one of them keeps behind its tables
#define WALK_LDS_BUDGET ((size_t)160 * 1024)
#define WALK_LDS_CONST (40 * sizeof(double))   // exp table (32 entries) + softening length per particle type (8)

// ngravs_set_tuning(): performance / test parameters, set explicitly by the host (no environment variables)
struct Tuning
{
  int walk_fused = 0, walk_waves = 0, walk_lcap = 0, walk_root = 0, walk_compact = 1, walk_spread = 0, walk_exact_reach = 0, walk_sg = 0, walk_nleaf = -1;
  long long walk_batch = 0;
  int sort_full = 0;        // Peano order by one radix sort on all 63 key bits (default: top 42 bits + fix-up of the rare ties)
  int tree_levelwise = 0;   // build the tree level by level (the multi-task path) also for single-task trees
  double dd_keep = 0;       // > 0: the next decompositions will be KEPT for some steps -- import for ALL own particles (not only the active ones), own boxes grown by dd_keep x the domain's side
  int walk_ring = 1;        // TreePM evaluation through the ring-pool kernel (kernels_eval.hip); 0: k_walk_group2<...,2>
  int walk_ring_k = 0;      // ... with at most this many slots per wave (0: as many as fit, at most 8)
  int pm_cus = -1;          // PM beside the walk on this many reserved CUs (-1: chosen per step, 0: PM and walk one after another)
  int walk_head = 1;        // group walk traversal reads the node head (TreeView::head); 0: the separate arrays, moments always fetched
  int walk_tg_sort = 1;     // ngravs_gravity_tree_targets walks its targets in Peano order (0: in the caller's order, for measurements)
  int sph_verbose = 0;      // ngravs_sph_density prints its iteration statistics (targets, rounds, candidates, neighbours) to stdout
};

// The global top of the tree for multi-task runs (force_exchange_pseudodata / force_treeupdate_pseudos, forcetree.c:766-996):
// the reference's adaptive TopNodes[] (domain.c:933-1138), the same on every task.  Every task knows, for every top node, the
// GLOBAL particle count and per-species mass / first moments.  The tree build forces the topology of the top tree from the
// global counts, so that it is the single-task tree's; a top LEAF whose particles are not on this task becomes a pseudo node
// (global monopoles, no children).
#define TOP_CW(ng) (7 + 4 * (ng))   // doubles per node: count (leaf sums: work), particles per type [6], per species m, m x, m y, m z
struct TopTree
{
  double total_count = 0;   // particles of all tasks (the root's count of the last ngravs_dd_set_top)
  bool on = false;                     // sums + presence are set: the next tree build forces the global top (ngravs_dd_set_top)
  double import_reach = 0;             // short-range reach (units of Asmth) the import decision was made for (walk mode at set_top)
  ngravs_toptree h = {0, 0, 0, 0, nullptr, nullptr, nullptr, nullptr, nullptr};   // host copy: child, level, xyz, leaf numbers
  DevBuf<int> child, leaf;             // per node: first child or -1; leaf number (curve order) or -1
  DevBuf<int> gcnt;                    // per node: global particle count
  DevBuf<unsigned char> info;          // per node: bits 0-2 octant in its parent (x << 2 | y << 1 | z), bit 3 PARTIAL
  DevBuf<double> gsum;                 // per node: TOP_CW doubles
  DevBuf<int> leaf_owner;              // per leaf
  DevBuf<unsigned long long> reqmask;  // per leaf: tasks that asked for its particles
  DevBuf<double> leaf_sums;            // per leaf: TOP_CW doubles of the own particles (+ 1 spare word)
  // ---- kept decomposition (the steps on which domain.c:76 keeps domain and tree: ngravs_host_kept_step) ----
  DevBuf<int> own_leaf;                // per own row: its top leaf at the decomposition (ngravs_dd_pack_leaves); rows stay, positions drift
  long long own_leaf_n = -1;           // own rows it covers (-1: none kept)
  int kept_rank = -1, kept_world = 0;
  std::vector<int> h_leaf_owner;       // host copies of the last decomposition's plan
  std::vector<unsigned char> h_present;
  std::vector<double> h_node_sums;
  DevBuf<int> kept_row;                // kept decomposition: the own row in every slot of the leaf-import records (k_dd_fill's order)
  std::vector<int64_t> kept_counts;    // ... records per receiving task
  long long kept_total = -1;
  DevBuf<double> kept_sums;            // per leaf: TOP_CW + 1 doubles (the last one: the grown side of the leaf's cell, from its owner) + 1 status word
  DevBuf<double> leaf_len;             // per leaf: grown side of its cell (all tasks' maximum), for the pseudo nodes of a refit
  ~TopTree() { ngravs_host_toptree_free(&h); }
};

// slab-decomposed particle mesh of the multi-task path (kernels_pmslab.hip)
struct PmSlab
{
  int world = 0, rank = 0, N = 0, stage = -1;
  int xs = 0, nx = 0, ys = 0, ny = 0;      // own x-slab of the real mesh, own y-slab of the transposed k-space
  int lo[3] = {0, 0, 0}, ext[3] = {0, 0, 0};   // brick: the mesh cells (lo + i) mod N the own particles' CIC clouds touch
  int elo[3] = {0, 0, 0}, eext[3] = {0, 0, 0}; // the same +-2 cells (4-point gradient)
  std::vector<int> bbox;                   // lo[3], ext[3] of every task's brick
  std::vector<int64_t> scount, rcount;     // doubles per peer of the stage being exchanged
  long long edesc_off = 0;                 // stage 3: where the extended-brick plane descriptors start in desc
  DevBuf<double> brick, slab, tbuf, ebrick, fmesh, send, recv;
  DevBuf<long long> desc;
  std::vector<long long> hdesc[2];         // host copies of the descriptor tables in flight (upload_desc)
  int hdesc_turn = 0;
  void *plan2f = nullptr, *plan2i = nullptr, *plan1 = nullptr;
  int plan_N = 0, plan_nx = 0, plan_ny = 0;
  double bytes_sent[4] = {0, 0, 0, 0};     // payload of the last step's four exchanges (this task, bytes)
};

struct ngravs_ctx
{
  ngravs_config_t cfg;
  Tuning tune;
  // Members are destroyed in reverse order of declaration: the streams stand before every buffer and event, so that these go
  // first and the streams last.  own_stream: the stream ngravs_create* made (`stream` is a plain handle, OnStream reassigns it);
  // pm_stream / walk_stream: PM beside the walk (ngravs_compute_accelerations), masked to disjoint sets of CUs
  DevStream own_stream, pm_stream, walk_stream;
  PmSlab pms;
  TopTree top;
  DevBuf<int> n_top;          // top-tree node a tree node is (multi-task trees; -1: none)
  ngravs_fatal_fn on_fatal = nullptr;
  hipStream_t stream = nullptr;
  double asmth = 0, rcut = 0;
  int64_t n = 0;           // particles in the working set (own + halo copies)
  int64_t n_local = 0;     // own particles: the first n_local of the input columns
  bool extent_override = false;
  double ext_lo[3], ext_hi[3];
  int dd_last_what = -1;
  long long dd_last_sent = 0;
  bool have_particles = false, have_order = false, have_tree = false, have_pm = false, have_acc = false;
  bool pm_parked = false;     // pm_orig holds the caller's GravPM (handed over with ngravs_set_particles)
  double dom[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  double pos_lo[3] = {0, 0, 0}, pos_hi[3] = {-1, -1, -1};   // extent of all positions the current decomposition saw (all tasks)
  int64_t shard_first = 0, shard_count = 0;

  // inputs (caller order)
  DevBuf<double> in_pos, in_mass, in_oldacc;
  DevBuf<double> in_cost;      // P[].GravCost (interactions of the particle's last walk): the work weight of the domain cut
  DevBuf<int> in_type;
  DevBuf<unsigned char> in_active;
  DevBuf<double2> in_rec;      // packed 48-byte records of the caller-order columns (dom_keys_and_sort)
  DevBuf<unsigned long long> in_key;
  DevBuf<long long> in_id;
  // multi-task decomposition scratch
  DevBuf<unsigned long long> dd_mask, dd_counts;
  int sort_low = 35;   // key bits the two-stage sort leaves to its fix-up (35 -> 28 -> 21 -> 0 = plain sort, as runs of ties get too long)
  long long own_order_nlocal = -1, own_order_len = 0;   // s_idx still is the Peano order of the last local decomposition (of own_order_len rows, own_order_nlocal of them own)
  DevBuf<unsigned char> dd_send, dd_recv;
  // sorted
  DevBuf<double4> s_pm;
  DevBuf<unsigned char> s_type, s_active;
  DevBuf<double> s_oldacc;
  DevBuf<unsigned long long> s_key;
  DevBuf<unsigned int> s_idx, idx_iota;
  DevBuf<unsigned char> sort_tmp;
  DevBuf<double> red_tmp;
  // tree
  int64_t max_nodes = 0, nnodes = 0;
  bool tree_refit = false;    // the tree was refit since it was built (cells may have grown)
  bool tree_stale = false;    // ngravs_update_particles was called: the columns of the sorted set are out of date
  int nlevels = 0;
  DevBuf<int> lvl_table;      // see TreeView::ltab
  int lvl_table_level = 0;
  int64_t level_start[MAX_LEVELS + 2];
  DevBuf<int> n_first, n_count, n_child, n_flags, n_nchild;
  DevBuf<double4> n_geo, n_mom;
  DevBuf<int4> n_head;        // see TreeView::head (written by k_moments of a build)
  bool head_valid = false;    // n_head matches n_flags / n_first / n_count / n_mom: set by the build, cleared by whatever alters them afterwards
  DevBuf<int> tb_count;   // one-pass build: per-level node counts of every block of particles
  DevBuf<int> n_npart;        // [nodes][NG] particle counts per species (BAM wirings only)
  DevBuf<int> scan_out;
  DevBuf<unsigned char> scan_tmp;
  DevBuf<int> d_counters;
  DevBuf<int> d_levels;        // tree build: first node / node count of every level (device-resident level table)
  long long level_hint[MAX_LEVELS + 2] = {0};   // level populations of the previous build (launch sizing only)
  // walk
  DevBuf<double> table;       // [ng][ng][NTAB] shortrange_fourier_force
  bool table_ready = false;
  DevBuf<double> lat;         // [ng][ng][3][65^3] Ewald / lattice-sum force corrections (periodic tree-only, periodic direct sum)
  bool lat_ready = false;
  DevBuf<int> walk_stack;     // per-wave scratch
  DevBuf<int> walk_tlist;     // compacted active targets of the shard (individual timesteps), Peano order
  DevBuf<unsigned char> walk_tmp;
  long long walk_ntargets = -1;   // >= 0: the group walk runs over walk_tlist[0..walk_ntargets)
  bool walk_dense_tlist = false;  // ... and that list is the own rows of a multi-task working set, nearly all of them active
  int walk_spread = 0;        // > 1: every group of 64 targets is walked as `spread` sub-groups by the fused kernel
  int walk_sg = 1;            // split walk: groups per traversal unit (shared item lists) of the last launch
  long long walk_unopened = 0;   // top leaves the last group walk wanted opened but had to use as monopoles (not imported)
  long long walk_moment_skips = 0, walk_head_survivors = 0;   // last group walk: nodes opened without their moments / nodes within reach (0 without a head)
  int walk_unit_state = 4;    // groups per traversal unit the TreePM walk is in (4, 2 or 1): changed with hysteresis on walk_ia_ratio
  double walk_ia_ratio = 0;   // pairs per target of the last TreePM group walk / what a uniform box of the same mean density gives
                              // (0: no such walk yet): > 1 in clustered sets, where smaller traversal units accept more cells
  bool all_active = true;     // the caller passed no active flags
  DevBuf<int> walk_ovf;       // split walk: groups left to the fused kernel (lists or LIFO outgrew their region)
  DevBuf<WalkCounters> walk_counters;   // one: what each field is stands with the struct
  DevBuf<double> r_acc, r_pm, r_oldacc;
  DevBuf<int> r_nint;
  // pm
  int pm_plan_n = 0;
  void *fft_fwd = nullptr, *fft_inv = nullptr;   // hipfftHandle (int) boxed
  DevBuf<double> pm_rho;      // [ng][N][N][N+2] real / complex in place
  DevBuf<double> pm_force;     // [N][N][N][3]: finite-difference force mesh of one target species (two-pass gather)
  DevBuf<double> pm_phi;      // [ng][N][N][N+2]
  DevBuf<double> pm_orig;     // GravPM in caller order (persists between PM steps)
  // staging for results
  DevBuf<double> out_tmp;
  DevBuf<float> out_tmpf;
  std::vector<unsigned char> host_stage;
  ngravs_stats_t stats;
  DevEvent ev0, ev1, evk0, evk1;
  std::vector<DevEvent> ev_batch;   // split walk: 3 events per batch (before traversal, between, after evaluation)
  int walk_batches = 0;               // batches of the last split walk (0: fused kernel)
  int walk_lcap = 0;                  // split walk: item-list capacity per group and species (grown on overflow)
  int walk_scap = 0;                  // split walk: LIFO capacity per group (grown on overflow)
  bool walk_used_split = false;       // walk_enqueue -> walk_complete: the split kernels ran (leftover units may follow)
  long long walk_cap_n = -1;          // split walk: scratch budget from hipMemGetInfo, asked again only when the particle count or
  size_t walk_cap_stack = 0;          // the size of the scratch itself has changed
  size_t walk_cap_bytes = 0;
  std::vector<std::pair<const void *, size_t>> walk_lds_set;   // walk kernels whose dynamic-LDS limit is set, and to what
  std::string last_error;
  // user-defined laws (ngravs_create_with_laws)
  std::vector<ngravs_user_fn_t> user_fns;
  std::vector<ngravs_user_lattice_t> user_lat;   // the model's lattice corrections (ngravs_create_with_lattice), tabulated in ensure_lattice
  DevBuf<double> user_tab;    // accel tables, then spline tables (UserTabs)
  UserTabs user_ut = {};
  bool user_ready = false;
  double user_soft[NGRAVS_NTYPES] = {0, 0, 0, 0, 0, 0};   // the softenings the tables were built for
  int last_walk_kernel = 0;   // NGRAVS_KERNEL_*
  // adaptive softening for gas (ngravs_set_gas_softening): the caller's lengths, own rows in caller order; what the walks read
  // is derived from them on demand (adaptive_refresh)
  bool gsoft_on = false;
  bool gsoft_col_stale = true, gsoft_node_stale = true;
  DevBuf<double> in_gsoft;    // [n_local] caller order; rows of other types hold 0
  DevBuf<double> gsoft_stage; // the next column while ngravs_set_gas_softening checks it
  DevBuf<double> s_soft;      // TreeView::soft
  DevBuf<double> n_maxsoft;   // TreeView::maxsoft
  // PM beside the walk: pm_stream and walk_stream (above)
  int pm_stream_cus = 0;      // CUs of pm_stream's mask (0: no masked streams); walk_stream has the device's other CUs
  int device_cus = 0;         // CUs of the device
  int stream_cus = 0;         // CUs the launches on c->stream may use (0: the whole device); set by OnStream
  int last_pm_cus = 0;        // CUs PM ran on beside the walk in the last step (0: one after another)
  double pm_solo_ms = 0, walk_solo_ms = 0;   // PM and walk spans of the last serial PM step of the particle set ...
  int pm_solo_steps = 0;      // ... of this many
  int pm_auto_cus = -1;       // the CUs chosen from them (-1: not yet)
  DevEvent ev_fork, ev_pm0, ev_pm1, ev_walk;
  DevBuf<int> probe_out;      // ngravs_cu_probe
  DevBuf<double> user_green;  // PM: user Green's functions G(k2) at the integer k2 (GreenParams::ug); empty without a user greens id
  long long user_green_nk2 = 0;
  // SPH density (ngravs_sph_density, kernels_sph.hip): buffers of its own, the walk's state is not touched
  DevBuf<double> sph_vel_in, sph_h_in;   // the caller's VelPred[3] and Hsml columns (own rows, caller order)
  DevBuf<double> sph_vel;                // VelPred in Peano order (sources are read through it)
  DevBuf<int> sph_tlist;                 // active type-0 own rows, Peano order
  DevBuf<unsigned char> sph_tmp;
  DevBuf<double> sph_res;                // [SPH_NRES][targets], list order
  DevBuf<int> sph_row, sph_rounds;       // per target: caller row, rounds taken
  DevBuf<unsigned long long> sph_counters;
  // SPH hydro force (ngravs_sph_hydro): the node hmax lives here, not in n_geo / n_mom, which gravity reads
  DevBuf<double> sph_col_in;             // the caller's Density, Pressure, DhsmlDensityFactor, DivVel, CurlVel columns, [5][own rows]
  DevBuf<int> sph_ts_in;                 // the caller's timestep column
  DevBuf<double> sph_hsrc;               // [SPH_HS_NCOL][n], Peano order: what hydro_evaluate needs of one gas particle
  DevBuf<double> sph_hmax;               // per tree node: largest Hsml of the type-0 particles below it (0: no gas)
  // the gas side in one call (ngravs_sph_accelerations); empty until it is used
  DevBuf<double> sph_gas_in;             // the caller's Entropy and DtEntropy columns, [2][own rows]
  DevBuf<int> sph_ti_in;                 // the caller's Ti_begstep and Ti_endstep columns, [2][own rows]
  DevBuf<int> sph_tpos;                  // per sorted particle: its place in sph_tlist, -1 when it is no target
  // the first smoothing-length guess (ngravs_sph_hsml_guess); empty until it is used
  DevBuf<double> sph_gmass;              // [n + 1], Peano order: gas mass of the rows before a row (inclusive scan shifted by one)
  DevBuf<int> sph_gcount;                // [n + 1]: gas rows before a row
  // sums for targets that are not own rows (ngravs_sph_density_sums / ngravs_sph_hydro_sums); empty until they are used
  DevBuf<double> sph_tg_in;              // the caller's target columns, caller order: pos[nt][3], vel[nt][3], then one column each
  DevBuf<int> sph_tg_ts;                 // the targets' timestep column
  DevBuf<unsigned long long> sph_tg_key; // [2][nt]: the targets' Peano keys (coordinates clamped to the domain cube), unsorted and sorted
  DevBuf<unsigned int> sph_tg_ord;       // [2][nt]: 0 .. nt-1, and the caller's indices in Peano order
  DevBuf<double> sph_tg_res;             // [nt][7] or [nt][5], caller order: copied out only when the whole call succeeded
  // gravity for targets that are not own rows (ngravs_gravity_tree_targets / ngravs_pm_targets); empty until they are used.  The
  // walk's own results (r_acc, r_nint, walk_counters, walk_tlist) are never written by these calls
  DevBuf<double> gt_in;                  // the caller's target columns, caller order: pos[nt][3], old_acc[nt], mass[nt]; then the positions clamped to the domain cube [nt][3]
  DevBuf<int> gt_type;                   // the targets' types
  DevBuf<unsigned long long> gt_key;     // [2][nt]: the targets' Peano keys, unsorted and sorted
  DevBuf<unsigned int> gt_ord;           // [2][nt]: 0 .. nt-1, and the caller's indices in Peano order
  DevBuf<unsigned char> gt_tmp;          // scratch of the radix sort
  DevBuf<double> gt_acc;                 // [nt][3], caller order: copied out only when the whole call succeeded
  DevBuf<int> gt_nint;                   // [nt]
  DevBuf<unsigned long long> gt_counters;   // GT_C_*: refused records, the farthest target, the walk's flag word
  // pm_phi holds the complete potentials of the last single-mesh PM step (pm_finish); false before one, while they are being
  // rewritten, and when the last PM step went through the slab path, which has no whole mesh
  bool pm_mesh_valid = false;
  // potentials (kernels_potential.hip); empty until ngravs_compute_potential / ngravs_potential_targets are used
  DevBuf<double> pot_table;   // [ng][ng][NTAB]: E = (force_tab + pot_tab) u, the long-range potential tempI / u of the TreePM split
  bool pot_table_ready = false;
  DevBuf<double> pot_lat;     // [ng][ng][65^3]: sign(law) ewald_psi / BoxSize on the octant grid of `lat` (periodic tree-only)
  bool pot_lat_ready = false;
  // the model's potential companions (ngravs_create_with_potentials): the entries, their distinct pot / pot_spline functions as a
  // registry of kinds NGRAVS_USER_POT / NGRAVS_USER_POT_SPLINE, and the tables of that registry (user_pot_tables_ensure)
  std::vector<ngravs_user_potential_t> user_pot;
  std::vector<ngravs_user_fn_t> upot_fns;
  DevBuf<double> upot_tab;
  UserTabs upot_ut = {};
  bool upot_ready = false;
  double upot_soft[NGRAVS_NTYPES] = {0, 0, 0, 0, 0, 0};
  DevBuf<double> r_pot;      // [n], Peano order: the walk's sum, then the finished potential
  // pm_phi holds the potentials of the mesh of the last ngravs_compute_potential, at the positions of that call; cleared by the
  // next deposit and by every hand-over of particles
  bool pot_mesh_valid = false;
  double pot_walk_ms = 0;     // device time of the walk kernel of the last ngravs_compute_potential
  // time integration (kernels_time.hip): counters, the decided steps of one advance call, the look-up tables, and the device
  // copies of host columns; nothing in it outlives a call
  DevBuf<unsigned char> time_buf;
  // the snapshot plan (kernels_snapshot.hip): the file order of the rows of the last ngravs_snapshot_plan, order[dest] = source
  // row, for snap_n rows (-1: no plan) with snap_npart[type] of each type; snap_tmp holds the partition's counts and bases
  DevBuf<int> snap_order, snap_tmp;
  long long snap_n = -1;
  int64_t snap_npart[NGRAVS_NTYPES] = {0, 0, 0, 0, 0, 0};
};

// Routes the context's launches to stream `s`, whose CU mask leaves them `cus` CUs, until the end of the scope (the kernels
// enqueue on c->stream, and the persistent ones size their grids by c->stream_cus)
struct OnStream
{
  ngravs_ctx *c;
  hipStream_t s0;
  int n0;
  OnStream(ngravs_ctx *c_, hipStream_t s, int cus) : c(c_), s0(c_->stream), n0(c_->stream_cus)
  {
    c->stream = s;
    c->stream_cus = cus;
  }
  ~OnStream()
  {
    c->stream = s0;
    c->stream_cus = n0;
  }
};

// ---- kernels_domain.hip
int dom_find_extent(ngravs_ctx *c);
int dom_keys_and_sort(ngravs_ctx *c);
int dom_keys_only(ngravs_ctx *c, const double *d_pos, int64_t n, const double corner[3], double fac, int bits,
                  long long *d_keys);
int dd_local_extent(ngravs_ctx *c, double lo[3], double hi[3]);
void dd_apply_extent(ngravs_ctx *c, const double lo[3], const double hi[3]);
int dd_set_toptree(ngravs_ctx *c, int nnode, const int *child);
int dd_leaf_sums(ngravs_ctx *c, void **dev_sums, int64_t *count);
int dd_pack(ngravs_ctx *c, int what, const int *leaf_owner, int nranks, int me, int64_t *counts, void **dev_records, int64_t *nrec);
int dd_apply_migration(ngravs_ctx *c, const void *dev_records, int64_t nrec);
int dd_get_dest(ngravs_ctx *c, const int *leaf_owner, int *dest);
int dd_target_bounds(ngravs_ctx *c, double out[2]);
int dd_pack_leaves(ngravs_ctx *c, const unsigned long long *reqmask, int nranks, int me, int64_t *counts, void **dev_records, int64_t *nrec);
int dd_set_top(ngravs_ctx *c, const double *node_sums, const unsigned char *present);
int dd_set_halo(ngravs_ctx *c, const void *dev_records, int64_t nrec);
int dd_leaf_sums_kept(ngravs_ctx *c, void **dev_sums, int64_t *count);
int dd_pack_leaves_kept(ngravs_ctx *c, int64_t *counts, void **dev_records, int64_t *nrec);
int dd_refresh_halo(ngravs_ctx *c, const void *dev_records, int64_t nrec);
int dd_update_top(ngravs_ctx *c, const double *node_sums, const double *leaf_len);
int dd_peano_order_own(ngravs_ctx *c, int force);
int dd_fill_ids(ngravs_ctx *c);
int dd_record_doubles(const ngravs_ctx *c, int what);
// ---- kernels_tree.hip
int tree_build(ngravs_ctx *c);
int tree_moments(ngravs_ctx *c, bool refit, bool counts = false);
int tree_top_leaf_len(ngravs_ctx *c, double *dev_kept_sums, int stride);   // kept steps: the grown sides of the own top leaves' cells
int tree_top_refit(ngravs_ctx *c);   // kept steps: moments of the top nodes from the new global sums, their sides from the leaves' up
int dom_regather(ngravs_ctx *c);
static inline bool cfg_has_bam(const ngravs_config_t &cfg)
{
  for(int i = 0; i < cfg.n_gravs; i++)
    for(int j = 0; j < cfg.n_gravs; j++)
      if((cfg.law_accel[i][j] >= NGRAVS_LAW_BAMBAM && cfg.law_accel[i][j] < NGRAVS_LAW_USER0) ||
         (cfg.law_spline[i][j] >= NGRAVS_SPLINE_BAMBAM && cfg.law_spline[i][j] < NGRAVS_SPLINE_USER0))
        return true;
  return false;
}
static inline bool cfg_has_user(const ngravs_config_t &cfg)
{
  for(int i = 0; i < cfg.n_gravs; i++)
    for(int j = 0; j < cfg.n_gravs; j++)
      if(cfg.law_accel[i][j] >= NGRAVS_LAW_USER0 || cfg.law_spline[i][j] >= NGRAVS_SPLINE_USER0)
        return true;
  return false;
}
// ---- user_laws.cpp
int user_check_config(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, const ngravs_user_lattice_t *lat, int nlat,
                      std::string &why);
// the lattice function of pair (a, b) (nullptr: none); whether every pair wired with a user accel id has one
ngravs_lattice_fn user_lattice_fn(const ngravs_ctx *c, int a, int b);
bool user_lattice_complete(const ngravs_ctx *c);
// samples fn into out[3][65^3] / box^2 on host threads; NGRAVS_ERR_WIRING with the first non-finite point in `why`
int user_lattice_tabulate(ngravs_lattice_fn fn, double box, double *out, std::string &why);
void ngravs_report(ngravs_ctx *ctx, int code, const std::string &msg);
int user_tables_ensure(ngravs_ctx *c, double r_need);
// The r_need of a law's or a potential's tables, a quarter to spare: the largest distance a pair is evaluated at.  shortrange: a
// walk, which a mesh cuts at the end of the short-range table; not the direct sum.  far: the largest distance of a target from
// the domain's centre (0: own rows)
double table_reach(const ngravs_ctx *c, bool shortrange, double far);
int user_green_ensure(ngravs_ctx *c);   // PM: the G(k2) tables of the user greens ids   // (re)build the tables if r_need or the softenings are not covered
double user_normed(const ngravs_user_fn_t *fns, int nfns, int law, double k2);
// the potential entries of ngravs_create_with_potentials: the creation checks; the entry of pair (a, b) (nullptr: none); the
// registry of distinct functions and the pair -> table maps; the tables for walks that reach r_need; one lattice table
// out[65^3] = fn / box, the origin zero / box, sampled on host threads
int user_check_potentials(const ngravs_config_t *cfg, const ngravs_user_potential_t *pots, int npot, std::string &why);
const ngravs_user_potential_t *user_pot_entry(const ngravs_ctx *c, int a, int b);
void user_pot_registry(ngravs_ctx *c);
void user_pot_maps(const ngravs_ctx *c, PotUser *pu);
int user_pot_tables_ensure(ngravs_ctx *c, double r_need);
int user_pot_lattice_tabulate(ngravs_lattice_pot_fn fn, double zero, double box, double *out, std::string &why);
// ---- kernels_walk.hip
void make_walk_params(const ngravs_ctx *c, WalkParams *wp);
int walk_run(ngravs_ctx *c);        // walk_enqueue + walk_complete
int walk_enqueue(ngravs_ctx *c);
int walk_complete(ngravs_ctx *c);
int walk_finish(ngravs_ctx *c);
// hipFuncAttributeMaxDynamicSharedMemorySize of a walk kernel: set when the kernel is first launched with this size, not on every
// step (the call takes the runtime's locks in front of the step's first walk launch).  The record is this engine's, the attribute the
// process's: two live engines that launch one kernel with different sizes (walk_ring_k 4 and the default, say) must not share a process
int walk_dyn_lds(ngravs_ctx *c, const void *kern, size_t lds);
int direct_run(ngravs_ctx *c, const int *d_idx, int64_t nt, double *d_acc);
int direct_run_targets(ngravs_ctx *c, const double4 *d_tpm, const int *d_ttype, int64_t nt, double *d_acc, double far = 0);   // far: as table_reach
// adaptive softening: s_soft from in_gsoft and the order, n_maxsoft bottom-up from the tree (nodes: also the node column), each
// only when stale
int adaptive_refresh(ngravs_ctx *c, bool nodes);
// The strict walk for target records that are not own rows.  Reads gt_in (pos, old_acc, mass) and gt_type; counts refused records
// (st: type outside 0..5, position not finite or outside [0, BoxSize] in a periodic run -- nothing is walked then), orders the
// targets along the Peano curve of the engine's domain, walks and writes gt_acc (x G) / gt_nint in caller order.
enum { GT_C_BADTYPE = 0, GT_C_BADPOS, GT_C_FAR, GT_C_FLAG, GT_C_COUNT };
struct GravTargetsStats
{
  long long bad_type, bad_pos;
};
int grav_targets_check(ngravs_ctx *c, long long nt, GravTargetsStats *st, double *far);   // far: the largest distance of a target from the domain's centre
int walk_targets_run(ngravs_ctx *c, long long nt, double far);
TreeView tree_view(ngravs_ctx *c);
// the order the targets of gt_in are walked in: gt_ord's 0 .. nt-1, or (walk_tg_sort) the caller's indices along the Peano curve
int grav_targets_order(ngravs_ctx *c, long long nt, const unsigned int **ord);
// ---- kernels_potential.hip
// The potential walk over ALL own rows into r_pot, self term, LatticeZero term, G, mesh part and the cosmological term (potential.c:
// 244-337); the column in caller order -> d_out[n_local] (a device buffer of the caller's).  nint: r_nint is NOT written; d_nint
// (may be null) gets the interaction counts in caller order.
int potential_run(ngravs_ctx *c, const ngravs_time_params_t *par, double *d_out, int *d_nint);
// the walk x G (+ the mesh part with a mesh) at the targets of gt_in / gt_type -> gt_acc[nt], gt_nint[nt], caller order
// far: the largest distance of a target from the domain's centre (grav_targets_check), for the reach of the model's potential tables
int potential_targets_run(ngravs_ctx *c, long long nt, double far);
int potential_lattice_ensure(ngravs_ctx *c);
// ---- kernels_eval.hip
int eval_ring_slots(const WalkParams &wp, bool yuk, int waves);
int launch_eval_ring(ngravs_ctx *c, const TreeView &tv, const WalkParams &wp, bool yuk, int nblk, int waves, int K, const int *region,
                     const int *gcount, long long g0, long long nb, int lcap, int scap, int S, const int *tlist, int SG, long long t_count);
// ---- kernels_sph.hip
// The SPH spline and its derivative at u = r/h < 1 (density.c:541-550, coefficients allvars.h:109-115), as host and device evaluate it
#define SPH_KC1 2.546479089470
#define SPH_KC2 15.278874536822
#define SPH_KC3 45.836623610466
#define SPH_KC4 30.557749073644
#define SPH_KC5 5.092958178941
#define SPH_KC6 (-15.278874536822)
#define SPH_NORM_COEFF 4.188790204786
#define SPH_MAXITER 150   // allvars.h:97
__host__ __device__ inline void sph_spline(double u, double hinv3, double hinv4, double *wk, double *dwk)
{
  if(u < 0.5)
    {
      *wk = hinv3 * (SPH_KC1 + SPH_KC2 * (u - 1) * u * u);
      *dwk = hinv4 * u * (SPH_KC3 * u - SPH_KC4);
    }
  else
    {
      *wk = hinv3 * SPH_KC5 * (1.0 - u) * (1.0 - u) * (1.0 - u);
      *dwk = hinv4 * SPH_KC6 * (1.0 - u) * (1.0 - u);
    }
}
enum { SPH_HSML = 0, SPH_DENSITY, SPH_NUMNGB, SPH_DIVVEL, SPH_CURLVEL, SPH_DHSML, SPH_NRES };
struct SphStats
{
  long long targets, bad_hsml, failed, stack_ovf, max_rounds, sum_rounds, candidates, neighbours;
};
// compacts the targets into sph_tlist, then iterates every target's smoothing length to acceptance in one launch: reads sph_vel
// (Peano order) and sph_h_in (caller order), writes sph_res / sph_row / sph_rounds in list order
int sph_density_run(ngravs_ctx *c, double des_num_ngb, double max_dev, double min_hsml, SphStats *st);
// setup_smoothinglengths (init.c:229-247) on the device tree: lists the type-0 rows (only_unset: those whose sph_h_in value is not
// > 0), writes their guesses to sph_res [rows] / sph_row in list order.  bad_mass: type-0 rows whose mass is <= 0 or not finite
// (nothing is computed then).
int sph_hsml_guess_run(ngravs_ctx *c, double des_num_ngb, int only_unset, long long *rows, long long *bad_mass);
// SPH hydro force.  Columns of sph_hsrc: VelPred[3], Hsml (0 for rows of other types), Density, Pressure / Density^2 *
// DhsmlDensityFactor, the sound speed as a source (hydra.c:441-442), f2 (hydra.c:504-506), the timestep, the sound speed and f1 as
// a target (hydra.c:379-382)
enum { SPH_HS_VX = 0, SPH_HS_VY, SPH_HS_VZ, SPH_HS_H, SPH_HS_RHO, SPH_HS_POR2, SPH_HS_CSJ, SPH_HS_F2, SPH_HS_TS, SPH_HS_CSI, SPH_HS_F1,
       SPH_HS_NCOL };
enum { SPH_HY_ACCX = 0, SPH_HY_ACCY, SPH_HY_ACCZ, SPH_HY_DTENTR, SPH_HY_MAXSIG, SPH_HY_NRES };
struct SphHydroParams
{
  int periodic, comoving, limiter, have_ts;
  double box, boxhalf;
  double hubble_a2, fac_mu, fac_vsic_fix;   // hydra.c:78-97 (1 when not comoving)
  double visc, tbi, gamma;                  // All.ArtBulkViscConst, All.Timebase_interval, GAMMA
};
struct SphHydroStats
{
  long long targets, bad_hsml, bad_density, bad_pressure, stack_ovf, candidates, pairs;
};
// reads sph_vel_in, sph_h_in, sph_col_in, sph_ts_in (caller order); fills sph_hsrc and sph_hmax, compacts the targets and walks
// once; writes sph_res [SPH_HY_NRES][targets] / sph_row in list order (nothing when a column held a bad value)
int sph_hydro_run(ngravs_ctx *c, const SphHydroParams &hp, SphHydroStats *st);
// The gas side in one call: sph_res [SPH_GAS_NRES][targets] = the density columns, the pressure, the hydro columns
enum { SPH_GAS_PRESSURE = SPH_NRES, SPH_GAS_HYDRO, SPH_GAS_NRES = SPH_GAS_HYDRO + SPH_HY_NRES };
struct SphGasParams
{
  double des, dev, minh;   // All.DesNumNgb, All.MaxNumNgbDeviation, All.MinGasHsml
  int ti_current, have_dte;   // All.Ti_Current; whether sph_gas_in holds a DtEntropy column
};
// reads sph_vel (Peano order), sph_h_in, sph_col_in, sph_gas_in, sph_ti_in (caller order); compacts the targets once, walks for
// the density, derives pressure and hydro sources on the device, walks for the forces; writes sph_res [SPH_GAS_NRES][targets] /
// sph_row in list order.  Returns after the density walk (ds says why) when a target's hsml was bad or MAXITER was reached.
// ev_density / ev_prep are recorded after the density walk and after the hmax pass.
int sph_gas_run(ngravs_ctx *c, const SphGasParams &gp, const SphHydroParams &hp, SphStats *ds, SphHydroStats *hs, hipEvent_t ev_density,
                hipEvent_t ev_prep);
struct SphScatterCols
{
  unsigned char *dst[SPH_GAS_NRES];   // NULL: not wanted
  long long stride[SPH_GAS_NRES];
};
// list order -> the targets' rows of every wanted strided device column, one launch
int sph_scatter_cols(ngravs_ctx *c, long long nt, const SphScatterCols &cols);
// list order -> rows of a strided device column
int sph_scatter(ngravs_ctx *c, const double *src, long long nt, double *dst, long long stride);
// ---- sums for targets that are not own rows: the reference's density_evaluate(j, 1) / hydro_evaluate(j, 1) -------------------------
enum { SPH_SUM_RHO = 0, SPH_SUM_NGB, SPH_SUM_DHR, SPH_SUM_DIV, SPH_SUM_ROTX, SPH_SUM_ROTY, SPH_SUM_ROTZ, SPH_NSUMS };   // density.c:531-575
// columns of sph_tg_in behind pos[nt][3] and vel[nt][3]: density targets hold SPH_TG_H only
enum { SPH_TG_H = 6, SPH_TG_MASS, SPH_TG_RHO, SPH_TG_P, SPH_TG_DHSML, SPH_TG_F1, SPH_TG_NCOL };
struct SphSumsStats
{
  long long bad_hsml, bad_density, bad_pressure, bad_pos, stack_ovf, candidates, pairs;
};
// reads sph_tg_in (pos, vel, SPH_TG_H) and sph_vel (Peano order); orders the targets along the Peano curve, walks ONE round and
// writes the raw sums to sph_tg_res [nt][SPH_NSUMS] in caller order (nothing is walked when a target was bad)
int sph_density_sums_run(ngravs_ctx *c, long long nt, SphSumsStats *st);
// reads sph_tg_in (all columns), sph_tg_ts and the own-row columns sph_vel_in, sph_h_in, sph_col_in, sph_ts_in; fills sph_hsrc and
// sph_hmax as sph_hydro_run does (have_tts: sph_tg_ts holds the targets' timesteps, else all 0), orders the targets, walks once and writes sph_tg_res [nt][SPH_HY_NRES] in caller order: acc[3],
// dt_entropy before hydra.c:320, max_signal_vel.  own: the counts of bad own rows
int sph_hydro_sums_run(ngravs_ctx *c, const SphHydroParams &hp, long long nt, int have_tts, SphSumsStats *st, SphHydroStats *own);
// The owner's side of one round for one target (density.c:296-389 as k_sph_density applies it per lane): the final operations on
// the added sums s[SPH_NSUMS], the acceptance and bracketing rules, the next trial length, the clamp.  Returns 0: accepted, out6 =
// Hsml, Density, NumNgb, DivVel, CurlVel, DhsmlDensityFactor; 1: to be repeated with the new *h; 2: the same, and *rounds is past
// MAXITER (density.c:416).  No contraction: host and device give the same bits but for pow() in the bisection.
__host__ __device__ inline int sph_density_update_one(const double *s, double des, double dev, double minh, double *h_io, double *left_io,
                                                      double *right_io, int *rounds_io, double *out6)
{
#pragma clang fp contract(off)
  double h = *h_io, left = *left_io, right = *right_io;
  const int nr = ++*rounds_io;
  // final operations (density.c:296-303)
  const double numngb = s[SPH_SUM_NGB], rho = s[SPH_SUM_RHO];
  const double dhf = 1 / (1 + h * s[SPH_SUM_DHR] / (3 * rho));
  // enough neighbours? (density.c:314-389, rule for rule)
  bool redo = numngb < (des - dev) || (numngb > (des + dev) && h > 1.01 * minh);
  if(redo && left > 0 && right > 0 && (right - left) < 1.0e-3 * left)
    redo = false;
  if(!redo)
    {
      out6[SPH_HSML] = h;
      out6[SPH_DENSITY] = rho;
      out6[SPH_NUMNGB] = numngb;
      out6[SPH_DIVVEL] = s[SPH_SUM_DIV] / rho;
      out6[SPH_CURLVEL] = sqrt(s[SPH_SUM_ROTX] * s[SPH_SUM_ROTX] + s[SPH_SUM_ROTY] * s[SPH_SUM_ROTY] + s[SPH_SUM_ROTZ] * s[SPH_SUM_ROTZ]) / rho;
      out6[SPH_DHSML] = dhf;
      return 0;
    }
  if(numngb < (des - dev))
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
      const bool newton = fabs(numngb - des) < 0.5 * des;
      const double fac = 1 - (numngb - des) / (3 * numngb) * dhf;
      if(right == 0 && left > 0)
        h *= newton ? fac : 1.26;
      if(right > 0 && left == 0)
        h = newton ? h * fac : h / 1.26;
    }
  if(h < minh)
    h = minh;
  *h_io = h, *left_io = left, *right_io = right;
  return nr > SPH_MAXITER ? 2 : 1;
}
// one thread per target over device arrays; *failed counts the targets past MAXITER
int sph_density_update_device(long long n, const double *sums, double *h, double *left, double *right, int *rounds, double des, double dev,
                              double minh, int *accepted, double *const out[SPH_NRES], long long *failed);
// ---- kernels_pm.hip
int pm_run(ngravs_ctx *c);
int pm_deposit(ngravs_ctx *c);
int pm_finish(ngravs_ctx *c);
int pm_solve(ngravs_ctx *c);   // the first half of pm_finish: forward FFTs, Green multiply, inverse FFTs -> pm_phi complete
// += G / (pi BoxSize) x the CIC-weighted potential of the 8 corners of pm_phi, each row reading its species' mesh: for the own rows
// (tpos null: r_pot, Peano order) or for nt target records (tpos [nt][3], ttype) into out[nt]
int pm_potential_gather(ngravs_ctx *c, const double *tpos, const int *ttype, long long nt, double *out);
void pm_release(ngravs_ctx *c);
// GravPM from pm_phi (pm_mesh_valid) at the targets of gt_in / gt_type -> d_out [nt][3], G included
int pm_targets_run(ngravs_ctx *c, long long nt, double *d_out);
// ---- kernels_pmslab.hip
int pmslab_begin(ngravs_ctx *c, int rank, int world, int bbox[6]);
int pmslab_pack(ngravs_ctx *c, int stage, const int *all_bbox, int64_t *send_counts, int64_t *recv_counts, void **send, void **recv);
int pmslab_unpack(ngravs_ctx *c, int stage);
void pmslab_release(ngravs_ctx *c);
// ---- shortrange_table.cpp
void host_shortrange_table(const ngravs_config_t *cfg, double *force, double *pot, const ngravs_user_fn_t *fns = nullptr, int nfns = 0);
double cfg_asmth(const ngravs_config_t *c);
double cfg_rcut(const ngravs_config_t *c);

// ---- time integration (kernels_time.hip; the entry points of capi.hip check for NULL and forward) -------------------------------
int time_tables(const ngravs_time_params_t *par, int rule, double *drift, double *gravkick, double *hydrokick);
int time_factors(const ngravs_time_params_t *par, int ti0, int ti1, double out[3]);
int time_dt_displacement(const ngravs_time_params_t *par, const double sums[18], double G, double asmth, double time, double *out);
int time_next_sync_point(ngravs_ctx *c, const ngravs_time_cols_t *cols, int pm_ti_endstep, ngravs_sync_t *out);
int time_move_particles(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int time0, int time1, int wrap);
int time_displacement_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, double sums[18]);
int time_advance(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int ti_current, double dt_displacement,
                 int32_t *pm_ti, int64_t *n_kicked);
int time_global_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int ti_current, const int32_t *pm_ti,
                     const double *potential, int64_t potential_stride, double sums[NGRAVS_GLOBAL_NSUMS]);
int time_global_finish(const double sums[NGRAVS_GLOBAL_NSUMS], ngravs_sysstate_t *out);
int time_energy_line(const ngravs_sysstate_t *s, double time, char *buf, int64_t len);
// ---- snapshot files (kernels_snapshot.hip)
int snapshot_plan(ngravs_ctx *c, const ngravs_time_cols_t *cols, int64_t npart[6]);
int snapshot_block_count(ngravs_ctx *c, const ngravs_snapshot_t *snap, int block, int64_t *count, int32_t *bytes_per_element);
int snapshot_block(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, int block,
                   int64_t first, int64_t count, void *out, int out_on_device);
int snapshot_header(const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, const int64_t npart[6], const int64_t npart_total[6],
                    int num_files, double time, unsigned char out[256]);
int snapshot_write(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                   uint32_t blocks_mask, int snap_format, int64_t buffer_bytes, const char *path);
int snapshot_next_outputtime(const ngravs_time_params_t *par, const ngravs_output_rule_t *rule, int ti_curr, int32_t *ti_next);
