// capi.hip -- the C ABI of include/ngravs_hip.h: orchestration only, no arithmetic of the path.
//
// Mirrors the reference's drivers: gravity_tree (gravtree.c:27-460), long_range_force /
// pmforce_periodic (longrange.c:56, pm_periodic.c:204), domain_Decomposition (domain.c:62-154),
// compute_accelerations (accel.c:24-96), init_grav_maps (ngravs_core.c:201-425).
#include "engine.hpp"
#include "columns.hpp"
#include "../../include/ngravs_peano.h"
#include <chrono>
#include <cmath>

static thread_local std::string g_create_error;   // ngravs_last_error(NULL): why this thread's last ngravs_create[_with_laws] failed

void ngravs_report(ngravs_ctx *ctx, int code, const std::string &msg)
{
  if(ctx)
    ctx->last_error = msg;
  else
    g_create_error = msg;
  if(ctx && ctx->on_fatal)
    ctx->on_fatal(code, msg.c_str());
  else
    fprintf(stderr, "task %d: endrun called with an error level of %d (%s)\n", ctx ? ctx->cfg.rank : 0, code, msg.c_str());
}

// ---- small device helpers ---------------------------------------------------------------------
// GravCost of the walked particles -> the work-weight column (caller order); other rows keep theirs (gravtree.c:387-392 updates
// P[].GravCost of active particles only)
__global__ void k_cost_update(const unsigned int *__restrict__ idx, const unsigned char *__restrict__ act, const int *__restrict__ nint,
                              long long first, long long count, double *__restrict__ cost)
{
  long long k = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(k >= count)
    return;
  const long long i = first + k;
  if(act[i] & 1)
    cost[idx[i]] = (double)nint[i];
}
__global__ void k_key18(const unsigned long long *k21, long long n, long long *out)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    out[i] = (long long)(k21[i] >> (3 * (TREE_BITS - NGRAVS_BITS_PER_DIMENSION)));
}
__global__ void k_inverse_perm(const unsigned int *idx, long long n, int *inv)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    inv[idx[i]] = (int)i;
}
__global__ void k_map_idx(const int *inv, const int *in, long long n, int *out)
{
  long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i < n)
    out[i] = inv[in[i]];
}

// ---- lifecycle --------------------------------------------------------------------------------
extern "C" int ngravs_abi_version(void) { return NGRAVS_ABI_VERSION; }

extern "C" const char *ngravs_build_info(void)
{
  static char buf[512];
  snprintf(buf, sizeof(buf),
           "libngravs_hip abi=%d arch=gfx950 N_GRAVS<=%d NTAB=%d TREE_BITS=%d sizeof(config)=%zu sizeof(particles)=%zu "
           "sizeof(stats)=%zu walks=strict,group laws=none,newtonian,neg_newtonian,yukawa,coloyuk,bambam,sourcebambaryon,sourcebaryonbam",
           NGRAVS_ABI_VERSION, NGRAVS_MAX_GRAVS, NGRAVS_NTAB, NGRAVS_TREE_BITS, sizeof(ngravs_config_t),
           sizeof(ngravs_particles_t), sizeof(ngravs_stats_t));
  return buf;
}

extern "C" void ngravs_config_default(ngravs_config_t *cfg)
{
  memset(cfg, 0, sizeof(*cfg));
  cfg->abi_version = NGRAVS_ABI_VERSION;
  cfg->n_gravs = 1;
  cfg->G = 1.0;
  cfg->err_tol_theta = 0.5;
  cfg->err_tol_force_acc = 0.005;
  cfg->yukawa_imass = 60.0;
  cfg->tree_alloc_factor = 0.8;
  cfg->world_size = 1;
  for(int i = 0; i < NGRAVS_MAX_GRAVS; i++)
    for(int j = 0; j < NGRAVS_MAX_GRAVS; j++)
      {
        cfg->law_accel[i][j] = cfg->law_greens[i][j] = cfg->law_normed[i][j] = NGRAVS_LAW_NEWTON;
        cfg->law_spline[i][j] = NGRAVS_SPLINE_PLUMMER;
      }
}

// the sanity checks of init_grav_maps (ngravs_core.c:235-261, 321-424)
static int check_config(const ngravs_config_t *cfg, std::string &why)
{
  if(cfg->abi_version != NGRAVS_ABI_VERSION)
    {
      why = "abi_version mismatch";
      return NGRAVS_ERR_ARG;
    }
  if(cfg->n_gravs < 1 || cfg->n_gravs > NGRAVS_MAX_GRAVS)
    {
      why = "n_gravs out of range";
      return NGRAVS_ERR_ARG;
    }
  if(cfg->pmgrid < 0 || (cfg->pmgrid & 1))
    {
      // odd PMGRID: the reference pads to PMGRID2 = 2*(PMGRID/2+1) = N+1; a mesh of [N][N][N+2] would be transformed wrongly
      why = "PMGRID must be 0 (no mesh) or positive and even: the in-place real-to-complex mesh is laid out [N][N][N+2], which is the "
            "padding of the transform only for even N";
      return NGRAVS_ERR_ARG;
    }
  if(cfg->pmgrid && !cfg->periodic)
    {
      why = "non-periodic PM is disabled by ngravs itself (ngravs_core.c:235-242)";
      return NGRAVS_ERR_ARG;
    }
  if((cfg->periodic || cfg->pmgrid) && !(cfg->box_size > 0))
    {
      why = "box_size must be > 0";
      return NGRAVS_ERR_ARG;
    }
  if(cfg->pmgrid && cfg->type_to_grav[0] != 0)
    {
      why = "gas must be gravitational species 0 with PMGRID (ngravs_core.c:255-261)";
      return NGRAVS_ERR_WIRING;
    }
  if(cfg->world_size < 1 || cfg->rank < 0 || cfg->rank >= cfg->world_size)
    {
      why = "rank/world_size";
      return NGRAVS_ERR_ARG;
    }
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    if(cfg->type_to_grav[t] < 0 || cfg->type_to_grav[t] >= cfg->n_gravs)
      {
        why = "TypeToGrav entry outside [0,N_GRAVS)";
        return NGRAVS_ERR_WIRING;
      }
  for(int i = 0; i < cfg->n_gravs; i++)
    for(int j = 0; j < cfg->n_gravs; j++)
      {
        // (user ids, NGRAVS_LAW_USER0 + k, are checked by user_check_config against the registry)
        auto bad = [](int id, int count) { return id < 0 || (id >= count && id < NGRAVS_LAW_USER0); };
        if(bad(cfg->law_accel[i][j], NGRAVS_LAW_COUNT) || bad(cfg->law_spline[i][j], NGRAVS_SPLINE_COUNT) ||
           bad(cfg->law_greens[i][j], NGRAVS_LAW_COUNT) || bad(cfg->law_normed[i][j], NGRAVS_LAW_COUNT))
          {
            why = "force-law table slot not wired (ngravs_core.c:321-360)";
            return NGRAVS_ERR_WIRING;
          }
        // Newton's third law probe F[i][j](1,1,0.5,3,1) == F[j][i](...) (ngravs_core.c:371-403): equal ids, or the two views of
        // the BAM-baryon pair (sourcebambaryon / sourcebaryonbam agree for unit masses and N = 1)
        // (a pair with a user id is probed through its callbacks by user_check_config)
        auto same = [](int a, int b, int p, int q) {
          return a == b || (a == p && b == q) || (a == q && b == p) || a >= NGRAVS_LAW_USER0 || b >= NGRAVS_LAW_USER0;
        };
        if(!same(cfg->law_accel[i][j], cfg->law_accel[j][i], NGRAVS_LAW_SOURCEBAM, NGRAVS_LAW_TARGETBAM) ||
           !same(cfg->law_spline[i][j], cfg->law_spline[j][i], NGRAVS_SPLINE_SOURCEBAM, NGRAVS_SPLINE_TARGETBAM) ||
           !same(cfg->law_normed[i][j], cfg->law_normed[j][i], -1, -1) || !same(cfg->law_greens[i][j], cfg->law_greens[j][i], -1, -1))
          {
            why = "force-law table violates Newton's third law (ngravs_core.c:371-403)";
            return NGRAVS_ERR_WIRING;
          }
      }
  if(cfg_has_bam(*cfg) && (cfg->pmgrid || cfg->periodic))
    {
      why = "the BAM laws have no Green's functions: tree-only, non-periodic runs (ngravs.c:189-194)";
      return NGRAVS_ERR_WIRING;
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_create(const ngravs_config_t *cfg, ngravs_ctx **out) { return ngravs_create_with_laws(cfg, nullptr, 0, out); }

extern "C" int ngravs_create_with_laws(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, ngravs_ctx **out)
{
  return ngravs_create_with_lattice(cfg, fns, nfns, nullptr, 0, out);
}

extern "C" int ngravs_create_with_lattice(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns,
                                          const ngravs_user_lattice_t *lat, int nlat, ngravs_ctx **out)
{
  return ngravs_create_with_potentials(cfg, fns, nfns, lat, nlat, nullptr, 0, out);
}

extern "C" int ngravs_create_with_potentials(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns,
                                             const ngravs_user_lattice_t *lat, int nlat, const ngravs_user_potential_t *pots, int npot,
                                             ngravs_ctx **out)
{
  if(!cfg || !out)
    return NGRAVS_ERR_ARG;
  *out = nullptr;
  std::string why;
  int rc = check_config(cfg, why);
  if(rc == NGRAVS_OK)
    rc = user_check_config(cfg, fns, nfns, lat, nlat, why);
  if(rc == NGRAVS_OK)
    rc = user_check_potentials(cfg, pots, npot, why);
  if(rc != NGRAVS_OK)
    {
      ngravs_report(nullptr, rc, why);
      return rc;
    }
  int ndev = 0;
  if(hipGetDeviceCount(&ndev) != hipSuccess || ndev <= 0)
    {
      ngravs_report(nullptr, NGRAVS_ERR_NO_DEVICE, "no HIP device: libngravs_hip has no CPU fallback");
      return NGRAVS_ERR_NO_DEVICE;
    }
  if(cfg->device < 0 || cfg->device >= ndev)
    return NGRAVS_ERR_ARG;
  ngravs_ctx *c = new ngravs_ctx;
  c->cfg = *cfg;
  c->user_fns.assign(fns, fns + nfns);
  c->user_lat.assign(lat, lat + nlat);
  c->user_pot.assign(pots, pots + npot);
  user_pot_registry(c);
  memset(&c->stats, 0, sizeof(c->stats));
  if(hipSetDevice(cfg->device) != hipSuccess || c->own_stream.create() != hipSuccess ||
     c->ev0.create() != hipSuccess || c->ev1.create() != hipSuccess ||
     c->evk0.create() != hipSuccess || c->evk1.create() != hipSuccess || c->ev_fork.create() != hipSuccess ||
     c->ev_pm0.create() != hipSuccess || c->ev_pm1.create() != hipSuccess || c->ev_walk.create() != hipSuccess)
    {
      delete c;
      return NGRAVS_ERR_NO_DEVICE;
    }
  c->stream = c->own_stream;
  if(cfg->pmgrid)
    {
      c->asmth = cfg_asmth(cfg);
      c->rcut = cfg_rcut(cfg);
    }
  *out = c;
  return NGRAVS_OK;
}

extern "C" void ngravs_destroy(ngravs_ctx *c)
{
  if(!c)
    return;
  (void)hipSetDevice(c->cfg.device);
  (void)hipStreamSynchronize(c->stream);
  if(c->pm_stream)
    {
      (void)hipStreamSynchronize(c->pm_stream);
      (void)hipStreamSynchronize(c->walk_stream);
    }
  pm_release(c);       // the FFT plans: boxed handles, not owners
  pmslab_release(c);
  delete c;            // buffers and events, then the streams (declaration order in ngravs_ctx)
}

extern "C" void ngravs_set_fatal_handler(ngravs_ctx *ctx, ngravs_fatal_fn fn)
{
  if(ctx)
    ctx->on_fatal = fn;
}

extern "C" int ngravs_set_opening(ngravs_ctx *c, double theta, double errtol)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  c->cfg.err_tol_theta = theta;
  c->cfg.err_tol_force_acc = errtol;
  return NGRAVS_OK;
}

// set_softenings() (gravtree.c:468-518) recomputes All.ForceSoftening[] from the scale factor at the top of every gravity_tree()
// of a comoving run (gravtree.c:50-51).  The walk, the direct sum and the import decision read the new lengths from the next
// call on; the max-softening-type flags of the nodes are those of the last tree build or refit, as in the reference
// (force_update_node_recursive, forcetree.c:704-713, runs at build time only).
extern "C" int ngravs_set_softening(ngravs_ctx *c, const double force_softening[NGRAVS_NTYPES])
{
  if(!c || !force_softening)
    return NGRAVS_ERR_ARG;
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    if(!(force_softening[t] >= 0.0))
      {
        ngravs_report(c, NGRAVS_ERR_ARG, "ngravs_set_softening: negative or NaN softening length");
        return NGRAVS_ERR_ARG;
      }
  for(int t = 0; t < NGRAVS_NTYPES; t++)
    c->cfg.force_softening[t] = force_softening[t];
  c->gsoft_col_stale = c->gsoft_node_stale = true;   // adaptive softening: the other types' lengths enter both columns
  return NGRAVS_OK;
}

extern "C" int ngravs_set_walk_mode(ngravs_ctx *c, int mode)
{
  if(!c || (mode != NGRAVS_WALK_STRICT && mode != NGRAVS_WALK_GROUP))
    return NGRAVS_ERR_ARG;
  c->cfg.walk_mode = mode;
  return NGRAVS_OK;
}

extern "C" int ngravs_get_config(ngravs_ctx *c, ngravs_config_t *out)
{
  if(!c || !out)
    return NGRAVS_ERR_ARG;
  *out = c->cfg;
  if(c->cfg.pmgrid)
    {
      out->asmth = c->asmth;
      out->rcut = c->rcut;
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_set_tuning(ngravs_ctx *c, const char *name, double v)
{
  if(!c || !name)
    return NGRAVS_ERR_ARG;
  const std::string k(name);
  const long long iv = (long long)v;
  Tuning &t = c->tune;
  if(k == "walk_fused")
    t.walk_fused = iv != 0;
  else if(k == "walk_batch" && iv >= 0)
    t.walk_batch = iv;
  else if(k == "walk_waves" && iv >= 0 && iv <= 16)
    t.walk_waves = (int)iv;
  else if(k == "walk_lcap" && (iv == 0 || (iv >= 1024 && iv <= 65536)))
    {
      t.walk_lcap = (int)iv;
      c->walk_lcap = 0;   // re-initialised by the next split walk
    }
  else if(k == "walk_root")
    t.walk_root = iv != 0;
  else if(k == "walk_compact")
    t.walk_compact = iv != 0;
  else if(k == "walk_spread" && iv >= 0 && iv <= 64 && (iv & (iv - 1)) == 0)
    t.walk_spread = (int)iv;
  else if(k == "walk_sg" && iv >= 0 && iv <= 16)
    t.walk_sg = (int)iv;
  else if(k == "walk_ring" && iv >= 0 && iv <= 1)
    t.walk_ring = (int)iv;
  else if(k == "walk_head" && iv >= 0 && iv <= 1)
    t.walk_head = (int)iv;
  else if(k == "walk_ring_k" && iv >= 0 && iv <= 8)
    t.walk_ring_k = (int)iv;
  else if(k == "walk_nleaf" && iv >= -1 && iv <= 8)
    t.walk_nleaf = (int)iv;
  else if(k == "walk_exact_reach")
    t.walk_exact_reach = iv != 0;
  else if(k == "sort_full")
    t.sort_full = iv != 0;
  else if(k == "tree_levelwise")
    t.tree_levelwise = iv != 0;
  else if(k == "dd_keep" && v >= 0 && v <= 0.25)
    t.dd_keep = v;
  else if(k == "pm_cus" && (iv == -1 || (iv >= 0 && iv <= 32 && iv % 8 == 0)))   // multiples of 8: the same share of every XCD
    t.pm_cus = (int)iv;
  else if(k == "walk_tg_sort")
    t.walk_tg_sort = iv != 0;
  else if(k == "sph_verbose")
    t.sph_verbose = iv != 0;
  else
    {
      ngravs_report(c, NGRAVS_ERR_ARG, "ngravs_set_tuning: unknown name or value out of range: " + k);
      return NGRAVS_ERR_ARG;
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_memcpy(ngravs_ctx *c, void *dst, const void *src, int64_t bytes, int kind)
{
  if(!c || bytes < 0 || kind < 1 || kind > 3 || (bytes > 0 && (!dst || !src)))
    return NGRAVS_ERR_ARG;
  if(bytes == 0)
    return NGRAVS_OK;
  (void)hipSetDevice(c->cfg.device);
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  HIP_TRY(c, hipMemcpy(dst, src, (size_t)bytes, kind == 1 ? hipMemcpyHostToDevice : (kind == 2 ? hipMemcpyDeviceToHost : hipMemcpyDeviceToDevice)));
  return NGRAVS_OK;
}

extern "C" int ngravs_device_alloc(ngravs_ctx *c, void **ptr, int64_t bytes)
{
  if(!c || !ptr || bytes < 0)
    return NGRAVS_ERR_ARG;
  *ptr = nullptr;
  (void)hipSetDevice(c->cfg.device);
  if(hipMalloc(ptr, (size_t)(bytes > 0 ? bytes : 1)) != hipSuccess)
    return NGRAVS_ERR_NOMEM;
  return NGRAVS_OK;
}

extern "C" int ngravs_device_free(ngravs_ctx *c, void *ptr)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  if(ptr)
    (void)hipFree(ptr);
  return NGRAVS_OK;
}

// ---- data hand-over -----------------------------------------------------------------------------
static double ev_ms(ngravs_ctx *c);

// the state after a hand-over: what every one resets, and what only a new particle set (not a kept tree's update) resets
static void handed_over(ngravs_ctx *c, bool keep_tree)
{
  c->walk_ia_ratio = 0;   // (a new particle set: the walk's unit is chosen afresh)
  c->pm_solo_steps = 0, c->pm_auto_cus = -1;   // ... and so are the CUs reserved for PM
  c->walk_unit_state = 4;
  c->have_particles = true;
  c->pot_mesh_valid = false;   // the mesh of the last ngravs_compute_potential belongs to the positions of that call
  if(keep_tree)
    {
      c->tree_stale = true;    // same order and topology; columns and moments are refreshed by ngravs_force_update_tree
      return;
    }
  c->have_order = c->have_tree = c->have_pm = c->have_acc = false;   // new P[]: nothing carries over ...
  c->gsoft_on = false;     // ... a new set has no gas softening lengths
  c->top.on = false;   // (the top tree itself is kept: it is the first guess of the next decomposition)
  c->pm_parked = false;
}

static int set_particles_impl(ngravs_ctx *c, const ngravs_particles_t *p, bool keep_tree)
{
  if(!c || !p || p->n < 0 || (p->n > 0 && (!p->pos || !p->mass || !p->type)))
    return NGRAVS_ERR_ARG;
  if(p->n == 0 && keep_tree)
    {
      // a task without own particles on a kept step of several tasks: its working set is imported copies (or nothing)
      if(!c->have_particles || c->n_local != 0)
        return NGRAVS_ERR_STATE;
      c->tree_stale = c->have_tree;
      return NGRAVS_OK;
    }
  if(p->n == 0)
    {
      // a task without particles (NumPart = 0): legal with several tasks -- it still owns mesh slabs, takes part in every
      // collective and may receive particles in the next migration.  Nothing to upload.
      (void)hipSetDevice(c->cfg.device);
      c->n = c->n_local = 0;
      c->own_order_nlocal = -1;
      c->sort_low = 35;
      c->all_active = true;
      handed_over(c, false);
      return NGRAVS_OK;
    }
  // (a multi-task working set: the caller's rows are its own particles; the imported copies behind them are refreshed by their
  // owners, ngravs_host_kept_step)
  const bool keep_halo = keep_tree && c->n_local != c->n;
  if(keep_tree && (!c->have_order || !c->have_tree || p->n != c->n_local))
    {
      ngravs_report(c, NGRAVS_ERR_STATE, "ngravs_update_particles: needs a built tree over the same own particles");
      return NGRAVS_ERR_STATE;
    }
  if(p->n >= (1ll << 31) - 64)
    {
      ngravs_report(c, NGRAVS_ERR_ARG, "int particle indices (reference All.MaxPart is int): n must be < 2^31");
      return NGRAVS_ERR_ARG;
    }
  (void)hipSetDevice(c->cfg.device);
  const int64_t n = p->n;
  if(c->in_pos.ensure(3 * n) || c->in_mass.ensure(n) || c->in_oldacc.ensure(n) || c->in_type.ensure(n) || c->in_active.ensure(n) ||
     (!keep_tree && c->in_cost.ensure(n)))
    {
      ngravs_report(c, NGRAVS_ERR_NOMEM, "device allocation failed");
      return NGRAVS_ERR_NOMEM;
    }
  if(!keep_halo)
    c->n = n;
  c->n_local = n;
  if(!keep_tree)
    {
      // The Peano order of the last decomposition (s_idx) is only a visiting order for the per-leaf sums -- any permutation is
      // correct, a good one lets a wave add up before it touches memory.  A host that hands the same rows over again with
      // drifted positions (P[] between two migrations) keeps it; a different row count means other rows.
      if(c->own_order_nlocal != n)
        c->own_order_nlocal = -1;
      c->sort_low = 35;
    }
  int rc;
  if(!keep_tree && (rc = dd_fill_ids(c)))
    return rc;
  if((rc = col_upload(c, p->pos, p->pos_stride, sizeof(double), 3, n, p->on_device, c->in_pos.p)))
    return rc;
  if((rc = col_upload(c, p->mass, p->mass_stride, sizeof(double), 1, n, p->on_device, c->in_mass.p)))
    return rc;
  if(p->old_acc)
    {
      if((rc = col_upload(c, p->old_acc, p->old_acc_stride, sizeof(double), 1, n, p->on_device, c->in_oldacc.p)))
        return rc;
    }
  else
    hipLaunchKernelGGL(k_fill_f64, GRID1(n), 0, c->stream, c->in_oldacc.p, (long long)n, 0.0);
  if(!keep_tree)
    {
      if(p->grav_cost && p->on_device)
        hipLaunchKernelGGL(k_pack_strided_f32_to_f64, GRID1(n), 0, c->stream, (const unsigned char *)p->grav_cost,
                           (long long)p->grav_cost_stride, (long long)n, c->in_cost.p);
      else if(p->grav_cost)
        {
          // the floats at the front of the staging buffer, their doubles behind them
          const size_t at = (sizeof(float) * (size_t)n + 7) & ~(size_t)7;
          unsigned char *st = col_stage_rows(c, p->grav_cost, p->grav_cost_stride, sizeof(float), n, at + sizeof(double) * (size_t)n);
          const float *f = reinterpret_cast<const float *>(st);
          double *h = reinterpret_cast<double *>(st + at);
          for(int64_t i = 0; i < n; i++)
            h[i] = f[i];
          if((rc = col_upload(c, h, sizeof(double), sizeof(double), 1, n, 0, c->in_cost.p)))
            return rc;
        }
      else
        hipLaunchKernelGGL(k_fill_f64, GRID1(n), 0, c->stream, c->in_cost.p, (long long)n, 0.0);
    }
  // Type (int32)
  if(p->on_device)
    {
      if(c->d_counters.ensure(16))
        return NGRAVS_ERR_NOMEM;
      int nbad = 0;
      HIP_TRY(c, hipMemsetAsync(c->d_counters.p + 15, 0, sizeof(int), c->stream));
      hipLaunchKernelGGL(k_pack_type, GRID1(n), 0, c->stream, (const unsigned char *)p->type, (long long)p->type_stride,
                         (long long)n, c->in_type.p, c->d_counters.p + 15);
      HIP_TRY(c, hipMemcpyAsync(&nbad, c->d_counters.p + 15, sizeof(int), hipMemcpyDeviceToHost, c->stream));
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      if(nbad)
        {
          ngravs_report(c, NGRAVS_ERR_ARG, "particle Type outside 0..5");
          return NGRAVS_ERR_ARG;
        }
    }
  else
    {
      const int *h = reinterpret_cast<const int *>(col_stage_rows(c, p->type, p->type_stride, sizeof(int), n, sizeof(int) * (size_t)n));
      for(int64_t i = 0; i < n; i++)
        if(h[i] < 0 || h[i] >= NGRAVS_NTYPES)
          {
            ngravs_report(c, NGRAVS_ERR_ARG, "particle Type outside 0..5");
            return NGRAVS_ERR_ARG;
          }
      if((rc = col_upload(c, h, sizeof(int), sizeof(int), 1, n, 0, c->in_type.p)))
        return rc;
    }
  c->all_active = p->active == nullptr;
  if(p->active)
    {
      if(p->on_device)
        hipLaunchKernelGGL(k_pack_active, GRID1(n), 0, c->stream, (const unsigned char *)p->active,
                           (long long)p->active_stride, (long long)n, c->in_active.p);
      else
        {
          unsigned char *h = col_stage_rows(c, p->active, p->active_stride, 1, n, (size_t)n);
          for(int64_t i = 0; i < n; i++)
            h[i] = h[i] ? 1 : 0;
          if((rc = col_upload(c, h, 1, 1, 1, n, 0, c->in_active.p)))
            return rc;
        }
    }
  else
    hipLaunchKernelGGL(k_fill_u8, GRID1(n), 0, c->stream, c->in_active.p, (long long)n, (unsigned char)1);
  HIP_TRY(c, hipGetLastError());
  handed_over(c, keep_tree);
  if(!keep_tree && p->grav_pm && c->cfg.pmgrid)
    {
      // nothing carries over except P[].GravPM, which the host keeps between PM steps: parked in caller order, permuted into the
      // Peano order by the next ngravs_domain_decomposition (OldAcc on non-PM steps needs it, gravtree.c:318-330)
      if(c->pm_orig.ensure(3 * n))
        return NGRAVS_ERR_NOMEM;
      if((rc = col_upload(c, p->grav_pm, p->grav_pm_stride, sizeof(double), 3, n, p->on_device, c->pm_orig.p)))
        return rc;
      c->pm_parked = true;
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_set_particles(ngravs_ctx *c, const ngravs_particles_t *p) { return set_particles_impl(c, p, false); }

extern "C" int ngravs_update_particles(ngravs_ctx *c, const ngravs_particles_t *p) { return set_particles_impl(c, p, true); }

// the drifted tree of predict.c:79-91 + force_update_len(): same decomposition and topology, fresh columns, recomputed
// moments and grown cell sides
extern "C" int ngravs_force_update_tree(ngravs_ctx *c)
{
  if(!c || !c->have_order || !c->have_tree)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(c->n == 0)   // an empty working set (a task without particles): no nodes to refit
    {
      c->tree_stale = false;
      return NGRAVS_OK;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  int rc = dom_regather(c);
  if(rc)
    return rc;
  if((rc = tree_moments(c, true)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->stats.t_treebuild = ev_ms(c) * 1e-3;
  c->stats.t_domain = c->stats.t_peano = 0;
  c->tree_stale = false;
  c->tree_refit = true;
  c->gsoft_node_stale = true;
  return NGRAVS_OK;
}

extern "C" int ngravs_set_old_acc(ngravs_ctx *c, const double *old_acc, int64_t stride, int on_device)
{
  if(!c || !c->have_particles || !old_acc)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  if(c->n_local == 0)
    return NGRAVS_OK;
  // the caller's rows are its OWN particles (NumPart = ngravs_dd_num_local()); imported copies of a multi-task working set are
  // sources only, their OldAcc is never read
  int rc = col_upload(c, old_acc, stride, sizeof(double), 1, c->n_local, on_device, c->in_oldacc.p);
  if(rc)
    return rc;
  if(c->have_order)
    hipLaunchKernelGGL(k_permute_f64, GRID1(c->n), 0, c->stream, c->s_idx.p, (long long)c->n, 1, c->in_oldacc.p, c->s_oldacc.p);
  HIP_TRY(c, hipGetLastError());
  return NGRAVS_OK;
}

// the staged column checked in place: type-0 rows whose length is negative or not finite are counted; rows of other types become 0
__global__ void k_gsoft_stage(const int *__restrict__ type, long long n, double *__restrict__ col, int *__restrict__ nbad)
{
  const long long i = blockIdx.x * (long long)blockDim.x + threadIdx.x;
  if(i >= n)
    return;
  double h = 0.0;
  if(type[i] == 0)
    {
      h = col[i];
      if(!(h >= 0.0) || isinf(h))
        atomicAdd(nbad, 1);
    }
  col[i] = h;
}

// ADAPTIVE_GRAVSOFT_FORGAS (forcetree.c:1398-1413): the caller-order copy of the gas lengths; the sorted column and the node
// column are derived from it when a walk or a direct sum needs them (adaptive_refresh)
extern "C" int ngravs_set_gas_softening(ngravs_ctx *c, const double *hsml, int64_t stride, int on_device)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  if(!hsml)
    {
      c->gsoft_on = false;
      return NGRAVS_OK;
    }
  if(!c->have_particles || c->n_local <= 0)
    {
      ngravs_report(c, NGRAVS_ERR_ARG, "ngravs_set_gas_softening: no particles handed over yet");
      return NGRAVS_ERR_ARG;
    }
  if(c->cfg.world_size > 1 || c->n_local != c->n || c->top.on)
    {
      ngravs_report(c, NGRAVS_ERR_STATE, "ngravs_set_gas_softening: single task only (imported copies and top-leaf sums carry no "
                                         "softening length)");
      return NGRAVS_ERR_STATE;
    }
  if(cfg_has_user(c->cfg))
    {
      ngravs_report(c, NGRAVS_ERR_ARG, "ngravs_set_gas_softening: not with user-defined laws (their spline tables are sampled per "
                                       "softening length)");
      return NGRAVS_ERR_ARG;
    }
  (void)hipSetDevice(c->cfg.device);
  const int64_t n = c->n_local;
  DevBuf<double> &stage = c->gsoft_stage;   // checked here, swapped in when the call succeeds: a refused call changes nothing
  if(stage.ensure(n) || c->d_counters.ensure(16))
    return NGRAVS_ERR_NOMEM;
  // the whole column is staged (only type-0 rows would have to be read) and checked on the device against the types there
  int nbad = 0, rc = NGRAVS_OK;
  if((rc = col_upload(c, hsml, stride, sizeof(double), 1, n, on_device, stage.p)))
    return rc;
  if(hipMemsetAsync(c->d_counters.p + 15, 0, sizeof(int), c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  hipLaunchKernelGGL(k_gsoft_stage, GRID1(n), 0, c->stream, c->in_type.p, (long long)n, stage.p, c->d_counters.p + 15);
  if(!rc && (hipMemcpyAsync(&nbad, c->d_counters.p + 15, sizeof(int), hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
             hipStreamSynchronize(c->stream) != hipSuccess || hipGetLastError() != hipSuccess))
    rc = NGRAVS_ERR_NO_DEVICE;
  if(!rc && nbad)
    {
      ngravs_report(c, NGRAVS_ERR_ARG, "ngravs_set_gas_softening: " + std::to_string(nbad) + " type-0 rows with a negative or non-finite length");
      rc = NGRAVS_ERR_ARG;
    }
  if(rc)
    return rc;
  std::swap(c->in_gsoft, c->gsoft_stage);
  c->gsoft_on = true;
  c->gsoft_col_stale = c->gsoft_node_stale = true;
  return NGRAVS_OK;
}

// ---- the path -------------------------------------------------------------------------------------
static double ev_ms(ngravs_ctx *c)
{
  float ms = 0;
  (void)hipEventSynchronize(c->ev1);
  (void)hipEventElapsedTime(&ms, c->ev0, c->ev1);
  return ms;
}

// P[].GravPM survives between PM steps (it is only rewritten by pmforce_periodic): park the OWN rows of r_pm (Peano order of the
// last decomposition) in caller order before the rows are re-sorted, migrated or joined by new imports.  pm_orig then is a
// caller-order column like in_mass: the migration moves it with the particles (kernels_domain.hip).
static int park_grav_pm(ngravs_ctx *c)
{
  if(!c->have_pm || !c->have_order)
    return NGRAVS_OK;
  if(c->pm_orig.ensure(3 * (c->n_local > 0 ? c->n_local : 1)))
    return NGRAVS_ERR_NOMEM;
  hipLaunchKernelGGL(k_unpermute_f64_lim, GRID1(c->n), 0, c->stream, c->s_idx.p, (long long)c->n, (long long)c->n_local, 3, c->r_pm.p,
                     c->pm_orig.p);
  c->pm_parked = true;
  c->have_pm = false;
  return NGRAVS_OK;
}

static int domain_decomposition_impl(ngravs_ctx *c, bool keep_pm)
{
  if(!c || !c->have_particles)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(keep_pm)
    {
      if(int rc = park_grav_pm(c))   // unless this step recomputes GravPM anyway
        return rc;
    }
  else
    c->pm_parked = false;
  // parked GravPM (own rows; handed over with the particles, ngravs_particles_t.grav_pm, or parked above / by
  // ngravs_dd_local_extent): permuted into the new order below; imported copies carry none and are never read (k_finish
  // visits active own rows only)
  c->have_pm = c->pm_parked;
  c->pm_parked = false;
  if(c->n == 0)
    {
      // a task without particles and without imported copies: an empty order
      c->own_order_nlocal = -1;
      c->shard_first = c->shard_count = 0;
      c->have_order = true;
      c->have_tree = c->tree_stale = c->have_pm = false;
      c->stats.t_domain = c->stats.t_peano = 0;
      return NGRAVS_OK;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  int rc = dom_find_extent(c);
  if(rc)
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->stats.t_domain = ev_ms(c) * 1e-3;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  c->own_order_nlocal = -1;
  rc = dom_keys_and_sort(c);
  if(rc)
    return rc;
  c->own_order_nlocal = c->n_local;   // the per-cell sums of the next multi-task decomposition visit the own rows in this order
  c->own_order_len = c->n;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->stats.t_peano = ev_ms(c) * 1e-3;
  // target shard of this rank: a contiguous segment of the Peano order (domain.c:347-456 cuts the
  // curve into NTask segments; here by particle count)
  int64_t ws = c->cfg.world_size, r = c->cfg.rank;
  int64_t lo = (c->n * r) / ws, hi = (c->n * (r + 1)) / ws;
  lo = (lo / 64) * 64;                       // wave-aligned cuts keep groups identical across world sizes
  hi = (r + 1 == ws) ? c->n : (hi / 64) * 64;
  c->shard_first = lo;
  c->shard_count = hi - lo;
  c->have_order = true;
  c->have_tree = false;   // TreeReconstructFlag = 1 (domain.c:84)
  c->gsoft_col_stale = c->gsoft_node_stale = true;
  c->tree_stale = false;
  if(c->have_pm)
    {
      if(c->r_pm.ensure(3 * c->n))
        return NGRAVS_ERR_NOMEM;
      hipLaunchKernelGGL(k_permute_f64_lim, GRID1(c->n), 0, c->stream, c->s_idx.p, (long long)c->n, (long long)c->n_local, 3, c->pm_orig.p,
                         c->r_pm.p);
      HIP_TRY(c, hipGetLastError());
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_domain_decomposition(ngravs_ctx *c) { return domain_decomposition_impl(c, true); }

// The step that follows recomputes GravPM (a PM step: long_range_force() comes before gravity_tree(), accel.c:34-46): the stored
// long-range force need not be parked in caller order, migrated and permuted into the new Peano order only to be overwritten
extern "C" int ngravs_discard_grav_pm(ngravs_ctx *c)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  c->have_pm = false;
  c->pm_parked = false;
  return NGRAVS_OK;
}

extern "C" int64_t ngravs_force_treebuild(ngravs_ctx *c)
{
  if(!c || !c->have_order)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(c->n == 0)   // nothing to build a tree of (a task without particles): no nodes, nothing will walk it
    {
      c->nnodes = 0;
      c->have_tree = true;
      c->tree_refit = false;
      c->stats.t_treebuild = 0;
      return 0;
    }
  if(hipEventRecord(c->ev0, c->stream) != hipSuccess)
    return NGRAVS_ERR_NO_DEVICE;
  int rc = tree_build(c);
  if(rc)
    return rc;
  if(hipEventRecord(c->ev1, c->stream) != hipSuccess)
    return NGRAVS_ERR_NO_DEVICE;
  c->stats.t_treebuild = ev_ms(c) * 1e-3;
  c->have_tree = true;
  c->tree_refit = false;
  c->gsoft_node_stale = true;
  return c->nnodes;
}

static int ensure_table(ngravs_ctx *c)
{
  if(!c->cfg.pmgrid || c->table_ready)
    return NGRAVS_OK;
  const int ng = c->cfg.n_gravs;
  std::vector<double> h((size_t)(ng * ng + 1) * NTAB);
  host_shortrange_table(&c->cfg, h.data(), nullptr, c->user_fns.data(), (int)c->user_fns.size());
  {
    // bin-wise Yukawa factor E[tab] = exp(-ym tab/asmthfac) behind the tables (kernels_walk.hip, WalkParams::exp_tab)
    WalkParams wp;
    make_walk_params(c, &wp);
    for(int t = 0; t < NTAB; t++)
      h[(size_t)ng * ng * NTAB + t] = exp(-wp.ym * (double)t * wp.inv_asmthfac);
  }
  if(c->table.ensure(h.size()))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipMemcpyAsync(c->table.p, h.data(), sizeof(double) * h.size(), hipMemcpyHostToDevice, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->table_ready = true;
  return NGRAVS_OK;
}

// PM beside the walk: whole CUs are split between two masked streams.  R = 8 m reserved CUs (m = 1..4) are m CUs of every XCD: mask
// bits 33 x + 8 j (x = 0..7, j < m) lie on XCD x whether the runtime deals the bits to the 8 XCDs round robin (bit % 8) or in blocks
// of 32 (bit / 32); tests/test_gpu_overlap.py checks with ngravs_cu_probe where the two streams' workgroups land.
static bool pm_cu_bit(int R, int b)
{
  const int x = b / 32, k = b - 33 * x;
  return b < 256 && k >= 0 && k % 8 == 0 && k / 8 < R / 8;
}

// the two masked streams for R reserved CUs (created on first use, recreated when R changes); an error leaves the serial path
static int masked_streams(ngravs_ctx *c, int R)
{
  if(c->pm_stream && c->pm_stream_cus == R)
    return NGRAVS_OK;
  if(!c->device_cus)
    {
      hipDeviceProp_t prop;
      HIP_TRY(c, hipGetDeviceProperties(&prop, c->cfg.device));
      c->device_cus = prop.multiProcessorCount;
    }
  if(c->device_cus != 256 || R < 8 || R > 32 || R % 8)   // (the mask layout above is that of 8 XCDs of 32 CUs)
    return NGRAVS_ERR_ARG;
  if(c->pm_stream)
    {
      HIP_TRY(c, hipStreamSynchronize(c->pm_stream));
      HIP_TRY(c, hipStreamSynchronize(c->walk_stream));
      c->pm_stream.adopt(nullptr);
      c->walk_stream.adopt(nullptr);
      c->pm_stream_cus = 0;
    }
  uint32_t mp[8] = {0}, mw[8] = {0};
  for(int b = 0; b < 256; b++)
    (pm_cu_bit(R, b) ? mp : mw)[b / 32] |= 1u << (b % 32);
  // local owners: the context gets the pair only when both exist and carry the masks asked for
  DevStream sp, sw;
  hipStream_t h = nullptr;
  if(hipExtStreamCreateWithCUMask(&h, 8, mp) == hipSuccess)
    sp.adopt(h);
  if(sp && hipExtStreamCreateWithCUMask(&h, 8, mw) == hipSuccess)
    sw.adopt(h);
  uint32_t gp[8] = {0}, gw[8] = {0};
  if(!sp || !sw || hipExtStreamGetCUMask(sp, 8, gp) != hipSuccess || hipExtStreamGetCUMask(sw, 8, gw) != hipSuccess ||
     memcmp(gp, mp, sizeof mp) || memcmp(gw, mw, sizeof mw))
    {
      (void)hipGetLastError();
      return NGRAVS_ERR_NO_DEVICE;
    }
  c->pm_stream = std::move(sp);
  c->walk_stream = std::move(sw);
  c->pm_stream_cus = R;
  return NGRAVS_OK;
}

// PM steps that can run PM beside the walk: one task, the group walk of a TreePM run
static bool overlap_eligible(const ngravs_ctx *c)
{
  return c->cfg.pmgrid && c->cfg.periodic && c->cfg.world_size == 1 && !c->top.on && c->cfg.walk_mode == NGRAVS_WALK_GROUP &&
         c->n > 0 && c->n_local > 0;
}

// The walk (traversal, evaluation, k_finish) in two halves, so that the host can enqueue PM on pm_stream between them: the walk
// needs nothing from PM, and its first kernel should be in the queue when the tree is done, not behind the host's work on PM's
// launches.
// First half: tree and tables made sure of, every launch of the walk enqueued.  beside_pm: PM runs on pm_stream beside it.
// *masked: the walk went to walk_stream; *empty: this task has no targets (nothing enqueued, nothing to finish).
static int gravity_tree_begin(ngravs_ctx *c, bool beside_pm, bool *masked, bool *empty)
{
  *masked = *empty = false;
  if(!c || !c->have_order)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  int rc;
  if(!c->have_tree)   // gravtree.c:56-67
    {
      int64_t nn = ngravs_force_treebuild(c);
      if(nn < 0)
        return (int)nn;
    }
  else if(c->tree_stale && (rc = ngravs_force_update_tree(c)))   // drifted tree: refresh columns and moments first
    return rc;
  if((rc = ensure_table(c)))
    return rc;
  if(c->n_local == 0)   // no targets on this task
    {
      c->stats.t_treewalk = 0;
      c->stats.walk_kernel_ms = 0;
      c->stats.interactions = 0;
      c->stats.n_active = 0;
      c->have_acc = true;
      *empty = true;
      return NGRAVS_OK;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  // the walk alone on walk_stream: beside PM, or (stand-alone calls) when the pm_cus knob forces the masked streams
  *masked = (beside_pm || (c->tune.pm_cus > 0 && overlap_eligible(c))) && masked_streams(c, beside_pm ? c->pm_stream_cus : c->tune.pm_cus) == NGRAVS_OK;
  if(*masked)
    {
      HIP_TRY(c, hipStreamWaitEvent(c->walk_stream, c->ev0, 0));
      OnStream on(c, c->walk_stream, c->device_cus - c->pm_stream_cus);
      return walk_enqueue(c);
    }
  return walk_enqueue(c);
}

// Second half: waits for the walk, then k_finish.  pm_done: PM was enqueued on pm_stream beside it, and k_finish waits for that event.
static int gravity_tree_end(ngravs_ctx *c, bool masked, hipEvent_t pm_done)
{
  int rc;
  if(masked)
    {
      {
        OnStream on(c, c->walk_stream, c->device_cus - c->pm_stream_cus);
        if((rc = walk_complete(c)))
          return rc;
      }
      HIP_TRY(c, hipEventRecord(c->ev_walk, c->walk_stream));
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_walk, 0));
    }
  else if((rc = walk_complete(c)))
    return rc;
  if(pm_done)
    HIP_TRY(c, hipStreamWaitEvent(c->stream, pm_done, 0));
  if((rc = walk_finish(c)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->stats.t_treewalk = ev_ms(c) * 1e-3;
  float kms = 0;
  (void)hipEventSynchronize(c->evk1);
  (void)hipEventElapsedTime(&kms, c->evk0, c->evk1);
  c->stats.walk_kernel_ms = kms;
  // Nf and interaction sum (gravtree.c:74-78, 408-447)
  double h[2] = {0, 0};   // summed by k_finish
  HIP_TRY(c, hipMemcpyAsync(h, c->red_tmp.p, 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  c->stats.interactions = h[0];
  c->stats.n_active = (int64_t)h[1];
  c->have_acc = true;
  if(c->cfg.pmgrid && c->cfg.walk_mode == NGRAVS_WALK_GROUP && h[1] > 0 && c->cfg.box_size > 0)
    {
      // pairs per target against the uniform expectation: the cut sphere's volume times the mean density of ALL tasks' particles
      const double reach = (c->cfg.group_reach > 0 ? c->cfg.group_reach : NGRAVS_GROUP_REACH) * c->asmth;
      const double ntot = c->top.on && c->top.total_count > 0 ? c->top.total_count : (double)c->n;
      const double L = c->cfg.box_size, expect = 4.18879020478639 * reach * reach * reach * ntot / (L * L * L);
      // The figure depends on the unit and the spread the walk used (clustered 2^20 probe: 1857 / 1393 / 1079 pairs per target for
      // units of 4 / 2 / 1 groups, 871 for 1 group of 32 targets): it is kept as the equivalent for units of four groups of 64, and
      // only dense walks update it (a sparse active set says nothing about the next dense step).
      const bool dense = c->walk_ntargets < 0 || c->walk_dense_tlist;
      if(expect > 0 && dense)
        {
          const double f_sg = c->walk_sg >= 4 ? 1.0 : (c->walk_sg >= 2 ? 1857.0 / 1393.0 : 1857.0 / 1079.0);
          const double f_s = c->walk_spread >= 2 ? 1079.0 / 871.0 : 1.0;
          c->walk_ia_ratio = (h[0] / h[1]) / expect * f_sg * f_s;
        }
    }
  if(c->shard_count > 0 && c->extent_override)   // the work weights only matter to a multi-task domain cut
    hipLaunchKernelGGL(k_cost_update, GRID1(c->shard_count), 0, c->stream, c->s_idx.p, c->s_active.p, c->r_nint.p,
                       (long long)c->shard_first, (long long)c->shard_count, c->in_cost.p);
  return NGRAVS_OK;
}

extern "C" int ngravs_gravity_tree(ngravs_ctx *c)
{
  bool masked, empty;
  const int rc = gravity_tree_begin(c, false, &masked, &empty);
  return (rc || empty) ? rc : gravity_tree_end(c, masked, nullptr);
}

// PM on pm_stream, after what c->stream holds so far; the span is timed by ev_pm0 / ev_pm1
static int pm_on_masked_stream(ngravs_ctx *c)
{
  HIP_TRY(c, hipEventRecord(c->ev_fork, c->stream));
  HIP_TRY(c, hipStreamWaitEvent(c->pm_stream, c->ev_fork, 0));
  OnStream on(c, c->pm_stream, c->pm_stream_cus);
  HIP_TRY(c, hipEventRecord(c->ev_pm0, c->stream));
  int rc = pm_run(c);
  if(rc)
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev_pm1, c->stream));
  return NGRAVS_OK;
}

extern "C" int ngravs_pmforce_periodic(ngravs_ctx *c)
{
  if(!c || !c->have_particles)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  int rc;
  if(!c->have_order && (rc = ngravs_domain_decomposition(c)))   // domain.c:66-73: PM steps always re-decompose
    return rc;
  if(!c->have_tree)   // the mesh patches of the tiled deposit / gather are the cells of one tree level
    {
      int64_t nn = ngravs_force_treebuild(c);
      if(nn < 0)
        return (int)nn;
    }
  else if(c->tree_stale && (rc = ngravs_force_update_tree(c)))
    return rc;
  if(c->tune.pm_cus > 0 && overlap_eligible(c) && masked_streams(c, c->tune.pm_cus) == NGRAVS_OK)
    {
      // the pm_cus knob: PM alone on its reserved CUs (how the two halves of the overlapped step are timed one at a time)
      if((rc = pm_on_masked_stream(c)))
        return rc;
      float ms = 0;
      HIP_TRY(c, hipEventSynchronize(c->ev_pm1));
      (void)hipEventElapsedTime(&ms, c->ev_pm0, c->ev_pm1);
      HIP_TRY(c, hipStreamWaitEvent(c->stream, c->ev_pm1, 0));
      c->stats.t_pm = ms * 1e-3;
      return NGRAVS_OK;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  if((rc = pm_run(c)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  c->stats.t_pm = ev_ms(c) * 1e-3;
  return NGRAVS_OK;
}

// Reserved CUs for PM beside the walk in this step (0: one after another), from the PM and walk spans of the second serial PM step
// of the particle set (the first is often a different walk: the reference's first force computation opens by the angle alone): the smallest R whose PM, PM_CU_SCALE x its whole-device span, ends inside the walk on the other 256 - R CUs
// with PM_FIT_MARGIN to spare, if the overlapped step is predicted to be shorter than the serial one (the walk, slower on fewer CUs,
// also loses PM_SHARE_COST beside PM's traffic).  A step whose PM ended after the walk moves R one notch up (to serial after 32);
// R never comes down for the same particle set, so that the streams are not recreated from step to step.
// Measured at C4 (2^26 particles, N_GRAVS = 2, PMGRID = 512): PM alone took 17.4 ms on 256 CUs and 309.5 / 158.2 /
// 107.4 / 82.6 ms on 8 / 16 / 24 / 32; the walk 78.8 ms on 256 and 89.8 ms on 224 CUs alone, 93.0 ms beside PM.
static const double PM_CU_SCALE[4] = {17.75, 9.07, 6.16, 4.74};
static const double PM_FIT_MARGIN = 1.05, PM_SHARE_COST = 1.04;
static int choose_pm_cus(ngravs_ctx *c)
{
  if(!overlap_eligible(c))
    return 0;
  if(c->tune.pm_cus >= 0)
    return c->tune.pm_cus;
  if(c->pm_auto_cus >= 0)
    return c->pm_auto_cus;
  if(c->pm_solo_steps < 2 || c->pm_solo_ms <= 0 || c->walk_solo_ms <= 0)
    return 0;   // (this step measures them)
  c->pm_auto_cus = 0;
  for(int m = 1; m <= 4; m++)
    {
      const double walk = c->walk_solo_ms * 256.0 / (256 - 8 * m);
      // (the walk PM has to end inside is the walk BESIDE PM: since the traversal skips the moments of the nodes it is sure to
      // open, C4's walk alone is 76-77 ms, and measured against the walk without PM_SHARE_COST the test sat on its threshold,
      // 87.35 against 87.3-88.3 ms -- one run in three fell back to the serial step, 107.5 instead of 102.7 ms, although PM took
      // 85.7 ms beside a walk of 90.3)
      if(c->pm_solo_ms * PM_CU_SCALE[m - 1] * PM_FIT_MARGIN < walk * PM_SHARE_COST)
        {
          if(walk * PM_SHARE_COST < 0.99 * (c->pm_solo_ms + c->walk_solo_ms))
            c->pm_auto_cus = 8 * m;
          break;
        }
    }
  return c->pm_auto_cus;
}

extern "C" int ngravs_compute_accelerations(ngravs_ctx *c, int pm_step)
{
  if(!c || !c->have_particles)
    return NGRAVS_ERR_STATE;
  int rc;
  if((rc = domain_decomposition_impl(c, !(pm_step && c->cfg.pmgrid))))
    return rc;
  c->last_pm_cus = 0;
  if(!(pm_step && c->cfg.pmgrid))
    return ngravs_gravity_tree(c);                                      // accel.c:46
  const int R = choose_pm_cus(c);
  if(R > 0 && masked_streams(c, R) == NGRAVS_OK)
    {
      // PM (accel.c:34-42) does not feed the walk: the tree first, then PM on its reserved CUs beside the walk on the others;
      // only k_finish, which adds GravPM, waits for both
      int64_t nn = ngravs_force_treebuild(c);
      if(nn < 0)
        return (int)nn;
      // the walk's launches first: its traversal starts when the tree is done, while the host is still enqueuing PM
      bool masked, empty;
      if((rc = gravity_tree_begin(c, true, &masked, &empty)))
        return rc;
      if((rc = pm_on_masked_stream(c)))
        return rc;
      if(!empty && (rc = gravity_tree_end(c, masked, c->ev_pm1)))
        return rc;
      float ms = 0;
      (void)hipEventElapsedTime(&ms, c->ev_pm0, c->ev_pm1);   // (complete: k_finish waited for it)
      c->stats.t_pm = ms * 1e-3;
      c->last_pm_cus = R;
      if(c->tune.pm_cus < 0 && ms > c->stats.walk_kernel_ms)   // PM did not fit beside the walk: more CUs next time
        c->pm_auto_cus = R < 32 ? R + 8 : 0;
      return NGRAVS_OK;
    }
  if((rc = ngravs_pmforce_periodic(c)))   // accel.c:34-42
    return rc;
  if((rc = ngravs_gravity_tree(c)))       // accel.c:46
    return rc;
  if(overlap_eligible(c) && c->tune.pm_cus < 0 && c->pm_auto_cus < 0)
    {
      c->pm_solo_ms = c->stats.t_pm * 1e3;
      c->walk_solo_ms = c->stats.walk_kernel_ms;
      c->pm_solo_steps++;
    }
  return NGRAVS_OK;
}

// ---- results ----------------------------------------------------------------------------------------
extern "C" int ngravs_get_accel(ngravs_ctx *c, double *grav_accel, int64_t accel_stride, double *grav_pm, int64_t pm_stride,
                                double *old_acc, int64_t old_acc_stride, float *grav_cost, int64_t cost_stride, int on_device,
                                int only_active)
{
  if(!c || !c->have_order)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  // the working set is own rows [0, n_local) followed by imported copies; ONLY the own rows are the caller's (its arrays hold
  // NumPart = ngravs_dd_num_local() rows -- the imports of a multi-task step never reach them)
  const int64_t n = c->n, nl = c->n_local;
  if(nl == 0)   // a task without own particles: no rows to deliver
    return NGRAVS_OK;
  if(c->out_tmp.ensure(3 * n) || c->out_tmpf.ensure(n))
    return NGRAVS_ERR_NOMEM;
  // in_active is the caller-order flag column of the last hand-over
  const unsigned char *mask = only_active ? c->in_active.p : nullptr;
  int rc;
  if(grav_accel)
    {
      if(!c->have_acc)
        return NGRAVS_ERR_STATE;
      HIP_TRY(c, hipMemsetAsync(c->out_tmp.p, 0, sizeof(double) * 3 * n, c->stream));
      hipLaunchKernelGGL(k_unpermute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 3, c->r_acc.p, c->out_tmp.p);
      if((rc = col_download(c, c->out_tmp.p, sizeof(double), 3, nl, grav_accel, accel_stride, on_device, mask)))
        return rc;
    }
  if(grav_pm)
    {
      if(!c->have_pm)
        return NGRAVS_ERR_STATE;
      hipLaunchKernelGGL(k_unpermute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 3, c->r_pm.p, c->out_tmp.p);
      if((rc = col_download(c, c->out_tmp.p, sizeof(double), 3, nl, grav_pm, pm_stride, on_device, nullptr)))
        return rc;
    }
  if(old_acc)
    {
      if(!c->have_acc)
        return NGRAVS_ERR_STATE;
      hipLaunchKernelGGL(k_unpermute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 1, c->r_oldacc.p, c->out_tmp.p);
      if((rc = col_download(c, c->out_tmp.p, sizeof(double), 1, nl, old_acc, old_acc_stride, on_device, mask)))
        return rc;
    }
  if(grav_cost)
    {
      if(!c->have_acc)
        return NGRAVS_ERR_STATE;
      hipLaunchKernelGGL(k_unpermute_i2f, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, c->r_nint.p, c->out_tmpf.p);
      if((rc = col_download(c, c->out_tmpf.p, sizeof(float), 1, nl, grav_cost, cost_stride, on_device, mask)))
        return rc;
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_get_stats(ngravs_ctx *c, ngravs_stats_t *out)
{
  if(!c || !out)
    return NGRAVS_ERR_ARG;
  *out = c->stats;
  return NGRAVS_OK;
}

// ---- kept decomposition (include/ngravs_hip.h, ngravs_host_kept_step)
static std::string kept_state(const ngravs_ctx *c, const char *who)
{
  char b[320];
  snprintf(b, sizeof(b), "%s: no kept decomposition to work on (own rows %lld, rows at the cut %lld, working set %lld, tree %d, top %d, task %d of %d)", who,
           (long long)c->n_local, (long long)c->top.own_leaf_n, (long long)c->n, (int)c->have_tree, (int)c->top.on, c->top.kept_rank, c->top.kept_world);
  return std::string(b);
}
extern "C" int ngravs_dd_leaf_sums_kept(ngravs_ctx *c, void **dev_sums, int64_t *count)
{
  if(!c || !dev_sums || !count)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int rc = dd_leaf_sums_kept(c, dev_sums, count);
  if(rc == NGRAVS_ERR_STATE)
    ngravs_report(c, rc, kept_state(c, "ngravs_dd_leaf_sums_kept"));
  return rc;
}
extern "C" int ngravs_dd_pack_leaves_kept(ngravs_ctx *c, int64_t *counts, void **dev_records, int64_t *nrec)
{
  if(!c || !counts || !dev_records || !nrec)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int rc = dd_pack_leaves_kept(c, counts, dev_records, nrec);
  if(rc == NGRAVS_ERR_STATE)
    ngravs_report(c, rc, kept_state(c, "ngravs_dd_pack_leaves_kept"));
  return rc;
}
extern "C" int ngravs_dd_refresh_halo(ngravs_ctx *c, const void *dev_records, int64_t nrec)
{
  if(!c || nrec < 0 || (nrec > 0 && !dev_records))
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int rc = dd_refresh_halo(c, dev_records, nrec);
  if(rc == NGRAVS_ERR_STATE)
    ngravs_report(c, rc, kept_state(c, "ngravs_dd_refresh_halo"));
  return rc;
}
extern "C" int ngravs_dd_update_top(ngravs_ctx *c, const double *node_sums, const double *leaf_len)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  const int rc = dd_update_top(c, node_sums, leaf_len);
  if(rc == NGRAVS_ERR_STATE)
    ngravs_report(c, rc, kept_state(c, "ngravs_dd_update_top"));
  return rc;
}
extern "C" int ngravs_dd_get_kept(ngravs_ctx *c, int32_t *rank, int32_t *world, const int32_t **leaf_owner, const uint8_t **present,
                                  const double **node_sums)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const TopTree &t = c->top;
  if(!(t.on && t.h.nnode > 0 && t.own_leaf_n == c->n_local && t.kept_rank >= 0 && (int)t.h_leaf_owner.size() == t.h.nleaf &&
       (int)t.h_present.size() == t.h.nleaf))
    {
      ngravs_report(c, NGRAVS_ERR_STATE, kept_state(c, "ngravs_dd_get_kept"));
      return NGRAVS_ERR_STATE;
    }
  if(rank)
    *rank = t.kept_rank;
  if(world)
    *world = t.kept_world;
  if(leaf_owner)
    *leaf_owner = t.h_leaf_owner.data();
  if(present)
    *present = t.h_present.data();
  if(node_sums)
    *node_sums = t.h_node_sums.data();
  return NGRAVS_OK;
}

extern "C" int ngravs_walk_unopened(ngravs_ctx *c, int64_t *count)
{
  if(!c || !count)
    return NGRAVS_ERR_ARG;
  *count = (int64_t)c->walk_unopened;
  return NGRAVS_OK;
}

extern "C" int ngravs_walk_moment_skips(ngravs_ctx *c, int64_t *skips, int64_t *within_reach)
{
  if(!c || !skips)
    return NGRAVS_ERR_ARG;
  *skips = (int64_t)c->walk_moment_skips;
  if(within_reach)
    *within_reach = (int64_t)c->walk_head_survivors;
  return NGRAVS_OK;
}

extern "C" int ngravs_get_domain(ngravs_ctx *c, double out[8])
{
  if(!c || !c->have_order)
    return NGRAVS_ERR_STATE;
  memcpy(out, c->dom, sizeof(double) * 8);
  return NGRAVS_OK;
}

extern "C" int ngravs_get_keys(ngravs_ctx *c, int64_t *keys, int on_device)
{
  if(!c || !c->have_order || !keys)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  const int64_t n = c->n;
  if(c->out_tmp.ensure(3 * n))
    return NGRAVS_ERR_NOMEM;
  long long *tmp = reinterpret_cast<long long *>(c->out_tmp.p);
  hipLaunchKernelGGL(k_key18, GRID1(n), 0, c->stream, c->in_key.p, (long long)n, tmp);
  return col_download(c, tmp, sizeof(long long), 1, c->n_local, keys, sizeof(long long), on_device, nullptr);   // own rows
}

extern "C" int ngravs_get_order(ngravs_ctx *c, int32_t *order, int on_device)
{
  if(!c || !c->have_order || !order)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return col_download(c, c->s_idx.p, sizeof(int), 1, c->n, order, sizeof(int), on_device, nullptr);
}

extern "C" int ngravs_get_shard(ngravs_ctx *c, int64_t *first, int64_t *count)
{
  if(!c || !c->have_order)
    return NGRAVS_ERR_STATE;
  if(first)
    *first = c->shard_first;
  if(count)
    *count = c->shard_count;
  return NGRAVS_OK;
}

extern "C" const char *ngravs_last_error(ngravs_ctx *c) { return c ? c->last_error.c_str() : g_create_error.c_str(); }
extern "C" int ngravs_last_walk_kernel(ngravs_ctx *c) { return c ? c->last_walk_kernel : NGRAVS_ERR_ARG; }
extern "C" int ngravs_last_pm_cus(ngravs_ctx *c) { return c ? c->last_pm_cus : NGRAVS_ERR_ARG; }

// ngravs_cu_probe: where the workgroups launched on a stream run.  Each workgroup takes a whole CU (its LDS) for about 20 us and
// records XCC_ID << 8 | bits 8-15 of HW_ID (CU, SH and SE of the CU); hardware registers are only read.
#define CU_PROBE_LDS (96 * 1024)
__global__ void k_cu_probe(int *out, int n)
{
  extern __shared__ int probe_lds[];
  if(threadIdx.x != 0)
    return;
  unsigned xcc = 0, hw = 0;
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc));
  asm volatile("s_getreg_b32 %0, hwreg(HW_REG_HW_ID)" : "=s"(hw));
  probe_lds[0] = (int)(((xcc & 15u) << 8) | ((hw >> 8) & 0xffu));
  const unsigned long long t0 = wall_clock64();
  while(wall_clock64() - t0 < 2000)   // 20 us of the 100 MHz clock
    __builtin_amdgcn_s_sleep(8);
  if((int)blockIdx.x < n)
    out[blockIdx.x] = probe_lds[0];
}

extern "C" int ngravs_cu_probe(ngravs_ctx *c, int which, int nblocks, int32_t *cu_ids)
{
  if(!c || !cu_ids || nblocks < 1 || nblocks > 65536 || which < 0 || which > 2)
    return NGRAVS_ERR_ARG;
  if(which > 0 && !c->pm_stream)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  hipStream_t s = which == 0 ? c->stream : (which == 1 ? c->pm_stream : c->walk_stream);
  if(c->probe_out.ensure((size_t)nblocks))
    return NGRAVS_ERR_NOMEM;
  HIP_TRY(c, hipFuncSetAttribute(reinterpret_cast<const void *>(k_cu_probe), hipFuncAttributeMaxDynamicSharedMemorySize, CU_PROBE_LDS));
  hipLaunchKernelGGL(k_cu_probe, dim3((unsigned)nblocks), dim3(64), CU_PROBE_LDS, s, c->probe_out.p, nblocks);
  HIP_TRY(c, hipGetLastError());
  HIP_TRY(c, hipMemcpyAsync(cu_ids, c->probe_out.p, sizeof(int) * nblocks, hipMemcpyDeviceToHost, s));
  HIP_TRY(c, hipStreamSynchronize(s));
  return NGRAVS_OK;
}

// ---- stand-alone pieces -------------------------------------------------------------------------------
extern "C" int64_t ngravs_peano_hilbert_key(int x, int y, int z, int bits) { return ngravs_ph_key(x, y, z, bits); }

extern "C" int ngravs_peano_keys(ngravs_ctx *c, const double *pos, int64_t n, const double corner[3], double fac, int bits,
                                 int64_t *keys)
{
  if(!c || !pos || !keys || n <= 0 || bits < 1 || bits > 21)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  DevBuf<double> dpos;
  DevBuf<long long> dkeys;
  if(dpos.ensure(3 * n) || dkeys.ensure(n))
    return NGRAVS_ERR_NOMEM;
  int rc = NGRAVS_OK;
  if(hipMemcpyAsync(dpos.p, pos, sizeof(double) * 3 * n, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  if(!rc)
    rc = dom_keys_only(c, dpos.p, n, corner, fac, bits, dkeys.p);
  if(!rc && hipMemcpyAsync(keys, dkeys.p, sizeof(long long) * n, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

extern "C" int ngravs_shortrange_table(const ngravs_config_t *cfg, double *force_out, double *pot_out)
{
  if(!cfg || !force_out || cfg->n_gravs < 1 || cfg->n_gravs > NGRAVS_MAX_GRAVS)
    return NGRAVS_ERR_ARG;
  host_shortrange_table(cfg, force_out, pot_out);
  return NGRAVS_OK;
}

extern "C" int ngravs_shortrange_table_with_laws(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, double *force_out,
                                                 double *pot_out)
{
  if(!cfg || !force_out || cfg->n_gravs < 1 || cfg->n_gravs > NGRAVS_MAX_GRAVS || nfns < 0 || nfns > NGRAVS_MAX_USER_FNS ||
     (nfns > 0 && !fns))
    return NGRAVS_ERR_ARG;
  for(int i = 0; i < cfg->n_gravs; i++)
    for(int j = 0; j < cfg->n_gravs; j++)
      {
        const int law = cfg->law_normed[i][j], k = law - NGRAVS_LAW_USER0;
        if(law >= NGRAVS_LAW_USER0 && (k >= nfns || fns[k].kind != NGRAVS_USER_NORMED || !fns[k].fn))
          return NGRAVS_ERR_WIRING;
      }
  host_shortrange_table(cfg, force_out, pot_out, fns, nfns);
  return NGRAVS_OK;
}

extern "C" int ngravs_direct_sum(ngravs_ctx *c, const int32_t *idx, int64_t nt, double *acc)
{
  if(!c || !c->have_order || !idx || !acc || nt <= 0)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  DevBuf<int> inv, din, dout;
  DevBuf<double> dacc;
  if(inv.ensure(c->n) || din.ensure(nt) || dout.ensure(nt) || dacc.ensure(3 * nt))
    return NGRAVS_ERR_NOMEM;
  int rc = NGRAVS_OK;
  hipLaunchKernelGGL(k_inverse_perm, GRID1(c->n), 0, c->stream, c->s_idx.p, (long long)c->n, inv.p);
  if(hipMemcpyAsync(din.p, idx, sizeof(int) * nt, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  hipLaunchKernelGGL(k_map_idx, GRID1(nt), 0, c->stream, inv.p, din.p, (long long)nt, dout.p);
  if(!rc)
    rc = direct_run(c, dout.p, nt, dacc.p);
  if(!rc && hipMemcpyAsync(acc, dacc.p, sizeof(double) * 3 * nt, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

extern "C" int ngravs_direct_sum_targets(ngravs_ctx *c, const double *pos, const double *mass, const int32_t *type, int64_t nt, double *acc)
{
  if(!c || !c->have_order || !pos || !type || !acc || nt <= 0)
    return NGRAVS_ERR_STATE;
  for(int64_t k = 0; k < nt; k++)
    if(type[k] < 0 || type[k] >= NGRAVS_NTYPES)
      return NGRAVS_ERR_ARG;
  if(c->gsoft_on)
    {
      ngravs_report(c, NGRAVS_ERR_STATE, "ngravs_direct_sum_targets: adaptive gas softening is on and explicit targets carry no "
                                         "softening length (ngravs_set_gas_softening(ctx, NULL, 0, 0) switches it off)");
      return NGRAVS_ERR_STATE;
    }
  (void)hipSetDevice(c->cfg.device);
  DevBuf<double4> dt;
  DevBuf<int> dty;
  DevBuf<double> dacc;
  if(dt.ensure(nt) || dty.ensure(nt) || dacc.ensure(3 * nt))
    return NGRAVS_ERR_NOMEM;
  std::vector<double4> h((size_t)nt);
  double far = 0;   // user-defined laws: the farthest target from the domain's centre (table_reach)
  for(int64_t k = 0; k < nt; k++)
    {
      h[k].x = pos[3 * k];
      h[k].y = pos[3 * k + 1];
      h[k].z = pos[3 * k + 2];
      h[k].w = mass ? mass[k] : 1.0;
      const double dx = h[k].x - c->dom[3], dy = h[k].y - c->dom[4], dz = h[k].z - c->dom[5];
      far = fmax(far, sqrt(dx * dx + dy * dy + dz * dz));
    }
  int rc = NGRAVS_OK;
  if(hipMemcpyAsync(dt.p, h.data(), sizeof(double4) * nt, hipMemcpyHostToDevice, c->stream) != hipSuccess ||
     hipMemcpyAsync(dty.p, type, sizeof(int) * nt, hipMemcpyHostToDevice, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  if(!rc)
    rc = direct_run_targets(c, dt.p, dty.p, nt, dacc.p, far);
  if(!rc && hipMemcpyAsync(acc, dacc.p, sizeof(double) * 3 * nt, hipMemcpyDeviceToHost, c->stream) != hipSuccess)
    rc = NGRAVS_ERR_NO_DEVICE;
  (void)hipStreamSynchronize(c->stream);
  return rc;
}

// ---- multi-task domain decomposition (host-driven collectives; see kernels_domain.hip) -------------------------------
extern "C" int64_t ngravs_dd_num_local(ngravs_ctx *c) { return c ? c->n_local : NGRAVS_ERR_ARG; }

extern "C" int ngravs_dd_local_extent(ngravs_ctx *c, double lo[3], double hi[3])
{
  if(!c || !c->have_particles)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(int rc = park_grav_pm(c))   // GravPM of the own rows outlives the order that is about to go (non-PM steps: gravtree.c:318-330)
    return rc;
  c->n = c->n_local;   // a new step: forget the previous halo
  c->have_order = c->have_tree = false;
  return dd_local_extent(c, lo, hi);
}

extern "C" int ngravs_dd_peano_order(ngravs_ctx *c, int force)
{
  if(!c || !c->have_particles)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(int rc = park_grav_pm(c))   // GravPM leaves the old order first: it moves with the rows as a caller-order column
    return rc;
  return dd_peano_order_own(c, force);
}

extern "C" int ngravs_dd_set_extent(ngravs_ctx *c, const double lo[3], const double hi[3])
{
  if(!c)
    return NGRAVS_ERR_ARG;
  c->extent_override = lo && hi;
  if(c->extent_override)
    {
      for(int j = 0; j < 3; j++)
        {
          c->ext_lo[j] = lo[j];
          c->ext_hi[j] = hi[j];
        }
      dd_apply_extent(c, lo, hi);
    }
  return NGRAVS_OK;
}

extern "C" int ngravs_dd_set_toptree(ngravs_ctx *c, int32_t nnode, const int32_t *child)
{
  if(!c || !child || nnode < 1)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  return dd_set_toptree(c, nnode, child);
}

extern "C" int ngravs_dd_get_toptree(ngravs_ctx *c, int32_t *nnode, const int32_t **child)
{
  if(!c || !nnode || !child)
    return NGRAVS_ERR_ARG;
  *nnode = c->top.h.nnode;
  *child = c->top.h.child;
  return NGRAVS_OK;
}

extern "C" int ngravs_host_toptree_borrow(ngravs_ctx *c, ngravs_toptree *view)
{
  if(!c || !view)
    return NGRAVS_ERR_ARG;
  *view = c->top.h;
  return NGRAVS_OK;
}

extern "C" int ngravs_dd_leaf_sums(ngravs_ctx *c, void **dev_sums, int64_t *count)
{
  if(!c || !c->have_particles || !c->extent_override || !dev_sums || !count)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_leaf_sums(c, dev_sums, count);
}

extern "C" int ngravs_dd_pack(ngravs_ctx *c, int what, const int32_t *leaf_owner, int nranks, int my_rank, int64_t *counts,
                              void **dev_records, int64_t *nrec)
{
  if(!c || !c->have_particles || !c->extent_override || !leaf_owner || !counts || !dev_records || !nrec)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_pack(c, what, leaf_owner, nranks, my_rank, counts, dev_records, nrec);
}

extern "C" int ngravs_get_domain_extent(ngravs_ctx *c, double out[8])
{
  if(!c || !c->extent_override || !out)
    return NGRAVS_ERR_STATE;
  memcpy(out, c->dom, sizeof(double) * 8);
  return NGRAVS_OK;
}

extern "C" int ngravs_dd_keep_margin(ngravs_ctx *c, double *margin)
{
  if(!c || !margin)
    return NGRAVS_ERR_ARG;
  *margin = c->tune.dd_keep * c->dom[6];
  return NGRAVS_OK;
}

extern "C" int ngravs_dd_target_bounds(ngravs_ctx *c, double out[2])
{
  if(!c || !c->have_particles || !out)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_target_bounds(c, out);
}

extern "C" int ngravs_dd_pack_leaves(ngravs_ctx *c, const uint64_t *reqmask, int nranks, int my_rank, int64_t *counts, void **dev_records,
                                     int64_t *nrec)
{
  if(!c || !c->have_particles || !c->extent_override || !reqmask || !counts || !dev_records || !nrec)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_pack_leaves(c, (const unsigned long long *)reqmask, nranks, my_rank, counts, dev_records, nrec);
}

extern "C" int ngravs_dd_set_top(ngravs_ctx *c, const double *node_sums, const uint8_t *present)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  // (periodic tree-only runs: the lattice-correction walk, forcetree.c:2077-2455, opens a node only if the force walk's criterion
  // opens it AND the node is large or straddles the half-box seam -- a subset of what the force walk opens, so the leaves the
  // import decision brings in for the force walk serve it too)
  (void)hipSetDevice(c->cfg.device);
  return dd_set_top(c, node_sums, present);
}

extern "C" int ngravs_dd_get_dest(ngravs_ctx *c, const int32_t *leaf_owner, int32_t *dest)
{
  if(!c || !c->have_particles || !c->extent_override || !leaf_owner || !dest)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_get_dest(c, leaf_owner, dest);
}

extern "C" int ngravs_dd_recv_buffer(ngravs_ctx *c, int64_t nrec, void **dev_records)
{
  if(!c || nrec < 0 || !dev_records)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  if(c->dd_recv.ensure((size_t)(nrec > 0 ? nrec : 1) * NGRAVS_DD_MAX_RECORD_BYTES))
    return NGRAVS_ERR_NOMEM;
  *dev_records = c->dd_recv.p;
  return NGRAVS_OK;
}

extern "C" int64_t ngravs_dd_record_bytes(ngravs_ctx *c, int what)
{
  return c ? (int64_t)sizeof(double) * dd_record_doubles(c, what) : NGRAVS_ERR_ARG;
}

extern "C" int ngravs_dd_apply_migration(ngravs_ctx *c, const void *dev_records, int64_t nrec)
{
  if(!c || !c->have_particles || nrec < 0)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_apply_migration(c, dev_records, nrec);
}

extern "C" int ngravs_dd_set_halo(ngravs_ctx *c, const void *dev_records, int64_t nrec)
{
  if(!c || !c->have_particles || nrec < 0)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  return dd_set_halo(c, dev_records, nrec);
}

extern "C" int ngravs_dd_set_ids(ngravs_ctx *c, const int64_t *ids, int on_device)
{
  if(!c || !c->have_particles || !ids)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(c->n_local == 0)
    return NGRAVS_OK;
  HIP_TRY(c, hipMemcpyAsync(c->in_id.p, ids, sizeof(long long) * c->n_local, on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice,
                            c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

extern "C" int ngravs_dd_get_ids(ngravs_ctx *c, int64_t *ids, int on_device)
{
  if(!c || !c->have_particles || !ids)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(c->n_local == 0)
    return NGRAVS_OK;
  return col_download(c, c->in_id.p, sizeof(long long), 1, c->n_local, ids, sizeof(long long), on_device, nullptr);
}

// ---- slab-decomposed pmforce_periodic (kernels_pmslab.hip) ------------------------------------------------------------------
extern "C" int ngravs_pm_slab_begin(ngravs_ctx *c, int rank, int world, int32_t bbox[6])
{
  if(!c || !bbox)
    return NGRAVS_ERR_ARG;
  if(!c->have_order)
    return NGRAVS_ERR_STATE;
  (void)hipSetDevice(c->cfg.device);
  if(!c->have_tree)   // the patches of the tiled brick deposit are the cells of one tree level (as in ngravs_pmforce_periodic)
    {
      int64_t nn = ngravs_force_treebuild(c);
      if(nn < 0)
        return (int)nn;
    }
  else if(c->tree_stale)   // drifted particles: the sorted columns are refreshed by the refit
    {
      int rc = ngravs_force_update_tree(c);
      if(rc)
        return rc;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  int bb[6];
  int rc = pmslab_begin(c, rank, world, bb);
  for(int j = 0; j < 6; j++)
    bbox[j] = bb[j];
  return rc;
}

extern "C" int ngravs_pm_slab_pack(ngravs_ctx *c, int stage, const int32_t *all_bbox, int64_t *send_counts, int64_t *recv_counts,
                                   void **send, void **recv)
{
  if(!c || !send_counts || !recv_counts || !send || !recv)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  return pmslab_pack(c, stage, all_bbox, send_counts, recv_counts, send, recv);
}

extern "C" int ngravs_pm_slab_unpack(ngravs_ctx *c, int stage)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  (void)hipSetDevice(c->cfg.device);
  int rc = pmslab_unpack(c, stage);
  if(rc == NGRAVS_OK && stage == 3)
    {
      HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
      c->stats.t_pm = ev_ms(c) * 1e-3;
    }
  return rc;
}

extern "C" int ngravs_pm_slab_bytes(ngravs_ctx *c, double bytes[4])
{
  if(!c || !bytes)
    return NGRAVS_ERR_ARG;
  for(int k = 0; k < 4; k++)
    bytes[k] = c->pms.bytes_sent[k];
  return NGRAVS_OK;
}

// ---- SPH: what ngravs_sph_density and ngravs_sph_hydro share ------------------------------------------------------------------
// What every SPH call does once its arguments are checked: one task, a built tree of the current particle set (refit first when
// the particles drifted, as ngravs_gravity_tree does); then max_rounds (may be NULL) and the nms values of kernel_ms (may be NULL)
// read 0 for a call that ends early.
static int sph_begin(ngravs_ctx *c, const Refuse &refuse, int32_t *max_rounds, double *kernel_ms, int nms)
{
  if(c->cfg.world_size > 1 || c->top.on || c->n_local != c->n)
    return refuse(NGRAVS_ERR_STATE, "single task only (the neighbour search does not cross task boundaries yet)");
  if(!c->have_order || !c->have_tree)
    return refuse(NGRAVS_ERR_STATE, "needs a built tree of the current particle set");
  (void)hipSetDevice(c->cfg.device);
  if(c->tree_stale)
    if(int rc = ngravs_force_update_tree(c))
      return rc;
  if(max_rounds)
    *max_rounds = 0;
  for(int k = 0; kernel_ms && k < nms; k++)
    kernel_ms[k] = 0;
  return NGRAVS_OK;
}

// an engine without particles (or without a tree node) has nothing to walk
static bool sph_empty(const ngravs_ctx *c) { return c->n_local == 0 || c->nnodes <= 0; }

// what a density walk's statistics mean for the call: the log line, then the three ways it can have gone wrong
static int sph_density_outcome(ngravs_ctx *c, const SphStats &st, const Refuse &refuse)
{
  if(c->tune.sph_verbose && st.targets > 0)   // the reference logs every round of its iteration (density.c:409-414); here one line per call
    printf("ngravs_sph_density: %lld targets, rounds mean %.3f max %lld, %lld candidates tested, %lld neighbours\n", st.targets,
           (double)st.sum_rounds / (double)st.targets, st.max_rounds, st.candidates, st.neighbours);
  if(st.bad_hsml)
    return refuse(NGRAVS_ERR_ARG, "a target's starting hsml is <= 0 or not finite");
  if(st.stack_ovf)
    return refuse(NGRAVS_ERR_TREE, "the tree is deeper than the walk's stack");
  if(st.failed)
    {
      ngravs_report(c, 1155, "failed to converge in neighbour iteration in density()");   // density.c:416-421
      return NGRAVS_ERR_STATE;
    }
  return NGRAVS_OK;
}

// the own rows' columns that k_sph_hydro_prep / k_sph_gas_prep counted as bad
static int sph_hydro_rows_outcome(const SphHydroStats &st, const Refuse &refuse)
{
  if(st.bad_hsml)
    return refuse(NGRAVS_ERR_ARG, "a type-0 row's hsml is <= 0 or not finite");
  if(st.bad_density)
    return refuse(NGRAVS_ERR_ARG, "a type-0 row's density is <= 0 or not finite");
  if(st.bad_pressure)
    return refuse(NGRAVS_ERR_ARG, "a type-0 row's pressure is < 0 or not finite");
  return NGRAVS_OK;
}

// The hydro side of ngravs_hydro_in_t and ngravs_gas_in_t, whose switch and column fields carry the same names.  Three steps, because
// each entry point has checks of its own between them and the order of the refusals is part of its behaviour:
// whether the seven columns of the own rows are given (the caller words the refusal: its list of names differs),
template <class In> static bool sph_hydro_cols_given(const In *in)
{
  return in && in->vel_pred && in->hsml && in->density && in->pressure && in->dhsml_factor && in->div_vel && in->curl_vel;
}
// the switches,
template <class In> static int sph_hydro_switches(const In *in, const Refuse &refuse)
{
  if(!(in->gamma >= 1) || !(in->art_bulk_visc_const >= 0) || !(in->timebase_interval >= 0))
    return refuse(NGRAVS_ERR_ARG, "gamma must be >= 1, art_bulk_visc_const and timebase_interval >= 0");
  if(in->comoving && (!(in->hubble_a2 > 0) || !(in->fac_mu > 0) || !(in->fac_vsic_fix > 0)))
    return refuse(NGRAVS_ERR_ARG, "comoving: hubble_a2, fac_mu and fac_vsic_fix must be > 0");
  return NGRAVS_OK;
}
// and, after sph_begin, the upload of the seven columns to sph_vel_in, sph_h_in and sph_col_in with SphHydroParams from the switches
// (have_ts and the timestep columns stay with the caller)
template <class In> static int sph_hydro_own(ngravs_ctx *c, const In *in, const Refuse &refuse, SphHydroParams *hp)
{
  const int64_t n = c->n_local;
  int rc;
  if(c->sph_vel_in.ensure(3 * n) || c->sph_h_in.ensure(n) || c->sph_col_in.ensure(5 * n))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if((rc = col_upload(c, in->vel_pred, in->vel_pred_stride, sizeof(double), 3, n, in->on_device, c->sph_vel_in.p)))
    return rc;
  if((rc = col_upload(c, in->hsml, in->hsml_stride, sizeof(double), 1, n, in->on_device, c->sph_h_in.p)))
    return rc;
  const double *col[5] = {in->density, in->pressure, in->dhsml_factor, in->div_vel, in->curl_vel};
  const int64_t cstride[5] = {in->density_stride, in->pressure_stride, in->dhsml_factor_stride, in->div_vel_stride, in->curl_vel_stride};
  for(int k = 0; k < 5; k++)
    if((rc = col_upload(c, col[k], cstride[k], sizeof(double), 1, n, in->on_device, c->sph_col_in.p + k * n)))
      return rc;
  hp->periodic = c->cfg.periodic;
  hp->box = c->cfg.box_size;
  hp->boxhalf = 0.5 * c->cfg.box_size;
  hp->comoving = in->comoving != 0;
  hp->limiter = in->viscosity_limiter != 0;
  hp->have_ts = 0;
  hp->hubble_a2 = hp->comoving ? in->hubble_a2 : 1.0;   // hydra.c:96-97
  hp->fac_mu = hp->comoving ? in->fac_mu : 1.0;
  hp->fac_vsic_fix = hp->comoving ? in->fac_vsic_fix : 1.0;
  hp->visc = in->art_bulk_visc_const;
  hp->tbi = in->timebase_interval;
  hp->gamma = in->gamma;
  return NGRAVS_OK;
}

// sph_res [nres][nt] (list order) -> the targets' rows of the caller's strided columns dst[k] (NULL: not wanted)
static int sph_write_targets(ngravs_ctx *c, int nres, long long nt, double *const *dst, const int64_t *stride, int on_device)
{
  int rc;
  if(on_device)
    {
      for(int k = 0; k < nres; k++)
        if(dst[k] && (rc = sph_scatter(c, c->sph_res.p + k * nt, nt, dst[k], stride[k])))
          return rc;
      HIP_TRY(c, hipStreamSynchronize(c->stream));
      return NGRAVS_OK;
    }
  c->host_stage.resize((sizeof(double) * nres + sizeof(int)) * (size_t)nt);
  double *hres = reinterpret_cast<double *>(c->host_stage.data());
  int *hrow = reinterpret_cast<int *>(c->host_stage.data() + sizeof(double) * nres * (size_t)nt);
  HIP_TRY(c, hipMemcpyAsync(hres, c->sph_res.p, sizeof(double) * nres * nt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipMemcpyAsync(hrow, c->sph_row.p, sizeof(int) * nt, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  for(int k = 0; k < nres; k++)
    if(dst[k])
      for(long long t = 0; t < nt; t++)
        memcpy(reinterpret_cast<unsigned char *>(dst[k]) + hrow[t] * stride[k], &hres[k * nt + t], sizeof(double));
  return NGRAVS_OK;
}

// ---- SPH density (density.c:56-441 for one task; kernels_sph.hip) ---------------------------------------------------------
extern "C" int ngravs_sph_density(ngravs_ctx *c, const ngravs_sph_in_t *in, const ngravs_sph_out_t *out, int32_t *max_rounds, double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_density"};
  if(!in || !in->hsml || !in->vel_pred)
    return refuse(NGRAVS_ERR_ARG, "in, in->hsml and in->vel_pred must not be NULL");
  if(!(in->des_num_ngb > 0) || !(in->max_num_ngb_deviation >= 0) || !(in->min_gas_hsml >= 0))
    return refuse(NGRAVS_ERR_ARG, "des_num_ngb must be > 0, max_num_ngb_deviation and min_gas_hsml >= 0");
  int rc;
  if((rc = sph_begin(c, refuse, max_rounds, kernel_ms, 1)) || sph_empty(c))
    return rc;
  const int64_t n = c->n_local;
  if(c->sph_vel_in.ensure(3 * n) || c->sph_h_in.ensure(n) || c->sph_vel.ensure(3 * n))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if((rc = col_upload(c, in->vel_pred, in->vel_stride, sizeof(double), 3, n, in->on_device, c->sph_vel_in.p)))
    return rc;
  if((rc = col_upload(c, in->hsml, in->hsml_stride, sizeof(double), 1, n, in->on_device, c->sph_h_in.p)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  hipLaunchKernelGGL(k_permute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 3, c->sph_vel_in.p, c->sph_vel.p);
  SphStats st;
  if((rc = sph_density_run(c, in->des_num_ngb, in->max_num_ngb_deviation, in->min_gas_hsml, &st)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  if(kernel_ms)
    *kernel_ms = ev_ms(c);
  if((rc = sph_density_outcome(c, st, refuse)))
    return rc;
  if(max_rounds)
    *max_rounds = (int32_t)st.max_rounds;
  const long long nt = st.targets;
  if(nt == 0)
    return NGRAVS_OK;
  // only the targets' rows are written
  double *dst[SPH_NRES] = {in->hsml, nullptr, nullptr, nullptr, nullptr, nullptr};
  int64_t stride[SPH_NRES] = {in->hsml_stride, 0, 0, 0, 0, 0};
  if(out)
    {
      dst[SPH_DENSITY] = out->density, stride[SPH_DENSITY] = out->density_stride;
      dst[SPH_NUMNGB] = out->num_ngb, stride[SPH_NUMNGB] = out->num_ngb_stride;
      dst[SPH_DIVVEL] = out->div_vel, stride[SPH_DIVVEL] = out->div_vel_stride;
      dst[SPH_CURLVEL] = out->curl_vel, stride[SPH_CURLVEL] = out->curl_vel_stride;
      dst[SPH_DHSML] = out->dhsml_factor, stride[SPH_DHSML] = out->dhsml_factor_stride;
    }
  return sph_write_targets(c, SPH_NRES, nt, dst, stride, in->on_device);
}

// ---- the first smoothing-length guess (setup_smoothinglengths, init.c:229-247, for one task; kernels_sph.hip) -----------------
extern "C" int ngravs_sph_hsml_guess(ngravs_ctx *c, double des_num_ngb, double *hsml, int64_t hsml_stride, int32_t only_unset, int32_t on_device,
                                     double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_hsml_guess"};
  if(!hsml || !(des_num_ngb > 0))
    return refuse(NGRAVS_ERR_ARG, "hsml must not be NULL and des_num_ngb must be > 0");
  int rc;
  if((rc = sph_begin(c, refuse, nullptr, kernel_ms, 1)) || sph_empty(c))
    return rc;
  const int64_t n = c->n_local;
  if(only_unset)
    {
      if(c->sph_h_in.ensure(n))
        return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
      if((rc = col_upload(c, hsml, hsml_stride, sizeof(double), 1, n, on_device, c->sph_h_in.p)))
        return rc;
    }
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  long long rows = 0, bad_mass = 0;
  if((rc = sph_hsml_guess_run(c, des_num_ngb, only_unset != 0, &rows, &bad_mass)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  if(kernel_ms)
    *kernel_ms = ev_ms(c);
  if(bad_mass)
    return refuse(NGRAVS_ERR_ARG, "a type-0 row's mass is <= 0 or not finite");
  if(rows == 0)
    return NGRAVS_OK;
  double *dst[1] = {hsml};
  const int64_t stride[1] = {hsml_stride};
  return sph_write_targets(c, 1, rows, dst, stride, on_device);
}

// ---- SPH hydro force (hydra.c:50-346 for one task; kernels_sph.hip) ---------------------------------------------------------
static_assert(sizeof(ngravs_hydro_in_t) == 192 && sizeof(ngravs_hydro_out_t) == 48, "the Python mirror (abi.HydroIn / HydroOut) assumes this layout");
extern "C" int ngravs_sph_hydro(ngravs_ctx *c, const ngravs_hydro_in_t *in, const ngravs_hydro_out_t *out, double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_hydro"};
  if(!sph_hydro_cols_given(in))
    return refuse(NGRAVS_ERR_ARG, "in and its vel_pred, hsml, density, pressure, dhsml_factor, div_vel, curl_vel must not be NULL");
  int rc;
  if((rc = sph_hydro_switches(in, refuse)))
    return rc;
  if((rc = sph_begin(c, refuse, nullptr, kernel_ms, 1)) || sph_empty(c))
    return rc;
  const int64_t n = c->n_local;
  SphHydroParams hp;
  if((rc = sph_hydro_own(c, in, refuse, &hp)))
    return rc;
  if(c->sph_ts_in.ensure(n))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if(in->timestep && (rc = col_upload(c, in->timestep, in->timestep_stride, sizeof(int), 1, n, in->on_device, c->sph_ts_in.p)))
    return rc;
  hp.have_ts = in->timestep != nullptr;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  SphHydroStats st;
  if((rc = sph_hydro_run(c, hp, &st)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  if(kernel_ms)
    *kernel_ms = ev_ms(c);
  if((rc = sph_hydro_rows_outcome(st, refuse)))
    return rc;
  if(c->tune.sph_verbose && st.targets > 0)
    printf("ngravs_sph_hydro: %lld targets, %lld candidates tested, %lld pairs evaluated\n", st.targets, st.candidates, st.pairs);
  if(st.stack_ovf)
    return refuse(NGRAVS_ERR_TREE, "the tree is deeper than the walk's stack");
  const long long nt = st.targets;
  if(nt == 0 || !out)
    return NGRAVS_OK;
  // only the targets' rows are written
  double *dst[SPH_HY_NRES] = {out->hydro_accel, out->hydro_accel ? out->hydro_accel + 1 : nullptr, out->hydro_accel ? out->hydro_accel + 2 : nullptr,
                              out->dt_entropy, out->max_signal_vel};
  const int64_t stride[SPH_HY_NRES] = {out->hydro_accel_stride, out->hydro_accel_stride, out->hydro_accel_stride, out->dt_entropy_stride,
                                       out->max_signal_vel_stride};
  return sph_write_targets(c, SPH_HY_NRES, nt, dst, stride, in->on_device);
}

// ---- the gas side in one call: density() with its pressure line, force_update_hmax(), hydro_force() (kernels_sph.hip) ---------------
static_assert(sizeof(ngravs_gas_in_t) == 264 && sizeof(ngravs_gas_out_t) == 64, "the Python mirror (abi.GasIn / GasOut) assumes this layout");
extern "C" int ngravs_sph_accelerations(ngravs_ctx *c, const ngravs_gas_in_t *in, const ngravs_gas_out_t *out, int32_t *max_rounds,
                                        double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_accelerations"};
  if(!sph_hydro_cols_given(in) || !in->entropy)
    return refuse(NGRAVS_ERR_ARG, "in and its vel_pred, entropy, hsml, density, pressure, dhsml_factor, div_vel, curl_vel must not be NULL");
  if(!in->ti_begstep != !in->ti_endstep)
    return refuse(NGRAVS_ERR_ARG, "ti_begstep and ti_endstep must both be given or both be NULL");
  if(!(in->des_num_ngb > 0) || !(in->max_num_ngb_deviation >= 0) || !(in->min_gas_hsml >= 0))
    return refuse(NGRAVS_ERR_ARG, "des_num_ngb must be > 0, max_num_ngb_deviation and min_gas_hsml >= 0");
  int rc;
  if((rc = sph_hydro_switches(in, refuse)))
    return rc;
  if((rc = sph_begin(c, refuse, max_rounds, kernel_ms, 3)) || sph_empty(c))
    return rc;
  const int64_t n = c->n_local;
  SphHydroParams hp;
  if((rc = sph_hydro_own(c, in, refuse, &hp)))
    return rc;
  if(c->sph_vel.ensure(3 * n) || c->sph_gas_in.ensure(2 * n) || c->sph_ti_in.ensure(2 * n))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if((rc = col_upload(c, in->entropy, in->entropy_stride, sizeof(double), 1, n, in->on_device, c->sph_gas_in.p)))
    return rc;
  if(in->dt_entropy && (rc = col_upload(c, in->dt_entropy, in->dt_entropy_stride, sizeof(double), 1, n, in->on_device, c->sph_gas_in.p + n)))
    return rc;
  if(in->ti_begstep && ((rc = col_upload(c, in->ti_begstep, in->ti_begstep_stride, sizeof(int), 1, n, in->on_device, c->sph_ti_in.p)) ||
                        (rc = col_upload(c, in->ti_endstep, in->ti_endstep_stride, sizeof(int), 1, n, in->on_device, c->sph_ti_in.p + n))))
    return rc;
  SphGasParams gp;
  gp.des = in->des_num_ngb;
  gp.dev = in->max_num_ngb_deviation;
  gp.minh = in->min_gas_hsml;
  gp.ti_current = in->ti_current;
  gp.have_dte = in->dt_entropy != nullptr;
  hp.have_ts = in->ti_begstep != nullptr;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));    // (recorded again where the stages end: a call that ends early reads 0)
  HIP_TRY(c, hipEventRecord(c->evk0, c->stream));
  hipLaunchKernelGGL(k_permute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 3, c->sph_vel_in.p, c->sph_vel.p);
  SphStats ds;
  SphHydroStats hs;
  if((rc = sph_gas_run(c, gp, hp, &ds, &hs, c->ev1, c->evk0)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->evk1, c->stream));
  HIP_TRY(c, hipEventSynchronize(c->evk1));
  const bool density_only = ds.bad_hsml || ds.stack_ovf || ds.failed;
  if(kernel_ms && ds.targets > 0)
    {
      float ms[3] = {0, 0, 0};
      (void)hipEventElapsedTime(&ms[0], c->ev0, c->ev1);
      if(!density_only)
        {
          (void)hipEventElapsedTime(&ms[1], c->ev1, c->evk0);
          (void)hipEventElapsedTime(&ms[2], c->evk0, c->evk1);
        }
      for(int k = 0; k < 3; k++)
        kernel_ms[k] = ms[k];
    }
  if((rc = sph_density_outcome(c, ds, refuse)) || (rc = sph_hydro_rows_outcome(hs, refuse)))
    return rc;
  if(c->tune.sph_verbose && hs.targets > 0)
    printf("ngravs_sph_hydro: %lld targets, %lld candidates tested, %lld pairs evaluated\n", hs.targets, hs.candidates, hs.pairs);
  if(hs.stack_ovf)
    return refuse(NGRAVS_ERR_TREE, "the tree is deeper than the walk's stack");
  if(max_rounds)
    *max_rounds = (int32_t)ds.max_rounds;
  const long long nt = ds.targets;
  if(nt == 0)
    return NGRAVS_OK;
  // only the targets' rows are written, all columns in one pass
  double *dst[SPH_GAS_NRES] = {};
  int64_t stride[SPH_GAS_NRES] = {};
  dst[SPH_HSML] = in->hsml, stride[SPH_HSML] = in->hsml_stride;
  dst[SPH_DENSITY] = in->density, stride[SPH_DENSITY] = in->density_stride;
  dst[SPH_DIVVEL] = in->div_vel, stride[SPH_DIVVEL] = in->div_vel_stride;
  dst[SPH_CURLVEL] = in->curl_vel, stride[SPH_CURLVEL] = in->curl_vel_stride;
  dst[SPH_DHSML] = in->dhsml_factor, stride[SPH_DHSML] = in->dhsml_factor_stride;
  dst[SPH_GAS_PRESSURE] = in->pressure, stride[SPH_GAS_PRESSURE] = in->pressure_stride;
  if(out)
    {
      dst[SPH_NUMNGB] = out->num_ngb, stride[SPH_NUMNGB] = out->num_ngb_stride;
      for(int k = 0; k < 3; k++)
        dst[SPH_GAS_HYDRO + SPH_HY_ACCX + k] = out->hydro_accel ? out->hydro_accel + k : nullptr, stride[SPH_GAS_HYDRO + SPH_HY_ACCX + k] = out->hydro_accel_stride;
      dst[SPH_GAS_HYDRO + SPH_HY_DTENTR] = out->dt_entropy_out, stride[SPH_GAS_HYDRO + SPH_HY_DTENTR] = out->dt_entropy_out_stride;
      dst[SPH_GAS_HYDRO + SPH_HY_MAXSIG] = out->max_signal_vel, stride[SPH_GAS_HYDRO + SPH_HY_MAXSIG] = out->max_signal_vel_stride;
    }
  if(!in->on_device)
    return sph_write_targets(c, SPH_GAS_NRES, nt, dst, stride, 0);
  SphScatterCols cols;
  for(int k = 0; k < SPH_GAS_NRES; k++)
    cols.dst[k] = reinterpret_cast<unsigned char *>(dst[k]), cols.stride[k] = stride[k];
  if((rc = sph_scatter_cols(c, nt, cols)))
    return rc;
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

// ---- SPH sums for targets that are not own rows: density_evaluate(j, 1) / hydro_evaluate(j, 1) (kernels_sph.hip) ---------------------
static_assert(sizeof(ngravs_sph_targets_t) == 48 && sizeof(ngravs_hydro_targets_t) == 144 && sizeof(ngravs_sph_update_out_t) == 56,
              "the Python mirror (abi.SphTargets / HydroTargets / SphUpdateOut) assumes this layout");
extern "C" int ngravs_sph_density_sums(ngravs_ctx *c, const double *own_vel_pred, int64_t own_vel_stride, const ngravs_sph_targets_t *tg, int64_t nt,
                                       double *sums, int32_t on_device, double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_density_sums"};
  if(nt < 0 || nt > 0x7fffffff)
    return refuse(NGRAVS_ERR_ARG, "nt must be >= 0 (and below 2^31)");
  if(!own_vel_pred || !tg || (nt > 0 && (!tg->pos || !tg->vel || !tg->hsml || !sums)))
    return refuse(NGRAVS_ERR_ARG, "own_vel_pred, targets, its pos, vel, hsml and sums must not be NULL");
  int rc;
  if((rc = sph_begin(c, refuse, nullptr, kernel_ms, 1)) || nt == 0)
    return rc;
  const int64_t n = c->n_local;
  if(sph_empty(c))
    return col_deliver_or_zeros(c, nullptr, sizeof(double) * SPH_NSUMS * (size_t)nt, sums, on_device);
  if(c->sph_vel_in.ensure(3 * n) || c->sph_vel.ensure(3 * n) || c->sph_tg_in.ensure((size_t)(SPH_TG_H + 1 + 3) * nt))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if((rc = col_upload(c, own_vel_pred, own_vel_stride, sizeof(double), 3, n, on_device, c->sph_vel_in.p)))
    return rc;
  if((rc = col_upload(c, tg->pos, tg->pos_stride, sizeof(double), 3, nt, on_device, c->sph_tg_in.p)) ||
     (rc = col_upload(c, tg->vel, tg->vel_stride, sizeof(double), 3, nt, on_device, c->sph_tg_in.p + 3 * nt)) ||
     (rc = col_upload(c, tg->hsml, tg->hsml_stride, sizeof(double), 1, nt, on_device, c->sph_tg_in.p + SPH_TG_H * nt)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  hipLaunchKernelGGL(k_permute_f64, GRID1(n), 0, c->stream, c->s_idx.p, (long long)n, 3, c->sph_vel_in.p, c->sph_vel.p);
  SphSumsStats st;
  if((rc = sph_density_sums_run(c, nt, &st)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  if(kernel_ms)
    *kernel_ms = ev_ms(c);
  if(st.bad_hsml)
    return refuse(NGRAVS_ERR_ARG, "a target's hsml is <= 0 or not finite");
  if(st.bad_pos)
    return refuse(NGRAVS_ERR_ARG, "a target's position is not finite, or outside [0, BoxSize] in a periodic run");
  if(c->tune.sph_verbose)
    printf("ngravs_sph_density_sums: %lld targets, %lld candidates tested, %lld neighbours\n", (long long)nt, st.candidates, st.pairs);
  if(st.stack_ovf)
    return refuse(NGRAVS_ERR_TREE, "the tree is deeper than the walk's stack");
  return col_deliver_or_zeros(c, c->sph_tg_res.p, sizeof(double) * SPH_NSUMS * (size_t)nt, sums, on_device);
}

extern "C" int ngravs_sph_hydro_sums(ngravs_ctx *c, const ngravs_hydro_in_t *in, const ngravs_hydro_targets_t *tg, int64_t nt, double *sums,
                                     int32_t on_device, double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_sph_hydro_sums"};
  if(nt < 0 || nt > 0x7fffffff)
    return refuse(NGRAVS_ERR_ARG, "nt must be >= 0 (and below 2^31)");
  if(!sph_hydro_cols_given(in))
    return refuse(NGRAVS_ERR_ARG, "own and its vel_pred, hsml, density, pressure, dhsml_factor, div_vel, curl_vel must not be NULL");
  if(!tg || (nt > 0 && (!tg->pos || !tg->vel || !tg->hsml || !tg->mass || !tg->density || !tg->pressure || !tg->dhsml_factor || !tg->f1 || !sums)))
    return refuse(NGRAVS_ERR_ARG, "targets, its pos, vel, hsml, mass, density, pressure, dhsml_factor, f1 and sums must not be NULL");
  int rc;
  if((rc = sph_hydro_switches(in, refuse)))
    return rc;
  if((rc = sph_begin(c, refuse, nullptr, kernel_ms, 1)) || nt == 0)
    return rc;
  const int64_t n = c->n_local;
  if(sph_empty(c))
    return col_deliver_or_zeros(c, nullptr, sizeof(double) * SPH_HY_NRES * (size_t)nt, sums, on_device);
  SphHydroParams hp;
  if((rc = sph_hydro_own(c, in, refuse, &hp)))
    return rc;
  if(c->sph_ts_in.ensure(n) || c->sph_tg_in.ensure((size_t)(SPH_TG_NCOL + 3) * nt) || c->sph_tg_ts.ensure((size_t)nt))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if(in->timestep && (rc = col_upload(c, in->timestep, in->timestep_stride, sizeof(int), 1, n, in->on_device, c->sph_ts_in.p)))
    return rc;
  if((rc = col_upload(c, tg->pos, tg->pos_stride, sizeof(double), 3, nt, on_device, c->sph_tg_in.p)) ||
     (rc = col_upload(c, tg->vel, tg->vel_stride, sizeof(double), 3, nt, on_device, c->sph_tg_in.p + 3 * nt)))
    return rc;
  const double *tcol[6] = {tg->hsml, tg->mass, tg->density, tg->pressure, tg->dhsml_factor, tg->f1};
  const int64_t tstride[6] = {tg->hsml_stride, tg->mass_stride, tg->density_stride, tg->pressure_stride, tg->dhsml_factor_stride, tg->f1_stride};
  for(int k = 0; k < 6; k++)
    if((rc = col_upload(c, tcol[k], tstride[k], sizeof(double), 1, nt, on_device, c->sph_tg_in.p + (SPH_TG_H + k) * nt)))
      return rc;
  if(tg->timestep && (rc = col_upload(c, tg->timestep, tg->timestep_stride, sizeof(int), 1, nt, on_device, c->sph_tg_ts.p)))
    return rc;
  hp.have_ts = in->timestep != nullptr;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  SphSumsStats st;
  SphHydroStats own;
  if((rc = sph_hydro_sums_run(c, hp, nt, tg->timestep != nullptr, &st, &own)))
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
  if(kernel_ms)
    *kernel_ms = ev_ms(c);
  if((rc = sph_hydro_rows_outcome(own, refuse)))
    return rc;
  if(st.bad_hsml)
    return refuse(NGRAVS_ERR_ARG, "a target's hsml is <= 0 or not finite");
  if(st.bad_density)
    return refuse(NGRAVS_ERR_ARG, "a target's density is <= 0 or not finite");
  if(st.bad_pressure)
    return refuse(NGRAVS_ERR_ARG, "a target's pressure is < 0 or not finite");
  if(st.bad_pos)
    return refuse(NGRAVS_ERR_ARG, "a target's position is not finite, or outside [0, BoxSize] in a periodic run");
  if(c->tune.sph_verbose)
    printf("ngravs_sph_hydro_sums: %lld targets, %lld candidates tested, %lld pairs evaluated\n", (long long)nt, st.candidates, st.pairs);
  if(st.stack_ovf)
    return refuse(NGRAVS_ERR_TREE, "the tree is deeper than the walk's stack");
  return col_deliver_or_zeros(c, c->sph_tg_res.p, sizeof(double) * SPH_HY_NRES * (size_t)nt, sums, on_device);
}

extern "C" int64_t ngravs_sph_density_update(int64_t n, const double *sums, double *hsml, double *left, double *right, int32_t *rounds,
                                             double des_num_ngb, double max_num_ngb_deviation, double min_gas_hsml,
                                             const ngravs_sph_update_out_t *out, int32_t on_device)
{
  if(n < 0 || !out || (n > 0 && (!sums || !hsml || !left || !right || !rounds || !out->accepted)) || !(des_num_ngb > 0) ||
     !(max_num_ngb_deviation >= 0) || !(min_gas_hsml >= 0))
    {
      ngravs_report(nullptr, NGRAVS_ERR_ARG,
                    "ngravs_sph_density_update: n >= 0; sums, hsml, left, right, rounds, out and out->accepted must not be NULL; des_num_ngb > 0, "
                    "max_num_ngb_deviation and min_gas_hsml >= 0");
      return NGRAVS_ERR_ARG;
    }
  if(n == 0)
    return 0;
  double *const col[SPH_NRES] = {out->hsml, out->density, out->num_ngb, out->div_vel, out->curl_vel, out->dhsml_factor};
  long long failed = 0;
  if(on_device)
    {
      int rc = sph_density_update_device(n, sums, hsml, left, right, rounds, des_num_ngb, max_num_ngb_deviation, min_gas_hsml, out->accepted, col,
                                         &failed);
      return rc ? rc : failed;
    }
  for(int64_t t = 0; t < n; t++)   // GPU-free, as ngravs_sph_kernel is
    {
      double o[SPH_NRES];
      const int r = sph_density_update_one(sums + SPH_NSUMS * t, des_num_ngb, max_num_ngb_deviation, min_gas_hsml, &hsml[t], &left[t], &right[t],
                                           &rounds[t], o);
      out->accepted[t] = r == 0;
      if(r == 0)
        {
          for(int k = 0; k < SPH_NRES; k++)
            if(col[k])
              col[k][t] = o[k];
        }
      else if(r == 2)
        failed++;
    }
  return failed;
}

extern "C" int ngravs_sph_kernel(double h, const double *r, int64_t n, double *wk, double *dwk)
{
  if(!(h > 0) || n < 0 || (n > 0 && (!r || !wk || !dwk)))
    return NGRAVS_ERR_ARG;
  const double h2 = h * h, hinv = 1.0 / h, hinv3 = hinv * hinv * hinv, hinv4 = hinv3 * hinv;
  for(int64_t i = 0; i < n; i++)
    {
      wk[i] = dwk[i] = 0;
      if(r[i] * r[i] < h2)   // the pair test of density.c:531
        sph_spline(r[i] * hinv, hinv3, hinv4, &wk[i], &dwk[i]);
    }
  return NGRAVS_OK;
}

// ---- gravity for targets that are not own rows: the tree walk of force_treeevaluate(j, 1) / force_treeevaluate_shortrange(j, 1) /
// force_treeevaluate_lattice_correction(j, 1) for one task (gravtree.c:133-285), and GravPM of the last PM step at their places ------
static_assert(sizeof(ngravs_grav_targets_t) == 72, "the Python mirror (abi.GravTargets) assumes this layout");

// What both calls refuse before anything is staged: NULL arguments and nt < 0, several tasks, adaptive gas softening
static int grav_targets_refusals(ngravs_ctx *c, const Refuse &refuse, const ngravs_grav_targets_t *t, int64_t nt, const void *result,
                                 const char *result_name)
{
  if(!t)
    return refuse(NGRAVS_ERR_ARG, "targets is NULL");
  if(!t->pos)
    return refuse(NGRAVS_ERR_ARG, "targets->pos is NULL");
  if(!t->type)
    return refuse(NGRAVS_ERR_ARG, "targets->type is NULL");
  if(!result)
    return refuse(NGRAVS_ERR_ARG, std::string(result_name) + " is NULL");
  if(nt < 0 || nt > 0x7fffffff)
    return refuse(NGRAVS_ERR_ARG, "nt must be >= 0 (and below 2^31)");
  if(c->cfg.world_size > 1 || c->top.on || c->n_local != c->n)
    return refuse(NGRAVS_ERR_STATE, "single task only (the top-level short-cuts of the reference's walk for imported targets, "
                                    "forcetree.c:1424-1434, and a mesh in slabs are not served)");
  if(c->gsoft_on)
    return refuse(NGRAVS_ERR_STATE, "adaptive gas softening is on and explicit targets carry no softening length "
                                    "(ngravs_set_gas_softening(ctx, NULL, 0, 0) switches it off)");
  return NGRAVS_OK;
}

// The records into gt_in (pos[nt][3], old_acc[nt], mass[nt]) and gt_type; refused, with nothing written: a type outside 0..5, a
// position that is not finite, or outside [0, BoxSize] in a periodic configuration.  *far: grav_targets_check
static int grav_targets_stage(ngravs_ctx *c, const Refuse &refuse, const ngravs_grav_targets_t *t, int64_t nt, double *far)
{
  if(c->gt_in.ensure(8 * (size_t)nt) || c->gt_type.ensure((size_t)nt))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  int rc;
  if((rc = col_upload(c, t->pos, t->pos_stride, sizeof(double), 3, nt, t->on_device, c->gt_in.p)) ||
     (rc = col_upload(c, t->type, t->type_stride, sizeof(int), 1, nt, t->on_device, c->gt_type.p)))
    return rc;
  if(t->old_acc)
    rc = col_upload(c, t->old_acc, t->old_acc_stride, sizeof(double), 1, nt, t->on_device, c->gt_in.p + 3 * nt);
  else
    hipLaunchKernelGGL(k_fill_f64, GRID1(nt), 0, c->stream, c->gt_in.p + 3 * nt, (long long)nt, 0.0);
  if(rc)
    return rc;
  if(t->mass)
    rc = col_upload(c, t->mass, t->mass_stride, sizeof(double), 1, nt, t->on_device, c->gt_in.p + 4 * nt);
  else
    hipLaunchKernelGGL(k_fill_f64, GRID1(nt), 0, c->stream, c->gt_in.p + 4 * nt, (long long)nt, 1.0);
  if(rc)
    return rc;
  HIP_TRY(c, hipEventRecord(c->ev0, c->stream));
  GravTargetsStats st;
  if((rc = grav_targets_check(c, nt, &st, far)))
    return rc;
  if(st.bad_type)
    return refuse(NGRAVS_ERR_ARG, "a target's type is outside 0..5");
  if(st.bad_pos)
    return refuse(NGRAVS_ERR_ARG, "a target's position is not finite, or outside [0, BoxSize] in a periodic run");
  return NGRAVS_OK;
}

extern "C" int ngravs_gravity_tree_targets(ngravs_ctx *c, const ngravs_grav_targets_t *t, int64_t nt, double *acc, int32_t *nint,
                                           double *kernel_ms)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_gravity_tree_targets"};
  int rc;
  if((rc = grav_targets_refusals(c, refuse, t, nt, acc, "acc")))
    return rc;
  if(!c->have_order || !c->have_tree)
    return refuse(NGRAVS_ERR_STATE, "needs a built tree of the current particle set");
  if(kernel_ms)
    *kernel_ms = 0;
  if(nt == 0)
    return NGRAVS_OK;
  (void)hipSetDevice(c->cfg.device);
  if(c->tree_stale && (rc = ngravs_force_update_tree(c)))   // drifted tree: refresh columns and moments first, as ngravs_gravity_tree does
    return rc;
  if((rc = ensure_table(c)))
    return rc;
  double far = 0;
  if((rc = grav_targets_stage(c, refuse, t, nt, &far)))
    return rc;
  const bool empty = c->n_local == 0 || c->nnodes <= 0;   // nothing to walk: no force, no interaction
  if(!empty)
    {
      if((rc = walk_targets_run(c, nt, far)))
        return rc;
      HIP_TRY(c, hipEventRecord(c->ev1, c->stream));
      if(kernel_ms)
        *kernel_ms = ev_ms(c);
    }
  if((rc = col_deliver_or_zeros(c, empty ? nullptr : c->gt_acc.p, sizeof(double) * 3 * (size_t)nt, acc, t->on_device)))
    return rc;
  return nint ? col_deliver_or_zeros(c, empty ? nullptr : c->gt_nint.p, sizeof(int) * (size_t)nt, nint, t->on_device) : NGRAVS_OK;
}

extern "C" int ngravs_pm_targets(ngravs_ctx *c, const ngravs_grav_targets_t *t, int64_t nt, double *grav_pm)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_pm_targets"};
  int rc;
  if((rc = grav_targets_refusals(c, refuse, t, nt, grav_pm, "grav_pm")))
    return rc;
  if(!c->cfg.pmgrid)
    return refuse(NGRAVS_ERR_STATE, "the configuration has no mesh (PMGRID = 0)");
  if(!c->pm_mesh_valid)
    return refuse(NGRAVS_ERR_STATE, "no valid mesh: needs the potential of a PM step (ngravs_pmforce_periodic) of this task");
  if(nt == 0)
    return NGRAVS_OK;
  (void)hipSetDevice(c->cfg.device);
  double far = 0;
  if((rc = grav_targets_stage(c, refuse, t, nt, &far)))
    return rc;
  if(c->gt_acc.ensure(3 * (size_t)nt))
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  if((rc = pm_targets_run(c, nt, c->gt_acc.p)))
    return rc;
  return col_deliver_or_zeros(c, c->gt_acc.p, sizeof(double) * 3 * (size_t)nt, grav_pm, t->on_device);
}

// ---- gravitational potentials (kernels_potential.hip) --------------------------------------------------------------------------------
// What the potential calls refuse whatever the arguments: the configurations they are not built for, then a missing tree
static int potential_refusals(ngravs_ctx *c, const Refuse &refuse)
{
  if(c->cfg.world_size > 1 || c->top.on || c->n_local != c->n)
    return refuse(NGRAVS_ERR_ARG, "single task only (world_size > 1 or a multi-task working set)");
  if(c->gsoft_on)
    return refuse(NGRAVS_ERR_ARG, "adaptive gas softening is on (ngravs_set_gas_softening(ctx, NULL, 0, 0) switches it off)");
  for(int a = 0; a < c->cfg.n_gravs; a++)
    for(int b = 0; b < c->cfg.n_gravs; b++)
      {
        const int law = c->cfg.law_accel[a][b], spl = c->cfg.law_spline[a][b];
        const std::string at = "[" + std::to_string(a) + "][" + std::to_string(b) + "]";
        if(user_pot_entry(c, a, b))
          {
            // the model's own companions serve any law a table linear in the source mass can carry
            if((law >= NGRAVS_LAW_BAMBAM && law < NGRAVS_LAW_USER0) || (spl >= NGRAVS_SPLINE_BAMBAM && spl < NGRAVS_SPLINE_USER0))
              return refuse(NGRAVS_ERR_ARG, "law_accel / law_spline" + at + " is a BAM law: its potential depends on the target mass and on N, "
                                            "which a node's monopole cannot carry; BAM potentials are not served");
            continue;
          }
        if(law != NGRAVS_LAW_NONE && law != NGRAVS_LAW_NEWTON && law != NGRAVS_LAW_NEG_NEWTON)
          return refuse(NGRAVS_ERR_ARG, "law_accel" + at + " has no wired potential companion (only newtonian and neg_newtonian have; Yukawa, "
                                        "coloyuk, BAM and user laws are not served)");
        if(spl != NGRAVS_SPLINE_NONE && spl != NGRAVS_SPLINE_PLUMMER && spl != NGRAVS_SPLINE_NEG_PLUMMER)
          return refuse(NGRAVS_ERR_ARG, "law_spline" + at + " has no wired potential companion (only plummer and neg_plummer have; BAM and "
                                        "user splines are not served)");
      }
  if(c->cfg.pmgrid && !c->cfg.periodic)
    return refuse(NGRAVS_ERR_ARG, "a mesh without periodic boundaries (non-periodic PM) is not served");
  if(!c->have_order || !c->have_tree)
    return refuse(NGRAVS_ERR_STATE, "needs a built tree of the current particle set");
  return NGRAVS_OK;
}

extern "C" int ngravs_compute_potential(ngravs_ctx *c, const ngravs_time_params_t *par, double *potential, int64_t potential_stride,
                                        int32_t on_device, int32_t *nint)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_compute_potential"};
  if(!potential)
    return refuse(NGRAVS_ERR_ARG, "potential is NULL");
  if(on_device && potential_stride != (int64_t)sizeof(double))
    return refuse(NGRAVS_ERR_ARG, "a device column must be contiguous");
  int rc;
  if((rc = potential_refusals(c, refuse)))
    return rc;
  const int64_t n = c->n_local;
  if(n == 0)
    return NGRAVS_OK;
  if(c->nnodes <= 0)
    return refuse(NGRAVS_ERR_STATE, "the tree has no nodes");
  (void)hipSetDevice(c->cfg.device);
  if(c->tree_stale && (rc = ngravs_force_update_tree(c)))   // drifted tree: refresh columns and moments first
    return rc;
  if(c->out_tmp.ensure(3 * (size_t)n))   // [n] the column in caller order, behind it room for the counts
    return refuse(NGRAVS_ERR_NOMEM, "device allocation failed");
  int *d_nint = nint ? reinterpret_cast<int *>(c->out_tmp.p + n) : nullptr;
  if((rc = potential_run(c, par, c->out_tmp.p, d_nint)))
    return rc;
  if((rc = col_download(c, c->out_tmp.p, sizeof(double), 1, n, potential, potential_stride, on_device, nullptr)))
    return rc;
  return nint ? col_deliver_or_zeros(c, d_nint, sizeof(int) * (size_t)n, nint, on_device) : NGRAVS_OK;
}

extern "C" int ngravs_potential_targets(ngravs_ctx *c, const ngravs_grav_targets_t *t, int64_t nt, double *pot, int32_t *nint)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_potential_targets"};
  if(!t || !t->pos || !t->type || !pot)
    return refuse(NGRAVS_ERR_ARG, "targets, targets->pos, targets->type or pot is NULL");
  if(nt < 0 || nt > 0x7fffffff)
    return refuse(NGRAVS_ERR_ARG, "nt must be >= 0 (and below 2^31)");
  int rc;
  if((rc = potential_refusals(c, refuse)))
    return rc;
  if(c->cfg.pmgrid && !c->pot_mesh_valid)
    return refuse(NGRAVS_ERR_STATE, "no valid potential mesh: needs an ngravs_compute_potential since the last PM step and hand-over");
  if(nt == 0)
    return NGRAVS_OK;
  (void)hipSetDevice(c->cfg.device);
  if(c->tree_stale && (rc = ngravs_force_update_tree(c)))
    return rc;
  double far = 0;
  if((rc = grav_targets_stage(c, refuse, t, nt, &far)))
    return rc;
  const bool empty = c->n_local == 0 || c->nnodes <= 0;   // nothing to walk
  if(!empty && (rc = potential_targets_run(c, nt, far)))
    return rc;
  if((rc = col_deliver_or_zeros(c, empty ? nullptr : c->gt_acc.p, sizeof(double) * (size_t)nt, pot, t->on_device)))
    return rc;
  return nint ? col_deliver_or_zeros(c, empty ? nullptr : c->gt_nint.p, sizeof(int) * (size_t)nt, nint, t->on_device) : NGRAVS_OK;
}

extern "C" int ngravs_lattice_potential_table(ngravs_ctx *c, int32_t target, int32_t source, double *out)
{
  if(!c)
    return NGRAVS_ERR_ARG;
  const Refuse refuse = {c, "ngravs_lattice_potential_table"};
  const int ng = c->cfg.n_gravs;
  if(!out || target < 0 || target >= ng || source < 0 || source >= ng)
    return refuse(NGRAVS_ERR_ARG, "out is NULL, or the pair is outside [0, N_GRAVS)");
  if(!c->cfg.periodic || c->cfg.pmgrid)
    return refuse(NGRAVS_ERR_ARG, "only periodic configurations without a mesh read a lattice potential table");
  (void)hipSetDevice(c->cfg.device);
  int rc;
  if((rc = potential_lattice_ensure(c)))
    return rc;
  const size_t sz = (size_t)65 * 65 * 65;
  HIP_TRY(c, hipMemcpyAsync(out, c->pot_lat.p + ((size_t)target * ng + source) * sz, sizeof(double) * sz, hipMemcpyDeviceToHost, c->stream));
  HIP_TRY(c, hipStreamSynchronize(c->stream));
  return NGRAVS_OK;
}

extern "C" int ngravs_last_potential_ms(ngravs_ctx *c, double *walk_ms)
{
  if(!c || !walk_ms)
    return NGRAVS_ERR_ARG;
  *walk_ms = c->pot_walk_ms;
  return NGRAVS_OK;
}

// ---- time integration: drift, kick and timestep assignment (run.c:32-65 around the forces; kernels_time.hip) ------------------------
static_assert(sizeof(ngravs_time_cols_t) == 288 && sizeof(ngravs_time_params_t) == 168 && sizeof(ngravs_sync_t) == 16,
              "the Python mirror (abi.TimeCols / TimeParams / SyncPoint) assumes this layout");
extern "C" int ngravs_time_tables(const ngravs_time_params_t *par, int32_t rule, double *drift, double *gravkick, double *hydrokick)
{
  return par && drift && gravkick && hydrokick ? time_tables(par, rule, drift, gravkick, hydrokick) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_time_factors(const ngravs_time_params_t *par, int32_t ti0, int32_t ti1, double out[3])
{
  return par && out ? time_factors(par, ti0, ti1, out) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_dt_displacement(const ngravs_time_params_t *par, const double sums[18], double G, double asmth, double time,
                                      double *dt_displacement)
{
  return par && sums && dt_displacement ? time_dt_displacement(par, sums, G, asmth, time, dt_displacement) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_next_sync_point(ngravs_ctx *c, const ngravs_time_cols_t *cols, int32_t pm_ti_endstep, ngravs_sync_t *out)
{
  return c ? time_next_sync_point(c, cols, pm_ti_endstep, out) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_move_particles(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int32_t time0,
                                     int32_t time1, int32_t wrap)
{
  return c ? time_move_particles(c, cols, par, time0, time1, wrap) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_displacement_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, double sums[18])
{
  return c ? time_displacement_sums(c, cols, sums) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_advance_and_find_timesteps(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par,
                                                 int32_t ti_current, double dt_displacement, int32_t *pm_ti, int64_t *n_kicked)
{
  return c ? time_advance(c, cols, par, ti_current, dt_displacement, pm_ti, n_kicked) : NGRAVS_ERR_ARG;
}
static_assert(sizeof(ngravs_sysstate_t) == 952, "struct state_of_system (allvars.h): 119 doubles; the Python mirror is abi.SysState");
extern "C" int ngravs_global_sums(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int32_t ti_current,
                                  const int32_t *pm_ti, const double *potential, int64_t potential_stride, double sums[NGRAVS_GLOBAL_NSUMS])
{
  return c ? time_global_sums(c, cols, par, ti_current, pm_ti, potential, potential_stride, sums) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_global_finish(const double sums[NGRAVS_GLOBAL_NSUMS], ngravs_sysstate_t *out)
{
  return sums && out ? time_global_finish(sums, out) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_energy_line(const ngravs_sysstate_t *s, double time, char *buf, int64_t len)
{
  return s && buf ? time_energy_line(s, time, buf, len) : NGRAVS_ERR_ARG;
}

// ---- snapshot files: savepositions (io.c:33-989) and find_next_outputtime (run.c:244-361); kernels_snapshot.hip ---------------------
static_assert(sizeof(ngravs_snapshot_t) == 112 && sizeof(ngravs_output_rule_t) == 32,
              "the Python mirror (abi.Snapshot / OutputRule) assumes this layout");
extern "C" int ngravs_snapshot_plan(ngravs_ctx *c, const ngravs_time_cols_t *cols, int64_t npart[6])
{
  return c ? snapshot_plan(c, cols, npart) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_snapshot_block_count(ngravs_ctx *c, const ngravs_snapshot_t *snap, int32_t block, int64_t *count, int32_t *bytes_per_element)
{
  return c ? snapshot_block_count(c, snap, block, count, bytes_per_element) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_snapshot_block(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                                     int32_t block, int64_t first, int64_t count, void *out, int32_t out_on_device)
{
  return c ? snapshot_block(c, cols, par, snap, block, first, count, out, out_on_device) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_snapshot_header(const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, const int64_t npart[6],
                                      const int64_t npart_total[6], int32_t num_files, double time, unsigned char out[256])
{
  return par && snap && npart && npart_total && out ? snapshot_header(par, snap, npart, npart_total, num_files, time, out) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_snapshot_write(ngravs_ctx *c, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                                     uint32_t blocks_mask, int32_t snap_format, int64_t buffer_bytes, const char *path)
{
  return c ? snapshot_write(c, cols, par, snap, blocks_mask, snap_format, buffer_bytes, path) : NGRAVS_ERR_ARG;
}
extern "C" int ngravs_find_next_outputtime(const ngravs_time_params_t *par, const ngravs_output_rule_t *rule, int32_t ti_curr, int32_t *ti_next)
{
  return snapshot_next_outputtime(par, rule, ti_curr, ti_next);
}
