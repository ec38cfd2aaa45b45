/* ngravs_hip.h -- C ABI of libngravs_hip.so, the MI355X (gfx950) gravitational force engine for
 * Gadget-2.0.7-ngravs.
 *
 * This is the drop-in boundary for ONE hot path of the reference: everything under
 * compute_accelerations() (accel.c:24-96) that computes gravity, i.e.
 *     domain_Decomposition()  (domain.c:62)      -> ngravs_domain_decomposition()
 *     force_treebuild()       (forcetree.c:61)   -> ngravs_force_treebuild()
 *     gravity_tree()          (gravtree.c:27)    -> ngravs_gravity_tree()
 *     pmforce_periodic()      (pm_periodic.c:204)-> ngravs_pmforce_periodic()
 *     init_grav_maps()/wire_grav_maps() (ngravs_core.c:201, ngravs.c:64) -> ngravs_config_t.law_*
 *     force_treeallocate() short-range tabulation (forcetree.c:3246-3403) -> ngravs_shortrange_table()
 *     gravity_forcetest() direct sum (gravtree_forcetest.c:28, forcetree.c:3428) -> ngravs_direct_sum()
 *
 * Plain C: pointers and sizes only, no torch / HIP types in any signature.  The reference keeps
 * its state in globals (P[], All, TypeToGrav[], AccelFxns[][] ...); the glue a maintainer adds to
 * the reference (gadget-2.0.7-ngravs_amd/host/gadget_glue.c) copies the fields
 * listed in SURVEY.md 8(b) into ngravs_config_t / ngravs_particles_t and calls the functions below
 * from the reference's own entry points, which keep their `void f(void)` signatures.
 *
 * Error convention: every call returns 0 on success or a negative ngravs_status; in addition a
 * fatal condition invokes the registered on_fatal(code, msg) callback first (default: print
 * "endrun called with an error level of C" in the reference's wording and return), mirroring
 * endrun(code) (endrun.c:25-43).  Codes reuse the reference's numbers where one exists
 * (1 = out of tree nodes, forcetree.c:247-253; 986/987 = massive empty node, forcetree.c:1482,1906).
 *
 * Threading: entry points are called serially from one host thread per process; one process per
 * GPU (SURVEY.md 8(b) "Threading").
 */
#ifndef NGRAVS_HIP_H
#define NGRAVS_HIP_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NGRAVS_ABI_VERSION 3
#define NGRAVS_MAX_GRAVS 3      /* N_GRAVS upper bound compiled in (allvars.h:130-152)            */
#define NGRAVS_NTYPES 6         /* Gadget particle types                                           */
#define NGRAVS_NTAB 2048        /* NTAB: short-range table length (Makefile.reference, forcetree.c:33) */
#define NGRAVS_ASMTH 1.25       /* allvars.h:83                                                     */
#define NGRAVS_RCUT 4.5         /* allvars.h:87                                                     */
#define NGRAVS_BITS_PER_DIMENSION 18 /* allvars.h:34: bits of the reference Peano-Hilbert key      */
#define NGRAVS_GROUP_REACH 4.5  /* default ngravs_config_t.group_reach = RCUT (DESIGN.md "Group walk cut")  */
#define NGRAVS_TREE_BITS 21     /* bits/dim of the engine's internal tree key; key21>>9 == key18    */

/* Force-law identifiers: the device cannot call through the reference's `gravity` function
 * pointers (allvars.h:131-150), so each wired pointer is named by an id.  The same id selects the
 * r-space law (AccelFxns), its k-space Green's function (GreensFxns) and the normalised Green's
 * function (NormedGreensFxns) of that law. */
typedef enum {
  NGRAVS_LAW_NONE = 0,        /* none            ngravs.c:344                         */
  NGRAVS_LAW_NEWTON = 1,      /* newtonian :351, pgdelta :390, normed_pgdelta :400    */
  NGRAVS_LAW_NEG_NEWTON = 2,  /* neg_newtonian :357, neg_pgdelta :406                 */
  NGRAVS_LAW_YUKAWA = 3,      /* yukawa :856, pgyukawa :869, normed_pgyukawa :880     */
  NGRAVS_LAW_COLOYUK = 4,     /* coloyuk :826, pgcoloyuk :830, normed_pgcoloyuk :834  */
  /* The BAM family (ngravs.c:495-668, NGRAVS_ACCUMULATOR_TESTING wiring :163-210): laws that depend on the TARGET mass and
   * on the number N of particles of the source species a node holds (allvars.h:645-648).  Tree-only (their Green's functions
   * are `none`); evaluated by both walks and the direct sum. */
  NGRAVS_LAW_BAMBAM = 5,      /* bambam :495             BAM target, BAM source              */
  NGRAVS_LAW_SOURCEBAM = 6,   /* sourcebambaryon :590    baryon target, BAM source            */
  NGRAVS_LAW_TARGETBAM = 7,   /* sourcebaryonbam :646    BAM target, baryon source            */
  NGRAVS_LAW_COUNT
} ngravs_law;

typedef enum {
  NGRAVS_SPLINE_NONE = 0,        /* none                 */
  NGRAVS_SPLINE_PLUMMER = 1,     /* plummer      ngravs.c:420-434 */
  NGRAVS_SPLINE_NEG_PLUMMER = 2, /* neg_plummer  ngravs.c:438-455 */
  NGRAVS_SPLINE_BAMBAM = 3,      /* bambam_spline :531 */
  NGRAVS_SPLINE_SOURCEBAM = 4,   /* sourcebambaryon_spline :562 */
  NGRAVS_SPLINE_TARGETBAM = 5,   /* sourcebaryonbam_spline :616 */
  NGRAVS_SPLINE_COUNT
} ngravs_spline;

/* User-defined laws (ngravs_create_with_laws): entry k of the registry is named NGRAVS_LAW_USER0 + k (accel, greens, normed
 * entries) or NGRAVS_SPLINE_USER0 + k (spline entries) and goes into law_accel / law_spline / law_greens / law_normed like a
 * built-in id. */
#define NGRAVS_LAW_USER0 64
#define NGRAVS_SPLINE_USER0 64
#define NGRAVS_MAX_USER_FNS 8

typedef enum {
  NGRAVS_OK = 0,
  NGRAVS_ERR_ARG = -1,        /* bad argument / unsupported configuration                 */
  NGRAVS_ERR_NO_DEVICE = -2,  /* no HIP device or HIP runtime error                       */
  NGRAVS_ERR_NOMEM = -3,      /* device allocation failed                                 */
  NGRAVS_ERR_STATE = -4,      /* call order violated (e.g. walk before tree build)        */
  NGRAVS_ERR_TREE = -5,       /* tree build failed (out of nodes: reference endrun(1))    */
  NGRAVS_ERR_WIRING = -6      /* law table not wired / asymmetric (ngravs_core.c:321-424) */
} ngravs_status;

/* Walk variants (what gravity_tree() does per particle). */
typedef enum {
  NGRAVS_WALK_STRICT = 0, /* per-target opening decisions, exactly force_treeevaluate[_shortrange]
                             (forcetree.c:1244-1610, 1623-2052): same interaction set and count     */
  NGRAVS_WALK_GROUP = 1   /* wavefront-cooperative walk: 64 Peano-contiguous targets share one
                             breadth-first traversal; a node is used only if EVERY target of the
                             group would use it (conservative => at least the reference accuracy)   */
} ngravs_walk_mode;

/* The subset of `All`, TypeToGrav[] and the law tables the path reads. */
typedef struct {
  int32_t abi_version;        /* NGRAVS_ABI_VERSION                                            */
  int32_t n_gravs;            /* N_GRAVS, 1..NGRAVS_MAX_GRAVS                                   */
  int32_t periodic;           /* PERIODIC                                                       */
  int32_t pmgrid;             /* PMGRID, 0 = tree-only; must be even and >= 0: the in-place real-to-complex mesh is laid
                                 out [N][N][N+2], the transform's padding only for even N -- an odd or negative
                                 value is refused with NGRAVS_ERR_ARG                                           */
  double box_size;            /* All.BoxSize                                                    */
  double G;                   /* All.G                                                          */
  double err_tol_theta;       /* All.ErrTolTheta (0 => relative criterion, gravtree.c:334-335)  */
  double err_tol_force_acc;   /* All.ErrTolForceAcc                                             */
  double force_softening[NGRAVS_NTYPES]; /* All.ForceSoftening[] = 2.8*SofteningTable (gravtree.c:514) */
  int32_t type_to_grav[NGRAVS_NTYPES];   /* TypeToGrav[] (ngravs_core.c:201-260)                */
  /* [TARGET][SOURCE] tables exactly as wire_grav_maps() fills them (ngravs.c:73-76) */
  int32_t law_accel[NGRAVS_MAX_GRAVS][NGRAVS_MAX_GRAVS];    /* AccelFxns        -> ngravs_law    */
  int32_t law_spline[NGRAVS_MAX_GRAVS][NGRAVS_MAX_GRAVS];   /* AccelSplines     -> ngravs_spline */
  int32_t law_greens[NGRAVS_MAX_GRAVS][NGRAVS_MAX_GRAVS];   /* GreensFxns       -> ngravs_law    */
  int32_t law_normed[NGRAVS_MAX_GRAVS][NGRAVS_MAX_GRAVS];   /* NormedGreensFxns -> ngravs_law    */
  double yukawa_imass;        /* YUKAWA_IMASS (ngravs.c:41-43), default 60.0                     */
  double asmth;               /* All.Asmth[0] = ASMTH*BoxSize/PMGRID (pm_periodic.c:59); 0 => derive */
  double rcut;                /* All.Rcut[0]  = RCUT*Asmth (pm_periodic.c:60); 0 => derive       */
  double tree_alloc_factor;   /* All.TreeAllocFactor (nodes per particle), 0 => 0.8              */
  double group_reach;         /* group walk only: radius, in units of Asmth, out to which short-range
                                 forces are evaluated.  0 => NGRAVS_GROUP_REACH.  RCUT (4.5) is the
                                 reference's nominal cut (allvars.h:87), 6.0 the end of its table
                                 (tabindex < NTAB, forcetree.c:1962-1967).  The strict walk ignores it. */
  int32_t walk_mode;          /* ngravs_walk_mode                                                */
  int32_t device;             /* HIP device ordinal                                              */
  int32_t rank, world_size;   /* ThisTask, NTask: target shard = Peano segment `rank` of `world_size` */
  double bam_epsilon;         /* BAM_EPSILON (ngravs.c:45-47); 0 => 1.31e-6                                */
  int32_t reserved[6];
} ngravs_config_t;

/* Host- or device-resident particle columns (the fields of struct particle_data the path reads,
 * allvars.h:546-581).  AoS callers pass strides in BYTES (e.g. stride 144 for P[] built with
 * PMGRID), SoA callers pass sizeof(element).  `on_device` != 0 means the pointers are HIP device
 * pointers (zero-copy hand-over; no PCIe traffic inside the call). */
typedef struct {
  int64_t n;                 /* NumPart; 0 is legal (a task without particles in a multi-task run: pointers may be NULL) */
  const double *pos;         /* Pos[3]          */  int64_t pos_stride;
  const double *mass;        /* Mass            */  int64_t mass_stride;
  const int32_t *type;       /* Type            */  int64_t type_stride;
  const double *old_acc;     /* OldAcc (may be NULL => 0) */ int64_t old_acc_stride;
  const uint8_t *active;     /* NULL => all active; else bit 0 set where Ti_endstep==All.Ti_Current (gravtree.c:113) */
  int64_t active_stride;
  const double *grav_pm;     /* GravPM[3] of the last PM step (may be NULL => none).  P[].GravPM lives in the host's P[] between
                              * PM steps; on non-PM steps OldAcc = |GravAccel + GravPM/G| needs it (gravtree.c:318-330) */
  int64_t grav_pm_stride;
  const float *grav_cost;    /* GravCost of the last walk (may be NULL => 0): the work weight 1 + GravCost of the domain cut
                              * (domain.c:859-862).  A host with individual timesteps passes (1 + GravCost)/(Ti_endstep -
                              * Ti_begstep) - 1 to reproduce the reference's weighting by step frequency. */
  int64_t grav_cost_stride;
  int32_t on_device;
  int32_t reserved;
} ngravs_particles_t;

/* Per-call statistics, the numbers gravity_tree() logs to timings.txt/cpu.txt
 * (gravtree.c:408-447, run.c:394-402). */
typedef struct {
  int64_t n_active;          /* Nf                                                       */
  int64_t n_nodes;           /* Numnodestree                                             */
  double interactions;       /* sum of ninteractions over active targets (ia/part * Nf)  */
  double t_domain, t_peano, t_treebuild, t_treewalk, t_pm; /* seconds, device time       */
  double walk_kernel_ms;     /* all walk kernels of the call (traversal + evaluation), HIP events */
  double reserved[7];        /* group walk, per group: [0] list entries [1] nodes tested [2] traversal batches
                              * [3] force-loop slots; split walk: [4] ms in the evaluation kernel (summed over its
                              * launches) [5] number of launches (batches) [6] ms in the traversal kernel */
} ngravs_stats_t;

typedef struct ngravs_ctx ngravs_ctx;
typedef void (*ngravs_fatal_fn)(int code, const char *msg);

/* A force law of the host: exactly the reference's `gravity` type (allvars.h:134), so that AccelFxns[i][j] etc. pass without
 * casts.  accel: f(target mass, source mass, r^2, r, N); spline: f(target, source, h, r, N), the softened force already divided
 * by r (ngravs.c, the WARNING above plummer); greens / normed: f(target, source, k^2, k, N). */
typedef double (*ngravs_gravity_fn)(double, double, double, double, long);
typedef enum {
  NGRAVS_USER_ACCEL = 0,    /* AccelFxns        */
  NGRAVS_USER_SPLINE = 1,   /* AccelSplines     */
  NGRAVS_USER_GREENS = 2,   /* GreensFxns       */
  NGRAVS_USER_NORMED = 3,   /* NormedGreensFxns */
  /* the two potential tables: for ngravs_user_table_eval only -- a registry refuses them, potentials travel in the
   * ngravs_user_potential_t entries of ngravs_create_with_potentials */
  NGRAVS_USER_POT = 4,        /* PotentialFxns    */
  NGRAVS_USER_POT_SPLINE = 5  /* PotentialSplines */
} ngravs_user_kind;
typedef struct {
  int32_t kind;             /* ngravs_user_kind */
  int32_t reserved;
  ngravs_gravity_fn fn;     /* called on the host only, at creation, in ngravs_set_softening and when a table grows; must
                               stay valid as long as the context */
} ngravs_user_fn_t;
/* A lattice-correction function of the host: exactly the reference's `latforce` type (allvars.h:138), so that
 * LatticeForce[l][m] passes without a cast.  Called as fn(i, j, k, x, force) at x = 0.5 (i, j, k) / 64, i, j, k = 0..64, in
 * units of the box; it writes the force correction of the periodic images into force[3] (force[] is zeroed before every call).
 * The library divides the samples by BoxSize^2, as lattice_init does (forcetree.c:3611-3793).  The function is called
 * concurrently from several host threads (at most 16): 65^3 = 274 625 calls per distinct function, once per context, at the
 * first periodic tree-only walk or periodic direct sum. */
typedef void (*ngravs_lattice_fn)(int i, int j, int k, double x[3], double force[3]);
typedef struct {
  int32_t target, source;   /* the species pair: law_accel[target][source] is a user id */
  ngravs_lattice_fn fn;     /* must stay valid as long as the context */
} ngravs_user_lattice_t;
/* The potential companions of one species pair, the reference's PotentialFxns, PotentialSplines, LatticePotential and LatticeZero
 * [target][source] (allvars.h:134-149; ngravs.c:132-150 wires newtonian_pot, plummer_pot, ewald_psi and 2.8372975).  pot and
 * pot_spline are evaluated at unit masses and N = 1 and scaled by the source mass; pot is tabulated over r alone, with 0 in the
 * place of h (as pm_nonperiodic.c:564 calls it), and must not depend on it.  lattice_pot is the reference's `latpot`
 * (allvars.h:139): called at x = 0.5 (i, j, k) / 64 in box units, every point of the octant grid but the origin, whose value is
 * lattice_zero; the library divides both by BoxSize (forcetree.c:3699-3702).  It is called concurrently from at most 16 host
 * threads, 65^3 - 1 calls per distinct function, at the first periodic tree-only potential call.  All functions must stay valid
 * as long as the context. */
typedef double (*ngravs_lattice_pot_fn)(double x[3]);
typedef struct {
  int32_t target, source;            /* the species pair [target][source]: law_accel of the pair is not NONE            */
  ngravs_gravity_fn pot;             /* PotentialFxns:    f(target mass, source mass, h, r, N); newtonian_pot = +source / r */
  ngravs_gravity_fn pot_spline;      /* PotentialSplines: f(target, source, h, r, N) for r < h; plummer_pot               */
  ngravs_lattice_pot_fn lattice_pot; /* LatticePotential; NULL where not needed (not periodic, or with a mesh)            */
  double lattice_zero;               /* LatticeZero                                                                      */
} ngravs_user_potential_t;
/* Which kernel the last ngravs_gravity_tree() walked with (ngravs_last_walk_kernel) */
typedef enum {
  NGRAVS_KERNEL_NONE = 0,
  NGRAVS_KERNEL_STRICT = 1,        /* k_walk_strict, built-in laws                                  */
  NGRAVS_KERNEL_STRICT_USER = 2,   /* k_walk_strict with the user-law tables                       */
  NGRAVS_KERNEL_GROUP = 3,         /* the group walk, built-in laws                                 */
  NGRAVS_KERNEL_GROUP_USER = 4,    /* the group walk with user laws: the law-id variant (tree-only) or k_walk_group2<..., USR> (TreePM) */
  NGRAVS_KERNEL_STRICT_ADAPTIVE = 5, /* k_walk_strict with per-particle gas softening (ngravs_set_gas_softening)   */
  NGRAVS_KERNEL_GROUP_ADAPTIVE = 6   /* the group walk with per-particle gas softening: k_walk_group2<..., ADA>    */
} ngravs_walk_kernel_id;

/* ---- lifecycle ------------------------------------------------------------------------- */
int ngravs_abi_version(void);
const char *ngravs_build_info(void);                    /* arch, N_GRAVS instantiations, NTAB ... */
void ngravs_config_default(ngravs_config_t *cfg);       /* N_GRAVS=1 Newton/plummer, tree-only    */
/* init_grav_maps()+wire_grav_maps() checks (ngravs_core.c:321-424) happen here. */
int ngravs_create(const ngravs_config_t *cfg, ngravs_ctx **out);
/* ngravs_create with a registry of nfns <= NGRAVS_MAX_USER_FNS host laws (ngravs_create is this with an empty one).  The laws
 * are sampled on the host into tables the kernels evaluate (DESIGN.md "User-defined force laws").  Refused with
 * NGRAVS_ERR_WIRING and a message in ngravs_last_error(NULL): a user id outside the registry or of the wrong kind for its
 * table; a pair that fails the reference's Newton's-third-law probe F[i][j](1,1,0.5,3,1) == F[j][i](...); an accel or spline
 * law that is not linear in the source mass or depends on the target mass or N (a tree node's monopole is a mass sum); a
 * Green's function that depends on its mass arguments; a user accel id in a periodic tree-only run (its lattice correction
 * needs the model's own tables: ngravs_create_with_lattice).  ngravs_last_error(NULL) is per thread. */
int ngravs_create_with_laws(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, ngravs_ctx **out);
/* ngravs_create_with_laws with the model's own lattice corrections, one entry per species pair wired with a user accel id
 * (the reference's LatticeForce[l][m]); ngravs_create_with_laws is this with nlat = 0.  A periodic tree-only run needs an entry
 * for every user-accel pair; in a TreePM run the entries are optional, and the periodic direct sum (ngravs_direct_sum[_targets])
 * needs them all.  Refused with NGRAVS_ERR_WIRING, without GPU work: an entry whose pair is out of range or that has no
 * function; two entries for one pair; an entry on a pair whose law_accel is not a user id; any entry in a non-periodic
 * configuration.  The tables are sampled lazily (see ngravs_lattice_fn); a non-finite sample fails that call with
 * NGRAVS_ERR_WIRING and names the pair and the point. */
int ngravs_create_with_lattice(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, const ngravs_user_lattice_t *lat,
                               int nlat, ngravs_ctx **out);
/* ngravs_create_with_lattice with the model's own potential companions, at most one entry per species pair;
 * ngravs_create_with_lattice is this with npot = 0.  A pair without an entry behaves as before: Newton / neg-Newton with the
 * Plummer splines have the built-in companions, every other law has none.  An entry may sit on any pair whose law_accel is not
 * NONE, built in (Yukawa, coloyuk; Newton too, whose built-in companion it then replaces) or a user id; the BAM laws stay
 * refused by the potential calls (their potentials depend on the target mass and on N, which a node's monopole cannot carry
 * through a table that is linear in the source mass).  ngravs_compute_potential and ngravs_potential_targets serve a context in
 * which every wired pair has a built-in companion or an entry.  The functions are sampled lazily into tables like the force
 * laws (degree-7 pieces; p(r) = r pot(1, 1, 0, r, 1) over the octaves of r, pot_spline(1, 1, h, u h, 1) over u in [0, 1) for
 * every distinct softening length; distinct function pointers once); they are rebuilt when ngravs_set_softening changes a length
 * or the walk's largest r outgrows them, and a law whose fit is not within 1e-9 fails that call with NGRAVS_ERR_WIRING.
 * Refused at creation with NGRAVS_ERR_WIRING, without GPU work and with nothing created: an entry out of range; two entries for
 * one pair; an entry on a pair wired NONE; an entry without pot or pot_spline; pot[i][j](1,1,0.5,3,1) != pot[j][i](...) and the
 * same for the splines (ngravs_core.c:408-413); lattice_pot pointers or lattice_zero that differ between [i][j] and [j][i]
 * (ngravs_core.c:389); a pot or pot_spline that is not linear in the source mass or depends on the target mass or on N, or a pot
 * that depends on h; a periodic tree-only configuration with an entry that has no lattice_pot; a lattice_pot in a configuration
 * that is not periodic.  With a mesh lattice_pot is optional and unused; lattice_zero is read by the tail in every periodic run. */
int ngravs_create_with_potentials(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, const ngravs_user_lattice_t *lat,
                                  int nlat, const ngravs_user_potential_t *pots, int npot, ngravs_ctx **out);
/* NGRAVS_KERNEL_* of the last walk of the context (0 before the first) */
int ngravs_last_walk_kernel(ngravs_ctx *ctx);
/* CUs reserved for PM beside the walk in the last ngravs_compute_accelerations (0: PM and walk ran one after another) */
int ngravs_last_pm_cus(ngravs_ctx *ctx);
/* Where workgroups launched on a stream of the context run: which = 0 its stream, 1 the PM stream, 2 the walk stream of the
 * overlapped step (NGRAVS_ERR_STATE before an overlapped step created them).  Writes one id per workgroup, nblocks of them:
 * XCC << 8 | bits 8-15 of the CU's hardware id. */
int ngravs_cu_probe(ngravs_ctx *ctx, int which, int nblocks, int32_t *cu_ids);
void ngravs_destroy(ngravs_ctx *ctx);
void ngravs_set_fatal_handler(ngravs_ctx *ctx, ngravs_fatal_fn fn);
/* Change the walk parameters between calls (All.ErrTolTheta latch, gravtree.c:334-335). */
int ngravs_set_opening(ngravs_ctx *ctx, double err_tol_theta, double err_tol_force_acc);
int ngravs_set_walk_mode(ngravs_ctx *ctx, int walk_mode);
/* New All.ForceSoftening[6] (= 2.8 * All.SofteningTable[]): set_softenings() (gravtree.c:468-518) recomputes it from the scale
 * factor at the top of every gravity_tree() of a comoving run (gravtree.c:50-51); the glue's set_softenings() forwards it here.
 * Takes effect from the next walk / direct sum / import decision on. */
int ngravs_set_softening(ngravs_ctx *ctx, const double force_softening[NGRAVS_NTYPES]);
/* the configuration the context was created with (opening parameters as last set) */
int ngravs_get_config(ngravs_ctx *ctx, ngravs_config_t *out);
/* Performance / test parameters of the engine, by name (none changes WHAT is computed beyond rounding; there is no
 * environment variable and no way to make the library skip work):
 *   "walk_fused" 1: one fused traversal+evaluation kernel instead of the pair     "walk_batch" n: groups per launch pair
 *   "walk_waves" n: waves per evaluation workgroup (<= 16)                         "walk_lcap" n: initial item-list capacity (>= 1024)
 *   "walk_root" 1: TreePM group walks start at the root, not at the start table   "walk_compact" 0: do not compact sparse active sets
 *   "walk_spread" S: lanes per target for compacted active sets (1..64, 0 = auto)  "walk_exact_reach" 1: fp64 reach test, no fp32 pre-test
 *   "walk_sg" n: groups of 64 targets per traversal unit = per shared item list (0 = auto: with TreePM 4, or 2 / 1 when the last walk evaluated more than 1.4 / 2 x the pairs per target of a uniform box -- a clustered set; else 1)
 *   "walk_nleaf" k: an opened node with <= k particles hands its particles over instead of its children (0..8, -1 = default 8)
 *   "tree_levelwise" 1: level-by-level tree build for single-task trees too
 *   "sort_full" 1: Peano order by one radix sort on all key bits (default: top 28 to 42 bits + fix-up of the ties, the same order)
 *   "dd_keep" f: decompositions are kept over several steps (ngravs_host_kept_step): leaves are imported for ALL own particles as
 *       targets, whose cells may have grown by f x the domain's side (0 <= f <= 0.25; default 0: import for this step's active targets)
 *   "walk_tg_sort" 0: ngravs_gravity_tree_targets walks its targets in the caller's order, not along the Peano curve (same results)
 *   "sph_verbose" 1: the SPH density call prints one line of iteration statistics (targets, rounds, candidates, neighbours) to stdout,
 *       the SPH hydro call one line (targets, candidates tested, pairs evaluated)
 * Returns NGRAVS_ERR_ARG for an unknown name or a value out of range. */
int ngravs_set_tuning(ngravs_ctx *ctx, const char *name, double value);
/* Plain copies for hosts that do not link HIP themselves (a C/MPI host staging exchange buffers through host memory):
 * kind 1 = host->device, 2 = device->host, 3 = device->device.  Synchronous. */
int ngravs_memcpy(ngravs_ctx *ctx, void *dst, const void *src, int64_t bytes, int kind);
/* ... and device memory for such a host's own exchange buffers (hipMalloc / hipFree on the context's device) */
int ngravs_device_alloc(ngravs_ctx *ctx, void **ptr, int64_t bytes);
int ngravs_device_free(ngravs_ctx *ctx, void *ptr);

/* ---- data hand-over ---------------------------------------------------------------------- */
/* Replace the engine's particle set (the role of P[] + NumPart).  PERIODIC runs: positions must lie in [0, BoxSize], as they do
 * in the reference after do_box_wrapping() (domain.c:81); the next decomposition fails with NGRAVS_ERR_ARG otherwise. */
int ngravs_set_particles(ngravs_ctx *ctx, const ngravs_particles_t *p);
/* Drifted tree (TreeDomainUpdateFrequency > 0: domain.c:76, predict.c:79-91): the same particles (same n, same order
 * in the caller's arrays) with new positions / OldAcc / active flags.  Keeps the last decomposition and tree topology;
 * the sorted columns and the nodes are refreshed by ngravs_force_update_tree(), which ngravs_gravity_tree() and
 * ngravs_pmforce_periodic() call by themselves when needed.  NGRAVS_ERR_STATE without a built tree. */
int ngravs_update_particles(ngravs_ctx *ctx, const ngravs_particles_t *p);
/* Update OldAcc only (second pass of accel.c:48-52 without re-uploading positions): the caller's OWN rows (NumPart =
 * ngravs_dd_num_local() of them; the imported copies of a multi-task working set are sources only and keep what they came with). */
int ngravs_set_old_acc(ngravs_ctx *ctx, const double *old_acc, int64_t stride, int on_device);
/* Adaptive gravitational softening for gas (the reference's ADAPTIVE_GRAVSOFT_FORGAS): hsml addresses one length per OWN row in
 * the caller's order (stride in bytes); rows that are not type 0 are never read.  From the next walk or direct sum on a type-0
 * particle's softening length is its hsml value instead of force_softening[0]; a pair is softened with the larger of its two
 * lengths, and a node is opened by the largest length below it (forcetree.c:1398-1413, :1503-1516).  hsml = NULL switches back to
 * the lengths per type.  ngravs_update_particles() keeps the column, ngravs_set_particles() drops it; the call may come before
 * or after the tree build.  Refused, with nothing changed: NGRAVS_ERR_ARG before particles were handed over, for a type-0 row
 * whose value is negative or not finite, and for a context with user-defined laws (their spline tables are sampled per softening
 * length); NGRAVS_ERR_STATE "single task only" with world_size > 1 or a multi-task working set.  While it is on,
 * ngravs_direct_sum_targets() returns NGRAVS_ERR_STATE (explicit targets carry no length), and ngravs_gravity_tree() returns
 * NGRAVS_ERR_ARG for a group-walk configuration that has no adaptive kernel (NGRAVS_WALK_STRICT serves every one). */
int ngravs_set_gas_softening(ngravs_ctx *ctx, const double *hsml, int64_t stride, int on_device);

/* ---- the path ---------------------------------------------------------------------------- */
/* domain_findExtent + keys + Peano-Hilbert order (domain.c:882-944, peano.c:36-185).  Computes
 * DomainCorner/Center/Len/Fac, the 18-bit reference keys and the device-side Peano order. */
int ngravs_domain_decomposition(ngravs_ctx *ctx);
/* Tell the library that the coming step is a PM step: the stored GravPM will be recomputed before anything reads it, so it need
 * not be carried through the decomposition (ngravs_compute_accelerations(ctx, 1) does this by itself; a multi-task host that
 * calls the decomposition and the PM force separately saves two passes over the particles) */
int ngravs_discard_grav_pm(ngravs_ctx *ctx);
/* force_treebuild(): returns the number of tree nodes (>0) or a negative status. */
int64_t ngravs_force_treebuild(ngravs_ctx *ctx);
/* The dynamic tree update between rebuilds (predict.c:79-91 node drift + force_update_len(), forcetree.c:1005-1122,
 * and the node kicks of timestep.c:331-344), done as a refit: every node's per-species mass and centre of mass are
 * recomputed bottom-up from the current particle positions (exact, where the reference extrapolates them with node
 * velocities; for N_GRAVS > 1 the reference's kick of a node adds a particle's dv to the node velocities of every species,
 * timestep.c:337-340 -- the refit does not follow that), softening flags likewise, and a cell's side grows to
 * enclose what its particles now reach. */
int ngravs_force_update_tree(ngravs_ctx *ctx);
/* gravity_tree(): walk for all active targets, OldAcc update, xG (gravtree.c:102-341). */
int ngravs_gravity_tree(ngravs_ctx *ctx);
/* pmforce_periodic(): GravPM for all particles (pm_periodic.c:204-790). */
int ngravs_pmforce_periodic(ngravs_ctx *ctx);
/* compute_accelerations(0) for gravity: [PM if pm_step] + domain + build + tree (accel.c:24-58). */
int ngravs_compute_accelerations(ngravs_ctx *ctx, int pm_step);

/* ---- results, in the caller's ORIGINAL particle order -------------------------------------- */
/* Any pointer may be NULL.  stride in bytes as above.  grav_cost = ninteractions (gravtree.c).
 * Rows: exactly the caller's own particles, i.e. the n rows of the last ngravs_set_particles() (ngravs_dd_num_local() rows after
 * a library-side migration) -- the copies of other tasks' particles a multi-task step imports are never delivered, so an array
 * of NumPart rows is enough (ABI 3; ABI 2 wrote NumPart + imported rows).
 * only_active != 0: GravAccel / OldAcc / GravCost are written ONLY for the rows the last hand-over marked active, as the
 * reference does (gravtree.c:318-341 touch only Ti_endstep == Ti_Current) -- inactive rows of the caller's arrays keep
 * their values.  only_active == 0: every row is written; rows that were not walked read GravAccel = 0, GravCost = 0 and
 * their input OldAcc.  GravPM is written for all rows either way (pm_periodic.c:716-763 updates every particle). */
int ngravs_get_accel(ngravs_ctx *ctx, double *grav_accel, int64_t accel_stride,
                     double *grav_pm, int64_t pm_stride, double *old_acc, int64_t old_acc_stride,
                     float *grav_cost, int64_t cost_stride, int on_device, int only_active);
int ngravs_get_stats(ngravs_ctx *ctx, ngravs_stats_t *out);
/* Multi-task trees: top-tree leaves the last GROUP walk wanted to open although their particles were not imported (the box of a
 * group that spans several top leaves can come closer to a node than any of the leaves' boxes the import decision tested, or the
 * host changed the opening criterion after the decomposition).  Such a leaf is used as a monopole and counted here (0 in a single
 * task).  The reference walk (NGRAVS_WALK_STRICT) does not substitute: ngravs_gravity_tree() returns NGRAVS_ERR_STATE instead.
 * Replaces nothing in the reference: its export / import loop (gravtree.c:112-285) follows the walk wherever it goes. */
int ngravs_walk_unopened(ngravs_ctx *ctx, int64_t *count);
/* Group walk (NGRAVS_WALK_GROUP), diagnostics of the last walk's traversal: how many tested nodes were opened from the node head
 * alone, their multipole moments never fetched (*skips), out of how many nodes within reach of their group of targets
 * (*within_reach, may be NULL).  Both 0 when the walk ran without the head: tuning "walk_head" 0, a refit tree, a multi-task tree,
 * a tree-only walk.
 * Replaces nothing in the reference. */
int ngravs_walk_moment_skips(ngravs_ctx *ctx, int64_t *skips, int64_t *within_reach);
/* DomainCorner[3], DomainCenter[3], DomainLen, DomainFac (domain.c:916-923) -> out[8] */
int ngravs_get_domain(ngravs_ctx *ctx, double out[8]);
/* 18-bit reference Peano-Hilbert keys in original particle order (domain.c:938-944). */
int ngravs_get_keys(ngravs_ctx *ctx, int64_t *keys, int on_device);
/* Device-side Peano order: order[i] = original index of the i-th particle along the curve. */
int ngravs_get_order(ngravs_ctx *ctx, int32_t *order, int on_device);
/* Target shard of this rank: positions [first, first+count) of the Peano order (the role of
 * DomainMyStart/DomainMyLast, domain.c:347-456).  Results outside the shard are zero. */
int ngravs_get_shard(ngravs_ctx *ctx, int64_t *first, int64_t *count);
/* Text of the last error reported through the fatal handler. */
const char *ngravs_last_error(ngravs_ctx *ctx);

/* ---- stand-alone pieces of the path ------------------------------------------------------- */
/* peano_hilbert_key(x,y,z,bits) (peano.c:356-398), host. */
int64_t ngravs_peano_hilbert_key(int x, int y, int z, int bits);
/* Keys for n positions on the device given corner/fac (domain.c:938-944); host buffers. */
int ngravs_peano_keys(ngravs_ctx *ctx, const double *pos, int64_t n, const double corner[3],
                      double fac, int bits, int64_t *keys);
/* shortrange_fourier_force[target][source][NTAB] (forcetree.c:3246-3403): out has
 * n_gravs*n_gravs*NTAB doubles; pot_out (may be NULL) the matching shortrange_fourier_pot. */
int ngravs_shortrange_table(const ngravs_config_t *cfg, double *force_out, double *pot_out);
/* The same with a registry of user laws: a user id in law_normed calls its NORMED callback.  No GPU needed. */
int ngravs_shortrange_table_with_laws(const ngravs_config_t *cfg, const ngravs_user_fn_t *fns, int nfns, double *force_out,
                                      double *pot_out);
/* The tables the kernels evaluate for one user law, built and evaluated on the host (no GPU): kind NGRAVS_USER_ACCEL tabulates
 * fn over r in [r_lo, r_hi] and returns accel(1, 1, r^2, r, 1) from the table at the n radii r[]; NGRAVS_USER_SPLINE tabulates
 * fn for softening h and returns spline(1, 1, h, r, 1) from the table (0 <= r < h).  NGRAVS_USER_POT and
 * NGRAVS_USER_POT_SPLINE do the same for the two potential functions of an ngravs_user_potential_t: pot(1, 1, 0, r, 1) over
 * [r_lo, r_hi] and pot_spline(1, 1, h, r, 1).  *max_err (may be NULL): the largest relative deviation from the callback the
 * fit saw at its check points. */
int ngravs_user_table_eval(const ngravs_user_fn_t *fn, double r_lo, double r_hi, double h, const double *r, int64_t n, double *out,
                           double *max_err);
/* One lattice-correction table as the kernels read it, built on the host (no GPU): out[3][65^3] (x, y, z; point (i, j, k) at
 * (i * 65 + j) * 65 + k) = fn's samples at x = 0.5 (i, j, k) / 64 divided by box_size^2.  NGRAVS_ERR_WIRING (message in
 * ngravs_last_error(NULL)) if a sample is not finite. */
int ngravs_user_lattice_table(ngravs_lattice_fn fn, double box_size, double *out);
/* force_treeevaluate_direct for targets idx[0..nt) against all particles; with PERIODIC the nearest-image
 * sum plus lattice_corr (Ewald / lattice-sum tables, forcetree.c:3515-3529, 3803-3885), i.e. the truth
 * gravity_forcetest() compares the tree / TreePM force against; result xG into acc[3*nt]. */
int ngravs_direct_sum(ngravs_ctx *ctx, const int32_t *idx, int64_t nt, double *acc);
/* The same truth with several tasks (gravity_forcetest's export of the test particles, gravtree_forcetest.c:100-260): the direct
 * sum for nt EXPLICIT targets (position, mass -- only the BAM laws read it, may be NULL --, type; host arrays) over the particles
 * this task OWNS (not its imported copies).  Every task calls it with the test particles of ALL tasks and the host adds the
 * partial sums up (MPI_Allreduce / ncclAllReduce).  xG, lattice correction included when PERIODIC. */
int ngravs_direct_sum_targets(ngravs_ctx *ctx, const double *pos, const double *mass, const int32_t *type, int64_t nt, double *acc);

/* ---- gravity for targets that are not the engine's own particles ----------------------------------------
 * The reference walks its tree for particles imported from other tasks (force_treeevaluate(j, 1), force_treeevaluate_shortrange(j, 1),
 * force_treeevaluate_lattice_correction(j, 1), gravtree.c:133-285): a target is given by value -- position, type,
 * OldAcc and mass (forcetree.c:1299-1313, :1683-1695) -- and need not be a particle of the tree.  The same here for one task: test
 * particles, tracers, map pixels, or the particles of another engine (the force on a set split over engines is the sum of every
 * engine's force at the targets).  The targets are no sources, the tree, the engine's own accelerations, costs and walk statistics
 * are not modified: ngravs_get_accel() returns afterwards what it returned before. */
typedef struct
{
  const double *pos;
  int64_t pos_stride;          /* 3 doubles per target; strides in bytes                                */
  const int32_t *type;
  int64_t type_stride;         /* 0..5                                                                  */
  const double *old_acc;
  int64_t old_acc_stride;      /* P[].OldAcc of the target; may be NULL: 0 for every target             */
  const double *mass;
  int64_t mass_stride;         /* may be NULL: 1.0; only the BAM laws read it (ngravs.c:495-668)        */
  int32_t on_device;           /* all pointers, results included, are device pointers (else host)       */
} ngravs_grav_targets_t;
/* The strict walk (the reference's semantics per target, whatever walk mode the engine is in) of the built tree for nt targets in
 * any order: every node the target's own criterion accepts is used, every opened node is followed, counts as
 * forcetree.c:1244-1610 / :1623-2052 / :2077-2455.  TreePM configurations give the short-range force, periodic tree-only ones add
 * the lattice-correction walk.  The criterion is the context's current one (ngravs_set_opening): Barnes-Hut when err_tol_theta != 0,
 * else the relative criterion with the target's old_acc -- with old_acc = 0 it opens every node that has mass.  A source at the
 * target's position contributes no force and counts as an interaction.  acc[3*nt] xG and nint[nt] (may be NULL), contiguous, in
 * the caller's order; kernel_ms (may be NULL): device time of ordering the targets along the Peano curve and walking them.
 * NGRAVS_ERR_ARG for a NULL ctx.  Refused with a message in ngravs_last_error() and nothing written: NGRAVS_ERR_ARG for a NULL
 * targets, pos, type or acc, nt < 0, a type outside 0..5, a position that is not finite or, in a periodic configuration, has a
 * coordinate outside [0, BoxSize] (elsewhere any finite position is served, also outside the domain cube); NGRAVS_ERR_STATE "single
 * task only" with world_size > 1 or a multi-task working set (the reference's short-cuts for top-level nodes, forcetree.c:1424-1434,
 * :1522-1526, are not implemented), with adaptive gas softening on (as ngravs_direct_sum_targets), and without a built tree of the
 * current particle set (after ngravs_update_particles the tree is refit first).  nt = 0 is NGRAVS_OK. */
int ngravs_gravity_tree_targets(ngravs_ctx *ctx, const ngravs_grav_targets_t *targets, int64_t nt, double *acc, int32_t *nint,
                                double *kernel_ms);
/* GravPM at nt targets: the 4-point gradient and CIC read-back (pm_periodic.c:681-763) of the potential meshes the last
 * ngravs_pmforce_periodic() of this task left, each target reading the mesh of its species; grav_pm[3*nt], G included, exactly as
 * GravPM is delivered.  old_acc and mass are not read.  The mesh stays valid across steps without PM, as P[].GravPM does, until the
 * next PM step rewrites it.  Refusals as above; NGRAVS_ERR_STATE also for PMGRID = 0 and without a valid mesh (no PM step yet, or
 * the last one ran over the slab-decomposed mesh). */
int ngravs_pm_targets(ngravs_ctx *ctx, const ngravs_grav_targets_t *targets, int64_t nt, double *grav_pm);

/* ---- multi-task domain decomposition ------------------------------------------------------------------
 * The role of domain_decompose()/domain_exchangeParticles() (domain.c:164-330, 554-760) and of the target export of
 * gravity_tree() (gravtree.c:112-285).  The Peano curve is cut at the leaves of an adaptive TOP TREE in key space (the
 * reference's TopNodes[], domain.c:933-1138: a cell is split while it holds more than a threshold of particles); a task owns a
 * run of leaves, holds its own particles plus copies of the particles of every foreign leaf one of its targets may open, and
 * then needs no communication for tree build and walk.  The library packs/unpacks; the HOST performs the collectives (RCCL /
 * MPI behind the vtable of ngravs_host.h, where this sequence lives as plain C):
 *   lo,hi   = ngravs_dd_local_extent()                 -> all-reduce min/max -> ngravs_dd_set_extent()
 *   ngravs_dd_set_toptree(child[])  the current top tree (every task the same)
 *   sums    = ngravs_dd_leaf_sums()                    -> all-reduce sum (device or host) -> host adapts the tree, cuts the curve
 *   records = ngravs_dd_pack(0, leaf_owner, ...)       -> all-to-all-v          -> ngravs_dd_apply_migration()
 *   records = ngravs_dd_pack_leaves(reqmask, ...)      -> all-to-all-v          -> ngravs_dd_set_halo()
 *   ngravs_dd_set_top(node sums, present leaves); ngravs_domain_decomposition(); slab PM (below); ngravs_gravity_tree();
 *   results: ngravs_get_accel() (own rows), ids from ngravs_dd_get_ids().
 * Records are 56 bytes (NGRAVS_DD_RECORD_BYTES): x,y,z,mass,old_acc,grav_cost (f64), meta (i64: type | active<<8 | id<<16).  world_size <= 64. */
#define NGRAVS_DD_RECORD_BYTES 56
#define NGRAVS_DD_MAX_RECORD_BYTES 80
/* bytes per record of ngravs_dd_pack(what, ...): what = 0 (migration) of a TreePM run appends P[].GravPM[3] (the particle's
 * long-range force of the last PM step travels with it, as the whole particle_data does in domain_exchangeParticles,
 * domain.c:695-795; OldAcc on non-PM steps needs it, gravtree.c:318-330): 80 bytes; everything else NGRAVS_DD_RECORD_BYTES */
int64_t ngravs_dd_record_bytes(ngravs_ctx *ctx, int what);
int64_t ngravs_dd_num_local(ngravs_ctx *ctx);
int ngravs_dd_local_extent(ngravs_ctx *ctx, double lo[3], double hi[3]);             /* domain.c:894-905 */
/* peano_hilbert_order() of P[] (domain.c:146, peano.c:36-90, reorder_particles :261-312) for the library's OWN copy of the
 * columns: the rows of the own particles are put into the Peano order of the last local decomposition, so that the passes that
 * visit particles in tree order (per-leaf sums, keys, gather, result scatter) read memory in order.  Only for callers that name
 * rows by ID (ngravs_dd_get_ids) -- the host layer's whole-decomposition driver (ngravs_host.h) calls it; a host that owns the row order (gadget_glue.c:
 * P[] is the reference's, already in this order) never does.  force = 0: only when more than 1 in 8 reads of the last gather
 * left its neighbourhood (64 rows).  Call it at the start of a step: imported copies, order, tree and results of the last
 * step are gone afterwards.  Returns 1 if rows moved, 0 if they were left, < 0: status. */
int ngravs_dd_peano_order(ngravs_ctx *ctx, int force);
int ngravs_dd_set_extent(ngravs_ctx *ctx, const double lo[3], const double hi[3]);   /* result of domain.c:906-907 */
/* DomainCorner[3], DomainCenter[3], DomainLen, DomainFac as set by ngravs_dd_set_extent (before the local Peano order exists) */
int ngravs_get_domain_extent(ngravs_ctx *ctx, double out[8]);
/* The top tree as its child table: child[t] = index of the first of the 8 consecutive children (key order) of node t, or -1 for a
 * leaf; node 0 = the root.  The library numbers the leaves in depth-first (= curve) order.  It keeps the table between steps
 * (ngravs_dd_get_toptree: *child points into the context, valid until the next set; nnode 0: none yet). */
int ngravs_dd_set_toptree(ngravs_ctx *ctx, int32_t nnode, const int32_t *child);
int ngravs_dd_get_toptree(ngravs_ctx *ctx, int32_t *nnode, const int32_t **child);
/* Per top LEAF, curve order, NGRAVS_TOP_CW(n_gravs) doubles: [0] the work sum(1 + GravCost) (domain_sumCost, domain.c:859-862),
 * [1..6] particles per type, then per species mass and mass-weighted position (the local part of DomainMoment[],
 * forcetree.c:766-850) -- of the own particles.  DEVICE buffer owned by the library (valid until the next call);
 * *count = nleaf * NGRAVS_TOP_CW doubles.  The host all-reduces it (in place on the device if it can) and reads it back. */
#define NGRAVS_TOP_CW(ng) (7 + 4 * (ng))
int ngravs_dd_leaf_sums(ngravs_ctx *ctx, void **dev_sums, int64_t *count);
/* min over the own active particles of ErrTolForceAcc * OldAcc and of the softening length: out[2].  With the tuning "dd_keep" > 0
 * (a decomposition that will be kept over steps with other active sets, All.TreeDomainUpdateFrequency > 0): over ALL own particles */
int ngravs_dd_target_bounds(ngravs_ctx *ctx, double out[2]);
/* "dd_keep" x the side of the domain cube: how far the import decision lets a target drift out of its top leaf's cell while the
 * decomposition is kept (0: the decomposition serves this step only) */
int ngravs_dd_keep_margin(ngravs_ctx *ctx, double *margin);
/* what = 0: the records of the own particles whose leaf belongs to another task (leaf_owner[leaf], host array), grouped by
 * destination; counts[r] records go to task r */
int ngravs_dd_pack(ngravs_ctx *ctx, int what, const int32_t *leaf_owner, int nranks, int my_rank, int64_t *counts, void **dev_records,
                   int64_t *nrec);
/* destination task of every local particle under the owner map (its own rank if it stays), host array of ngravs_dd_num_local() ints */
int ngravs_dd_get_dest(ngravs_ctx *ctx, const int32_t *leaf_owner, int32_t *dest);
/* ---- the global top of the tree: top-leaf moments and tree-node import (force_exchange_pseudodata / force_treeupdate_pseudos,
 * forcetree.c:766-996; replaces the target export / partial-force import of gravtree.c:112-285) ---------------------------------
 * The host decides which foreign leaves the task's targets may have to open (ngravs_host_import_request: the walk's own opening
 * tests against the task's domain), the owners ship ALL particles of the requested leaves (ngravs_dd_pack_leaves: reqmask[leaf]
 * bit r = task r asked for it), and ngravs_dd_set_top() hands the global sums of every top node over: the next tree build
 * forces the topology of the top tree from the global counts -- it is the single-task tree's --, gives the top nodes global
 * monopoles, and turns every leaf whose particles are elsewhere into a pseudo node.  Forces are then independent of the
 * number of tasks (domain.c:18-21). */
int ngravs_dd_pack_leaves(ngravs_ctx *ctx, const uint64_t *reqmask, int nranks, int my_rank, int64_t *counts, void **dev_records,
                          int64_t *nrec);
/* node_sums: NGRAVS_TOP_CW doubles per top NODE ([0] = global particle count); present[leaf] != 0: the leaf's particles are on
 * this task (own or imported).  NULL, NULL: single-task trees again. */
int ngravs_dd_set_top(ngravs_ctx *ctx, const double *node_sums, const uint8_t *present);
/* a library-owned device buffer for nrec incoming records (valid until the next ngravs_dd_recv_buffer call) */
int ngravs_dd_recv_buffer(ngravs_ctx *ctx, int64_t nrec, void **dev_records);
int ngravs_dd_apply_migration(ngravs_ctx *ctx, const void *dev_records, int64_t nrec);
int ngravs_dd_set_halo(ngravs_ctx *ctx, const void *dev_records, int64_t nrec);
/* ---- kept decomposition: the steps on which domain.c:76 keeps domain and tree (All.TreeDomainUpdateFrequency > 0) -------------
 * The reference drifts its nodes with their velocities, refreshes the other tasks' top-leaf moments (force_update_pseudoparticles,
 * forcetree.c:753) and the sides of the top nodes (force_update_node_len_toptree, :1096-1122), and goes on exporting targets.  Here
 * the cut, the top tree and the import requests of the last decomposition stay; the caller hands its own rows over again
 * (ngravs_update_particles: same rows, drifted positions) and ngravs_host_kept_step in ngravs_host.h does the rest with two
 * collectives: the owners ship the drifted particles of the leaves that were asked for at the decomposition -- the same records in
 * the same order (ngravs_dd_pack_leaves_kept -> all-to-all-v -> ngravs_dd_refresh_halo); the tree is refit
 * (ngravs_force_update_tree); the per-leaf sums BY THE MEMBERSHIP OF THE DECOMPOSITION plus the grown side of every leaf's cell in
 * its owner's tree are all-reduced (ngravs_dd_leaf_sums_kept: NGRAVS_TOP_CW + 1 doubles per leaf) and set
 * (ngravs_dd_update_top: node sums as for ngravs_dd_set_top, one side per leaf).  The refit tree is then the single task's refit
 * tree wherever this task's targets look.  NGRAVS_ERR_STATE without a kept decomposition (none yet, rows changed, single task). */
int ngravs_dd_leaf_sums_kept(ngravs_ctx *ctx, void **dev_sums, int64_t *count);
int ngravs_dd_pack_leaves_kept(ngravs_ctx *ctx, int64_t *counts, void **dev_records, int64_t *nrec);
int ngravs_dd_refresh_halo(ngravs_ctx *ctx, const void *dev_records, int64_t nrec);
int ngravs_dd_update_top(ngravs_ctx *ctx, const double *node_sums, const double *leaf_len);
/* the plan of the kept decomposition (host memory of the context, valid until the next decomposition): this task's rank and the
 * task count, owner of every leaf, present[leaf] (own or imported here), global sums of every top node */
int ngravs_dd_get_kept(ngravs_ctx *ctx, int32_t *rank, int32_t *world, const int32_t **leaf_owner, const uint8_t **present,
                       const double **node_sums);
int ngravs_dd_set_ids(ngravs_ctx *ctx, const int64_t *ids, int on_device);
int ngravs_dd_get_ids(ngravs_ctx *ctx, int64_t *ids, int on_device);
/* ---- pmforce_periodic() for many tasks: x-slab decomposed mesh -----------------------------------------------------------
 * The reference's scheme (pm_periodic.c:74-123 slab tables; :336-427 density patches -> slab owners; :433,:525 distributed
 * FFT in transposed order; :436-520 Green's function on the transposed layout; :529-670 potential bricks with ghost planes
 * back; :681-763 finite differences + CIC gather on the brick).  A task deposits its own particles (not its halo copies)
 * into a brick -- the box of mesh cells (lo[j] + i) mod PMGRID, 0 <= i < ext[j], its CIC clouds touch -- and four
 * all-to-all-v exchanges move planes of that brick / of the slabs:
 *     ngravs_pm_slab_begin(ctx, rank, world, bbox);              bbox = {lo[3], ext[3]};   host: all-gather -> all_bbox[world][6]
 *     for stage = 0..3:
 *         ngravs_pm_slab_pack(ctx, stage, all_bbox, send_counts, recv_counts, &send, &recv);
 *         host: all-to-all-v of doubles, send_counts[r] to / recv_counts[r] from task r, blocks in task order, device buffers
 *         ngravs_pm_slab_unpack(ctx, stage);
 *   stage 0 density planes -> slab owners (+ 2-D r2c FFTs)   1 transpose x<->y (+ 1-D FFTs, Green, inverse 1-D FFTs)
 *   stage 2 transpose back (+ 2-D c2r FFTs)                  3 potential planes with 2 ghost cells per side -> bricks
 *                                                               (+ gradient and CIC gather: GravPM of the own particles)
 * Task r owns the x planes [r*PMGRID/world, (r+1)*PMGRID/world) (integer division), and the same y range of k-space.
 * Mesh memory per task: NG x (brick + two slabs + exchange buffers).  world <= PMGRID/2. */
int ngravs_pm_slab_begin(ngravs_ctx *ctx, int rank, int world, int32_t bbox[6]);
int ngravs_pm_slab_pack(ngravs_ctx *ctx, int stage, const int32_t *all_bbox, int64_t *send_counts, int64_t *recv_counts,
                        void **send, void **recv);
int ngravs_pm_slab_unpack(ngravs_ctx *ctx, int stage);
/* payload this task sent to OTHER tasks in each of the four exchanges of the last step, bytes */
int ngravs_pm_slab_bytes(ngravs_ctx *ctx, double bytes[4]);

/* ---- SPH density: density() (density.c:56-441) for ONE task -----------------------------------------------------------------
 * Targets are the caller's own rows of type 0 that the last hand-over marked active (density.c:95, :123); sources are all type-0
 * particles (ngb.c:221), nearest image in periodic runs.  Every target's smoothing length is iterated to acceptance by the
 * reference's rules (density.c:314-389: NumNgb inside DesNumNgb +- MaxNumNgbDeviation, or above it with Hsml <= 1.01 MinGasHsml,
 * or a bracket narrower than 1e-3; bisection in h^3, the Newton-like step, the factor 1.26; clamp to MinGasHsml), and Density,
 * NumNgb, DivVel, CurlVel, DhsmlDensityFactor come out as after its final operations (density.c:296-303; this call leaves the pressure line,
 * density.c:305-308, to its caller -- ngravs_sph_accelerations below takes the entropy and computes it).  A target that needs more than MAXITER = 150 repeats is the reference's endrun(1155):
 * the fatal handler is called with 1155 and the call returns NGRAVS_ERR_STATE.
 * Needs a built tree of the current particle set (NGRAVS_ERR_STATE otherwise); after ngravs_update_particles the tree is refit
 * first.  The tree, the walk's state and the stored accelerations are not modified.  NGRAVS_ERR_ARG with a message: NULL in /
 * hsml / vel_pred, des_num_ngb <= 0, a negative deviation or minimum, a target whose hsml is <= 0 or NaN.  NGRAVS_ERR_STATE,
 * "single task only": world_size > 1 or a multi-task working set.  No type-0 target: success, nothing written, 0 rounds.
 * Not provided: several tasks, TWODIMS, LONG_X/Y/Z (hydro forces: ngravs_sph_hydro below). */
typedef struct {
  const double *vel_pred; int64_t vel_stride;   /* SphP[].VelPred[3] per own row (rows of other types are not read)      */
  double *hsml;           int64_t hsml_stride;  /* in: starting guess per own row (> 0 for every target), out: result    */
  double des_num_ngb, max_num_ngb_deviation, min_gas_hsml;   /* All.DesNumNgb, All.MaxNumNgbDeviation, All.MinGasHsml   */
  int32_t on_device, reserved;
} ngravs_sph_in_t;
typedef struct {   /* any pointer may be NULL; strides in bytes; rows = own rows, only targets are written */
  double *density, *num_ngb, *div_vel, *curl_vel, *dhsml_factor;
  int64_t density_stride, num_ngb_stride, div_vel_stride, curl_vel_stride, dhsml_factor_stride;
} ngravs_sph_out_t;
/* max_rounds, kernel_ms may be NULL: the most evaluations any target took; device time of the call (HIP events) */
int ngravs_sph_density(ngravs_ctx *ctx, const ngravs_sph_in_t *in, const ngravs_sph_out_t *out, int32_t *max_rounds,
                       double *kernel_ms);
/* The first guess of the smoothing lengths: the loop of setup_smoothinglengths() (init.c:229-247, 3-D branch) for ONE task, on the
 * device tree.  The reference's rule, on its gas-only tree in the domain cube of all particles: from the deepest cell that holds
 * particle i and at least one more gas particle, climb while 10 DesNumNgb m_i > (gas mass of the cell), stop at the root; then
 * Hsml = cbrt(3 / (4 pi) DesNumNgb m_i / mass) * (side of the cell).  hsml (stride in bytes, own rows) is written for every own
 * type-0 row; with only_unset != 0 only for those whose current value is not > 0.  hsml addresses one value per own row; those
 * of rows of other types are never used and never written.  Needs a built tree of the current particle set (NGRAVS_ERR_STATE otherwise; after ngravs_update_particles the tree is
 * refit first); NGRAVS_ERR_STATE, "single task only": world_size > 1 or a multi-task working set.  NGRAVS_ERR_ARG: hsml NULL,
 * des_num_ngb <= 0, a type-0 row whose mass is <= 0 or not finite (nothing is written then).  No type-0 row: success, nothing
 * written.  The tree, the walk's state and the stored accelerations are not modified.  kernel_ms may be NULL. */
int ngravs_sph_hsml_guess(ngravs_ctx *ctx, double des_num_ngb, double *hsml, int64_t hsml_stride, int32_t only_unset, int32_t on_device,
                          double *kernel_ms);
/* GPU-free: the spline and its derivative as the device code evaluates them, wk[i], dwk[i] at r[i] for smoothing length h
 * (0 where r >= h) */
int ngravs_sph_kernel(double h, const double *r, int64_t n, double *wk, double *dwk);

/* ---- SPH hydro force: hydro_force() (hydra.c:50-346) for ONE task -----------------------------------------------------------------
 * The second half of the gas side of compute_accelerations(): after ngravs_sph_density and the host's pressure line, HydroAccel,
 * DtEntropy and MaxSignalVel of every target (own active type-0 row) from hydro_evaluate (hydra.c:353-555) over the symmetric
 * neighbour set r < h_i or r < h_j (ngb_treefind_pairs, ngb.c:64-185; the tree nodes' hmax, forcetree.c:1134-1203, is recomputed
 * from the hsml column on every call and kept apart from what gravity reads), nearest image in periodic runs, with the final
 * operation DtEntropy *= (gamma - 1) / (hubble_a2 Density^(gamma - 1)) (hydra.c:320).  One walk, no iteration.
 * The columns are read for EVERY own type-0 row (every gas particle is a source), rows of other types are not read.  timestep is
 * Ti_endstep - Ti_begstep per row (NULL: all 0, which switches the viscosity limiter off through dt > 0, as at the reference's
 * first step).  What the reference fixes at compile time is an input: gamma (5/3; 1 is ISOTHERM_EQS), viscosity_limiter (1; 0 is
 * NOVISCOSITYLIMITER).  comoving != 0: the caller passes hubble_a2, fac_mu, fac_vsic_fix as hydra.c:78-97 gives them; otherwise
 * the three are taken as 1 whatever was passed.
 * Needs a built tree of the current particle set (NGRAVS_ERR_STATE otherwise); after ngravs_update_particles the tree is refit
 * first.  The tree, the walk's state and the stored accelerations are not modified.  NGRAVS_ERR_ARG with a message: NULL in or
 * a NULL column other than timestep, gamma < 1, a negative constant, a type-0 row whose hsml or density is <= 0 or not finite or
 * whose pressure is < 0 or not finite (the message names the column; nothing is written).  NGRAVS_ERR_STATE, "single task only":
 * world_size > 1 or a multi-task working set.  No type-0 target: success, nothing written.
 * Not provided: several tasks, TWODIMS, LONG_X/Y/Z, SPH_BND_PARTICLES; there is no neighbour list, hence no MAX_NGB second loop. */
typedef struct {   /* strides in bytes; rows = own rows */
  const double *vel_pred;     int64_t vel_pred_stride;      /* SphP[].VelPred[3]                                            */
  const double *hsml;         int64_t hsml_stride;          /* SphP[].Hsml                                                  */
  const double *density;      int64_t density_stride;       /* SphP[].Density                                               */
  const double *pressure;     int64_t pressure_stride;      /* SphP[].Pressure                                              */
  const double *dhsml_factor; int64_t dhsml_factor_stride;  /* SphP[].DhsmlDensityFactor                                    */
  const double *div_vel;      int64_t div_vel_stride;       /* SphP[].DivVel                                                */
  const double *curl_vel;     int64_t curl_vel_stride;      /* SphP[].CurlVel                                               */
  const int32_t *timestep;    int64_t timestep_stride;      /* P[].Ti_endstep - P[].Ti_begstep, or NULL                     */
  double art_bulk_visc_const, timebase_interval, gamma;     /* All.ArtBulkViscConst, All.Timebase_interval, GAMMA           */
  double hubble_a2, fac_mu, fac_vsic_fix;                   /* hydra.c:78-97, read when comoving != 0                       */
  int32_t viscosity_limiter, comoving, on_device, reserved;
} ngravs_hydro_in_t;
typedef struct {   /* any pointer may be NULL; strides in bytes; rows = own rows, only targets are written */
  double *hydro_accel, *dt_entropy, *max_signal_vel;   /* SphP[].HydroAccel[3], DtEntropy, MaxSignalVel */
  int64_t hydro_accel_stride, dt_entropy_stride, max_signal_vel_stride;
} ngravs_hydro_out_t;
/* kernel_ms may be NULL: device time of the call (HIP events) */
int ngravs_sph_hydro(ngravs_ctx *ctx, const ngravs_hydro_in_t *in, const ngravs_hydro_out_t *out, double *kernel_ms);

/* ---- The gas side of compute_accelerations() (accel.c:60-96) for ONE task, in one device-resident call ------------------------------
 * density() INCLUDING its pressure line (density.c:305-308), then force_update_hmax(), then hydro_force(): what ngravs_sph_density,
 * the host's pressure line and ngravs_sph_hydro give one after the other, bit for bit (the two walks are the same kernels), with one
 * target list, one upload of the velocities and no trip through the host between the stages other than the read-back of the
 * density walk's error flags.  Targets are the own active type-0 rows, sources all type-0 rows.
 * The SphP columns hsml, density, pressure, dhsml_factor, div_vel, curl_vel are IN/OUT, as SphP[] is in the reference: read for
 * every type-0 row that is no target (an inactive gas particle is a source with its values of the step before), overwritten for the
 * targets only; a target's hsml is its starting guess on entry, its other five are not read.  Rows of other types are not read.
 * Pressure = (entropy + dt_entropy * dt_entr) * pow(Density, gamma) with dt_entr = (ti_current - (ti_begstep + ti_endstep) / 2) *
 * timebase_interval, the / 2 being the reference's integer division; the hydro timestep of a row is ti_endstep - ti_begstep.
 * dt_entropy NULL: 0.  ti_begstep and ti_endstep both NULL: dt_entr and every timestep are 0.  gamma, viscosity_limiter, comoving and
 * its factors: as in ngravs_hydro_in_t.
 * Refusals are those of the two calls above, code and message: single task only; needs a built tree (refit first when the particles
 * drifted); NGRAVS_ERR_ARG for NULL in, a NULL column other than dt_entropy / the ti pair, only one of the ti pair, des_num_ngb <= 0,
 * a negative deviation, minimum or constant, gamma < 1, a target whose hsml is <= 0 or not finite, a type-0 row whose hsml or
 * density is <= 0 or not finite or whose pressure is < 0 or not finite (of a row that is no target: the value given; of a target:
 * the value computed, e.g. from an entropy that is not finite); MAXITER: the fatal handler is called with 1155, NGRAVS_ERR_STATE,
 * and nothing of the hydro stage has run.  Nothing is written unless the whole call succeeds.  No type-0 target: success, nothing
 * written, 0 rounds.  The tree, the walk's state and the stored accelerations are not modified.
 * Not provided: several tasks, TWODIMS, LONG_X/Y/Z, SPH_BND_PARTICLES. */
typedef struct {   /* strides in bytes; rows = own rows */
  const double *vel_pred;      int64_t vel_pred_stride;      /* SphP[].VelPred[3]                                            */
  const double *entropy;       int64_t entropy_stride;       /* SphP[].Entropy                                               */
  const double *dt_entropy;    int64_t dt_entropy_stride;    /* SphP[].DtEntropy of the step before, or NULL                 */
  const int32_t *ti_begstep;   int64_t ti_begstep_stride;    /* P[].Ti_begstep, or NULL (then ti_endstep is NULL too)        */
  const int32_t *ti_endstep;   int64_t ti_endstep_stride;    /* P[].Ti_endstep                                               */
  double *hsml;                int64_t hsml_stride;          /* in/out: SphP[].Hsml (a target's: the starting guess, > 0)    */
  double *density;             int64_t density_stride;       /* in/out: SphP[].Density                                       */
  double *pressure;            int64_t pressure_stride;      /* in/out: SphP[].Pressure                                      */
  double *dhsml_factor;        int64_t dhsml_factor_stride;  /* in/out: SphP[].DhsmlDensityFactor                            */
  double *div_vel;             int64_t div_vel_stride;       /* in/out: SphP[].DivVel                                        */
  double *curl_vel;            int64_t curl_vel_stride;      /* in/out: SphP[].CurlVel                                       */
  double des_num_ngb, max_num_ngb_deviation, min_gas_hsml;   /* All.DesNumNgb, All.MaxNumNgbDeviation, All.MinGasHsml        */
  double art_bulk_visc_const, timebase_interval, gamma;      /* All.ArtBulkViscConst, All.Timebase_interval, GAMMA           */
  double hubble_a2, fac_mu, fac_vsic_fix;                    /* hydra.c:78-97, read when comoving != 0                       */
  int32_t ti_current, viscosity_limiter, comoving, on_device;   /* All.Ti_Current                                            */
} ngravs_gas_in_t;
typedef struct {   /* any pointer may be NULL; strides in bytes; rows = own rows, only targets are written */
  double *num_ngb, *hydro_accel, *dt_entropy_out, *max_signal_vel;   /* SphP[].NumNgb, HydroAccel[3], DtEntropy, MaxSignalVel */
  int64_t num_ngb_stride, hydro_accel_stride, dt_entropy_out_stride, max_signal_vel_stride;
} ngravs_gas_out_t;
/* max_rounds, kernel_ms may be NULL: the most evaluations any target took; device time (HIP events) of the density walk, of the
 * pressure line + hydro sources + hmax, and of the hydro walk */
int ngravs_sph_accelerations(ngravs_ctx *ctx, const ngravs_gas_in_t *in, const ngravs_gas_out_t *out, int32_t *max_rounds,
                             double *kernel_ms /* [3] */);

/* ---- SPH sums for targets that are NOT the engine's own rows: the per-task half of density() / hydro_force() across tasks ---------
 * What the reference does for a particle it imported, density_evaluate(j, 1) (density.c:231-284) and hydro_evaluate(j, 1)
 * (hydra.c:232-287): partial sums over the LOCAL gas for a target handed in as a record, returned UNFINALISED so that the owner
 * adds the sums of all tasks and finishes them.  The same calls give density, velocity divergence and curl of the gas at
 * arbitrary probe points (tracers, grids).  No communicator is involved: who sends which target where is the caller's business
 * (sph_split.py plays the reference's export loop between engines of one process).
 * Sources are the engine's own type-0 rows (ngb.c:221), nearest image in periodic runs.  A target may lie anywhere in an open
 * run (also outside the cube of the engine's particles); in a periodic run inside [0, BoxSize].  The caller's target order is
 * arbitrary: the targets are walked in the order of the engine's Peano curve (coordinates clamped to the domain cube for the key
 * only) and the sums come back in the caller's order.  An engine without gas: success, all sums 0.  nt == 0: success.
 * Both need a built tree of the current particle set (NGRAVS_ERR_STATE otherwise; after ngravs_update_particles the tree is
 * refit first); NGRAVS_ERR_STATE, "single task only": world_size > 1 or a multi-task working set.  The tree, the walk's state and
 * the stored accelerations are not modified.  NGRAVS_ERR_ARG with a message, and nothing written: a NULL argument, nt < 0, a
 * target whose hsml (hydro: or density) is <= 0 or not finite, whose pressure is < 0 or not finite, whose position is not finite
 * or, in a periodic run, outside [0, BoxSize]; for the hydro sums also what ngravs_sph_hydro refuses about the own rows.
 * on_device: every array of the call (own columns of ngravs_sph_density_sums, targets, sums) is a device array; the own columns
 * of ngravs_sph_hydro_sums follow own->on_device.  sums is contiguous.  kernel_ms may be NULL.
 * Not provided: TWODIMS, LONG_X/Y/Z, SPH_BND_PARTICLES; the exchange itself (ngravs_host_* drivers, the glue). */
typedef struct {   /* strides in bytes; nt rows */
  const double *pos;  int64_t pos_stride;    /* the target's Pos[3]                                  */
  const double *vel;  int64_t vel_stride;    /* its VelPred[3]                                       */
  const double *hsml; int64_t hsml_stride;   /* the trial smoothing length of this round, > 0        */
} ngravs_sph_targets_t;
/* ONE round at the given hsml.  sums [nt][7]: the raw sums of density.c:531-575 -- rho, the weighted neighbour number, dhsmlrho,
 * div, rot[3] -- NOT passed through the final operations density.c:296-303.  A target that coincides with a source gets the
 * r = 0 term and no velocity terms (density.c:560), so an own particle handed in as a target gets its self term.
 * own_vel_pred: SphP[].VelPred[3] per own row (rows of other types are not read). */
int ngravs_sph_density_sums(ngravs_ctx *ctx, const double *own_vel_pred, int64_t own_vel_stride, const ngravs_sph_targets_t *targets,
                            int64_t nt, double *sums, int32_t on_device, double *kernel_ms);
typedef struct {   /* the reference's hydrodata_in (hydra.c:145-162); strides in bytes; nt rows */
  const double *pos;          int64_t pos_stride;            /* Pos[3]                                                      */
  const double *vel;          int64_t vel_stride;            /* VelPred[3]                                                  */
  const double *hsml;         int64_t hsml_stride;           /* Hsml                                                        */
  const double *mass;         int64_t mass_stride;           /* Mass                                                        */
  const double *density;      int64_t density_stride;        /* Density                                                     */
  const double *pressure;     int64_t pressure_stride;       /* Pressure                                                    */
  const double *dhsml_factor; int64_t dhsml_factor_stride;   /* DhsmlDensityFactor                                          */
  const double *f1;           int64_t f1_stride;             /* F1 = |div| / (|div| + curl + 0.0001 c_s / Hsml / fac_mu), computed by the sender (hydra.c:160) */
  const int32_t *timestep;    int64_t timestep_stride;       /* Ti_endstep - Ti_begstep, or NULL (all 0)                    */
} ngravs_hydro_targets_t;
/* own: the engine's own source columns and the constants, as for ngravs_sph_hydro (every own type-0 row is a source).  Per pair
 * exactly hydra.c:416-534.  sums [nt][5]: acc[3], dt_entropy BEFORE the final operation of hydra.c:320, max_signal_vel starting
 * from 0 (the owner adds acc and dt_entropy, takes the maximum of max_signal_vel, then applies hydra.c:320). */
int ngravs_sph_hydro_sums(ngravs_ctx *ctx, const ngravs_hydro_in_t *own, const ngravs_hydro_targets_t *targets, int64_t nt, double *sums,
                          int32_t on_device, double *kernel_ms);
/* The owner's side of one round of density() for n targets whose sums [n][7] have been added up: the final operations
 * density.c:296-303 and the acceptance and bracketing rules density.c:314-389 as ngravs_sph_density applies them (the band, above
 * the band with hsml <= 1.01 MinGasHsml, a bracket narrower than 1e-3; bisection in h^3, the Newton-like step, the factor 1.26;
 * the clamp to MinGasHsml).  hsml, left, right, rounds [n] are IN/OUT: left = right = 0 and rounds = 0 before the first round;
 * rounds is incremented; for a target that is to be repeated hsml holds the next trial length.  accepted [n]: 1 / 0; for accepted
 * targets the six result columns (any may be NULL) are written.  All arrays contiguous, host or device (on_device); the host
 * path needs no GPU.  Host and device give the same bits except for pow() in the bisection step.
 * Returns the number of targets that are to be repeated with rounds > MAXITER = 150 (the reference's endrun(1155)), or a
 * negative NGRAVS_ERR_*. */
typedef struct {
  int32_t *accepted;
  double *hsml, *density, *num_ngb, *div_vel, *curl_vel, *dhsml_factor;
} ngravs_sph_update_out_t;
int64_t ngravs_sph_density_update(int64_t n, const double *sums, double *hsml, double *left, double *right, int32_t *rounds,
                                  double des_num_ngb, double max_num_ngb_deviation, double min_gas_hsml,
                                  const ngravs_sph_update_out_t *out, int32_t on_device);

/* ---- Time integration for ONE task: the stations of run.c:32-65 around the force computation -------------------------------------
 * find_next_sync_point_and_drift (run.c:151-234), move_particles (predict.c:31-76), do_box_wrapping (predict.c:106-133),
 * find_dt_displacement_constraint (timestep.c:587-665), advance_and_find_timesteps with get_timestep (timestep.c:24-576) and the
 * look-up tables of driftfac.c, so that a host whose particles live on the device runs the whole loop without a column leaving it.
 * Every call is STATELESS over the caller's columns: ngravs_time_cols_t is a view of the host's P[] and SphP[] (pointer + stride in
 * bytes per field; any layout, SoA or interleaved), n its number of rows.  on_device != 0: device pointers, used in place;
 * otherwise host pointers, staged by the library.  The context supplies only G, BoxSize, PERIODIC, PMGRID ("a mesh": PMGRID > 0),
 * Asmth and All.SofteningTable[type] = force_softening[type] / 2.8 of the last softening set.  No call touches the engine's
 * particles, its tree, the walk's state or the stored accelerations.  One task: the calls are local; a host with several tasks
 * all-reduces the scalars of the sync point and the 18 displacement sums itself.
 * Which columns a call reads (R) and writes (W), rows of type != 0 never touching a gas column:
 *   sync point        R ti_endstep
 *   move              R type vel, W pos; gas rows: R grav_accel [grav_pm with a mesh] hydro_accel div_vel entropy dt_entropy ti_begstep
 *                     ti_endstep, W vel_pred density hsml pressure
 *   displacement sums R type vel mass
 *   advance           active rows: R type grav_accel [grav_pm with a mesh], W vel ti_begstep ti_endstep; active gas rows: R hydro_accel
 *                     density hsml max_signal_vel, W vel_pred entropy dt_entropy; on a long-range kick ALL rows: R grav_pm, W vel, and
 *                     all gas rows: R grav_accel hydro_accel, W vel_pred
 *   global sums       R type pos vel mass ti_begstep ti_endstep grav_accel [grav_pm with a mesh] [the potential argument, if given];
 *                     gas rows: R hydro_accel entropy dt_entropy density; writes no column
 * Refusals (NGRAVS_ERR_ARG with a message, nothing written): NULL ctx, cols or params, n < 0, NULL where a column is required, a gas
 * column missing while a type-0 row exists, a type outside 0..5, timebase_interval <= 0, gamma < 1, time1 < time0, a comoving
 * call without tables.
 * Not provided: FLEXSTEPS, PSEUDOSYMMETRIC, MAKEGLASS, CONDUCTION, NOPMSTEPADJUSTMENT, PLACEHIGHRESREGION, the node drift and
 * node kicks (predict.c:79-91, timestep.c:331-344: the library refits its tree instead). */
#define NGRAVS_TIMEBASE (1 << 28)          /* allvars.h: TIMEBASE                                     */
#define NGRAVS_DRIFT_TABLE_LENGTH 1000     /* allvars.h: DRIFT_TABLE_LENGTH                           */
typedef struct {   /* strides in bytes; n rows */
  int32_t *type;           int64_t type_stride;            /* P[].Type                                   */
  double *pos;             int64_t pos_stride;             /* P[].Pos[3]                                 */
  double *vel;             int64_t vel_stride;             /* P[].Vel[3]                                 */
  double *mass;            int64_t mass_stride;            /* P[].Mass                                   */
  int32_t *ti_begstep;     int64_t ti_begstep_stride;      /* P[].Ti_begstep                             */
  int32_t *ti_endstep;     int64_t ti_endstep_stride;      /* P[].Ti_endstep                             */
  double *grav_accel;      int64_t grav_accel_stride;      /* P[].GravAccel[3]                           */
  double *grav_pm;         int64_t grav_pm_stride;         /* P[].GravPM[3]; read only with a mesh       */
  double *vel_pred;        int64_t vel_pred_stride;        /* SphP[].VelPred[3]                          */
  double *hydro_accel;     int64_t hydro_accel_stride;     /* SphP[].HydroAccel[3]                       */
  double *entropy;         int64_t entropy_stride;         /* SphP[].Entropy                             */
  double *dt_entropy;      int64_t dt_entropy_stride;      /* SphP[].DtEntropy                           */
  double *density;         int64_t density_stride;         /* SphP[].Density                             */
  double *hsml;            int64_t hsml_stride;            /* SphP[].Hsml                                */
  double *pressure;        int64_t pressure_stride;        /* SphP[].Pressure                            */
  double *div_vel;         int64_t div_vel_stride;         /* SphP[].DivVel                              */
  double *max_signal_vel;  int64_t max_signal_vel_stride;  /* SphP[].MaxSignalVel                        */
  int64_t n;                                               /* NumPart                                    */
  int32_t on_device, reserved;
} ngravs_time_cols_t;
typedef struct {
  double timebase_interval;         /* All.Timebase_interval                                                                   */
  double time_begin, time_max;      /* All.TimeBegin, All.TimeMax: the span of the integer time line (and of the tables)       */
  double omega0, omega_lambda, omega_baryon, hubble;   /* All.Omega0, OmegaLambda, OmegaBaryon, Hubble; read when comoving     */
  double gamma;                     /* GAMMA (5/3; 1 is ISOTHERM_EQS)                                                          */
  double min_gas_hsml;              /* All.MinGasHsml                                                                          */
  double err_tol_int_accuracy, courant_fac;            /* All.ErrTolIntAccuracy, All.CourantFac                                */
  double max_size_timestep, min_size_timestep;         /* All.MaxSizeTimestep, All.MinSizeTimestep                             */
  double max_rms_displacement_fac;  /* All.MaxRMSDisplacementFac                                                               */
  double min_egy_spec;              /* All.MinEgySpec (0: no floor)                                                            */
  double timestep_scale;            /* NGRAVS_TIMESTEP_SCALE (timestep.c:484-493); 0 => 1                                      */
  const double *drift_table, *gravkick_table, *hydrokick_table;   /* HOST arrays of NGRAVS_DRIFT_TABLE_LENGTH (driftfac.c);
                                                                     required when comoving != 0                               */
  int32_t comoving;                 /* All.ComovingIntegrationOn                                                               */
  int32_t adaptive_gravsoft;        /* ADAPTIVE_GRAVSOFT_FORGAS: a gas row's softening in the step criterion is Hsml / 2.8      */
  int32_t synchronization;          /* SYNCHRONIZATION (timestep.c:240-246); 1 in the reference's Makefile                     */
  int32_t stop_below_min_timestep;  /* 1: a step below MinSizeTimestep is fatal (888), the reference's default; 0: the step
                                       becomes MinSizeTimestep (NOSTOP_WHEN_BELOW_MINTIMESTEP)                                 */
} ngravs_time_params_t;
typedef struct {
  int32_t ti_next;       /* the next sync point: min Ti_endstep, or PM_Ti_endstep when the minimum is not below it (run.c:175-181) */
  int32_t full_step;     /* Flag_FullStep: every row sits on the minimum, or the PM rule applied                                  */
  int64_t n_active;      /* NumForceUpdate: rows with Ti_endstep == ti_next                                                        */
} ngravs_sync_t;
/* init_drift_table (driftfac.c:26-60), host, no GPU: drift[i], gravkick[i], hydrokick[i] = the integrals of driftfac.c:179-212 from
 * time_begin to exp(log time_begin + (log time_max - log time_begin) / LENGTH * (i + 1)), LENGTH entries each.  Reads omega0,
 * omega_lambda, hubble, gamma, time_begin, time_max of par.  A fixed rule instead of the reference's adaptive one at 1e-8: every
 * table cell is integrated in log a by Gauss-Legendre, rule 0 with 12 nodes on one panel, rule 1 (the check) with 12 nodes on each
 * of two panels, and the cells are added up.  NGRAVS_ERR_ARG: a NULL argument, time_begin <= 0, time_max <= time_begin, hubble <= 0,
 * gamma < 1, another rule. */
int ngravs_time_tables(const ngravs_time_params_t *par, int32_t rule, double *drift, double *gravkick, double *hydrokick);
/* get_drift_factor, get_gravkick_factor, get_hydrokick_factor (driftfac.c:67-174) for the integer times ti0, ti1 from the tables
 * in par -> out[3]; the branch for the first two cells and the clamp at the table's end included.  Host, no GPU; the device code
 * evaluates the same function. */
int ngravs_time_factors(const ngravs_time_params_t *par, int32_t ti0, int32_t ti1, double out[3]);
/* run.c:161-191.  pm_ti_endstep < 0: no PM time (tree-only).  NGRAVS_ERR_ARG also for n = 0 (the minimum of nothing). */
int ngravs_next_sync_point(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, int32_t pm_ti_endstep, ngravs_sync_t *out);
/* move_particles from the integer time time0 to time1 (predict.c:31-76) over ALL rows; the three factors come from the tables,
 * once per call, when comoving.  wrap != 0: afterwards do_box_wrapping (predict.c:124-132) when the configuration is periodic --
 * the reference wraps only in front of a decomposition, the caller decides. */
int ngravs_move_particles(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int32_t time0,
                          int32_t time1, int32_t wrap);
/* The local sums of timestep.c:606-612: sums[0..5] = sum of |Vel|^2 per type, [6..11] the smallest mass per type (1.0e30 for a
 * type without rows), [12..17] the number of rows per type.  The same sums bit for bit on every call with the same columns. */
int ngravs_displacement_sums(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, double sums[18]);
/* The rest of find_dt_displacement_constraint (timestep.c:595-659) from the (all-reduced) sums, host, no GPU: MaxSizeTimestep
 * without comoving integration; else per populated type the dmean rule (OmegaBaryon for type 0) and, when asmth > 0 (a mesh:
 * All.Asmth[0]) and asmth < dmean, the Asmth rule, with hfac = a^2 H(a) at the expansion factor `time`. */
int ngravs_dt_displacement(const ngravs_time_params_t *par, const double sums[18], double G, double asmth, double time,
                           double *dt_displacement);
/* advance_and_find_timesteps at All.Ti_Current = ti_current (timestep.c:24-413) for the rows with Ti_endstep == ti_current, with
 * the caller's dt_displacement; All.Time is time_begin * exp(ti_current * timebase_interval) when comoving.  With a mesh pm_ti[2] =
 * {All.PM_Ti_begstep, All.PM_Ti_endstep} is required, in/out, and when pm_ti[1] == ti_current the long-range kick of
 * timestep.c:351-408 runs over ALL rows.  The steps are decided in one pass and applied in a second: NOTHING is written unless the
 * whole call succeeds.  The two fatal cases call the fatal handler with the reference's code and the lowest failing row, and
 * return NGRAVS_ERR_STATE: 888, a step below MinSizeTimestep (with stop_below_min_timestep); 818, a step on the integer line that
 * is not in (0, TIMEBASE) -- a quotient dt / timebase_interval that no int holds is this case.  n_kicked (may be NULL): the rows
 * advanced. */
int ngravs_advance_and_find_timesteps(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par,
                                      int32_t ti_current, double dt_displacement, int32_t *pm_ti, int64_t *n_kicked);

/* ---- Energy statistics: compute_global_quantities_of_system (global.c:22-198) and the energy.txt line of energy_statistics
 * (run.c:413-433), the station of the main loop between compute_accelerations() and advance_and_find_timesteps() (run.c:52-59).
 * Split like the displacement constraint: the local sums on the device, then a host rule on the (all-reduced) sums, so that a host
 * with several tasks adds the 78 numbers of its tasks in between (the reference's MPI_Reduce, global.c:118-127).
 * P[].Potential is a column the caller hands in, ngravs_compute_potential's or its own; without it EnergyPot is 0, as in the
 * reference built without COMPUTE_POTENTIAL_ENERGY. */
#define NGRAVS_GLOBAL_NSUMS 78
typedef struct {   /* struct state_of_system, allvars.h, field for field: 119 doubles, 952 bytes; [3] of a vector is its norm */
  double Mass, EnergyKin, EnergyPot, EnergyInt, EnergyTot, Momentum[4], AngMomentum[4], CenterOfMass[4];
  double MassComp[6], EnergyKinComp[6], EnergyPotComp[6], EnergyIntComp[6], EnergyTotComp[6];
  double MomentumComp[6][4], AngMomentumComp[6][4], CenterOfMassComp[6][4];
} ngravs_sysstate_t;
/* The local sums of global.c:52-114 at All.Ti_Current = ti_current over ALL rows: sums[13 * type + k], k = 0 mass, 1 kinetic
 * energy 0.5 m |vel|^2 / a^2, 2 internal energy (type 0 only), 3 potential energy 0.5 m Potential / a (0 without the column),
 * 4..6 m vel, 7..9 m (pos x vel), 10..12 m pos.  vel is the velocity predicted to ti_current from the middle of the row's step:
 * Vel + GravAccel dt_gravkick [+ HydroAccel dt_hydrokick for type 0] [+ GravPM dt_pm with a mesh], and the entropy of a gas row is
 * Entropy + DtEntropy dt; when comoving the two kick factors come from the tables and a = time_begin * exp(ti_current *
 * timebase_interval), else a = 1.  The internal energy is m entr / (gamma - 1) (Density / a^3)^(gamma - 1), and m entr for gamma = 1
 * (ISOTHERM_EQS).  potential: NULL, or P[].Potential with its stride in bytes, a device or host pointer as cols->on_device says.
 * With a mesh pm_ti[2] = {All.PM_Ti_begstep, All.PM_Ti_endstep} is required (read only).  n = 0 gives 78 zeros.  The same sums bit
 * for bit on every call with the same columns: no floating-point atomic, one partial per block, added in an order the number of
 * rows alone fixes.  Refusals as for the other time calls, and a mesh without pm_ti; nothing is written then. */
int ngravs_global_sums(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, int32_t ti_current,
                       const int32_t *pm_ti, const double *potential, int64_t potential_stride, double sums[NGRAVS_GLOBAL_NSUMS]);
/* global.c:130-194 from the (all-reduced) sums, host, no GPU, in the reference's order of operations: EnergyTotComp, the totals,
 * the centres of mass divided by the mass where that is > 0, and the norms in [3]. */
int ngravs_global_finish(const double sums[NGRAVS_GLOBAL_NSUMS], ngravs_sysstate_t *out);
/* The line energy_statistics() appends to energy.txt (run.c:419-429), host, no GPU: time, EnergyInt, EnergyPot, EnergyKin, the same
 * three per type, MassComp[6] -- 28 %g fields separated by blanks, a newline, a terminating 0.  Returns the length without the
 * 0, or NGRAVS_ERR_ARG for a NULL argument or a buffer shorter than length + 1. */
int ngravs_energy_line(const ngravs_sysstate_t *s, double time, char *buf, int64_t len);

/* ---- Snapshot files: savepositions() (io.c:33-989) for one task and one file, and find_next_outputtime() (run.c:244-361), the
 * station of the main loop inside find_next_sync_point_and_drift (run.c:206-225).  The device does the per-row conversions of
 * fill_write_buffer (io.c:129-357) and the grouping by type; the host frames the records.
 * The FILE ORDER of io.c is type by type, and within a type the order of P[] (io.c:178-206).  ngravs_snapshot_plan builds it once
 * per snapshot from the type column, a stable partition, as a permutation kept in the context until the next plan or
 * ngravs_destroy; the same permutation on every call.  Every block call then takes a range [first, first + count) of a block's
 * elements in that order and writes them as they lie on disk: float32 (int32 for ID), three per element for POS, VEL and ACCE.
 * The statements are the reference's and round to float after EACH of them, with nothing contracted into a fused multiply-add:
 *   POS   (float) Pos; periodic: the two while loops of io.c:198-201 on the float (-1e-9 becomes BoxSize and then 0)
 *   VEL   Vel + GravAccel dt_gravkick; type 0: += HydroAccel dt_hydrokick; with a mesh: += GravPM dt_gravkick_pm; *= sqrt(a3inv);
 *         the kick factors as in ngravs_global_sums
 *   ID    snap->ids (int32; LONGIDS is not provided)
 *   MASS  Mass, only for the types whose mass_table entry is 0 (io.c:501-508)
 *   U     dmax(MinEgySpec, Entropy / (gamma - 1) * pow(Density a3inv, gamma - 1)); gamma == 1: Entropy (ISOTHERM_EQS)
 *   RHO HSML ENDT   Density, Hsml, DtEntropy of the type-0 rows
 *   POT   snap->potential (ngravs_compute_potential's column, or the caller's own); the block exists only with the column
 *   ACCE  fac1 GravAccel; with a mesh: += fac1 GravPM; type 0: += fac2 HydroAccel  (fac1 = 1 / a^2, fac2 = 1 / a^(3 gamma - 2))
 *   TSTP  (Ti_endstep - Ti_begstep) Timebase_interval
 * a = time_begin exp(ti_current timebase_interval) when comoving, else 1.  The context supplies PERIODIC, BoxSize and PMGRID.
 * Refusals (NGRAVS_ERR_ARG with a message, nothing written, a file not touched): those of the other time calls, a type outside
 * 0..5 (at the plan), a block whose column is missing, a range outside the block, a mesh without pm_ti, a periodic POS coordinate
 * that is not finite or has |x| >= 1024 BoxSize (the reference's loops would run that many trips, and for ever from 2^24 box
 * lengths on), snap_format 3 (no HDF5).  NGRAVS_ERR_STATE: a block call before a plan or with an n that is not the plan's.
 * Not provided: HDF5, LONGIDS, LONG_X/Y/Z, several files per snapshot and the communicator driver for several tasks (the ranged
 * block call is the per-task half), restart files. */
enum { NGRAVS_SNAP_POS, NGRAVS_SNAP_VEL, NGRAVS_SNAP_ID, NGRAVS_SNAP_MASS, NGRAVS_SNAP_U, NGRAVS_SNAP_RHO, NGRAVS_SNAP_HSML,
       NGRAVS_SNAP_POT, NGRAVS_SNAP_ACCE, NGRAVS_SNAP_ENDT, NGRAVS_SNAP_TSTP, NGRAVS_SNAP_NBLOCKS };   /* enum iofields, allvars.h */
typedef struct {
  int32_t ti_current, reserved;      /* All.Ti_Current                                                                        */
  const int32_t *pm_ti;              /* {All.PM_Ti_begstep, All.PM_Ti_endstep}, HOST; required with a mesh, else NULL         */
  double mass_table[6];              /* All.MassTable: header.mass, and which types the MASS block holds                      */
  const int32_t *ids;     int64_t ids_stride;         /* P[].ID, of the kind of the columns (cols->on_device)                 */
  const double *potential; int64_t potential_stride;  /* P[].Potential or NULL, of the kind of the columns                    */
  double box_size;                   /* header.BoxSize (the block calls wrap with the context's BoxSize)                      */
  double hubble_param;               /* header.HubbleParam = All.HubbleParam                                                  */
} ngravs_snapshot_t;
typedef struct {
  int32_t output_list_on, output_list_length;   /* All.OutputListOn, All.OutputListLength                                     */
  const double *output_list_times;              /* All.OutputListTimes, HOST                                                  */
  double time_of_first_snapshot, time_bet_snapshot;   /* All.TimeOfFirstSnapshot, All.TimeBetSnapshot                         */
} ngravs_output_rule_t;
/* The file order of cols->type, cols->n rows, into the context; npart[6]: the rows of each type.  Reads the type column only. */
int ngravs_snapshot_plan(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, int64_t npart[6]);
/* get_particles_in_block (io.c:465-523) for the plan's counts and snap->mass_table, host: the block's number of elements and the
 * bytes of one (12 or 4; may be NULL). */
int ngravs_snapshot_block_count(ngravs_ctx *ctx, const ngravs_snapshot_t *snap, int32_t block, int64_t *count, int32_t *bytes_per_element);
/* The elements [first, first + count) of `block` -> out, count * bytes_per_element bytes, a device pointer when out_on_device != 0.
 * A host writes with a bounded buffer this way (All.BufferSize, io.c:821), and a host with several tasks asks each for its share. */
int ngravs_snapshot_block(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                          int32_t block, int64_t first, int64_t count, void *out, int32_t out_on_device);
/* struct io_header as write_file fills it (io.c:720-761), host, no GPU: npart, mass = mass_table, time, redshift (1 / time - 1 when
 * comoving, else 0), five zero flags, npartTotal and its high word, num_files, BoxSize, Omega0, OmegaLambda, HubbleParam, zeros. */
int ngravs_snapshot_header(const ngravs_time_params_t *par, const ngravs_snapshot_t *snap, const int64_t npart[6], const int64_t npart_total[6],
                           int32_t num_files, double time, unsigned char out[256]);
/* savepositions() for one task and one file: plan (the context's plan is this call's afterwards), header, and every present block
 * with elements, in the reference's order, in chunks of buffer_bytes (0: 64 MiB) through the device.  snap_format 1, or 2 with the
 * label records of io.c:796-803, 832-839.  blocks_mask: bit NGRAVS_SNAP_* set = the block is present (blockpresent, io.c:532-556: the
 * four OUTPUT* switches); POS VEL ID MASS U RHO HSML always are.  Everything is checked before the file is opened. */
int ngravs_snapshot_write(ngravs_ctx *ctx, const ngravs_time_cols_t *cols, const ngravs_time_params_t *par, const ngravs_snapshot_t *snap,
                          uint32_t blocks_mask, int32_t snap_format, int64_t buffer_bytes, const char *path);
/* find_next_outputtime(ti_curr) (run.c:244-361), host, no GPU: the first output time >= ti_curr on the integer time line, from the
 * list of times or from TimeOfFirstSnapshot / TimeBetSnapshot; 2 * NGRAVS_TIMEBASE when there is none.  Reads timebase_interval,
 * time_begin, time_max and comoving of par.  NGRAVS_ERR_ARG with a message in ngravs_last_error(NULL) where the reference ends
 * with 13123 (TimeBetSnapshot <= 1 comoving, <= 0 otherwise), 110 or 111 (no time found in a million steps). */
int ngravs_find_next_outputtime(const ngravs_time_params_t *par, const ngravs_output_rule_t *rule, int32_t ti_curr, int32_t *ti_next);

/* ---- Gravitational potentials: compute_potential() (potential.c:22-345) for one task -- the column ngravs_global_sums and the POT
 * block of a snapshot take.  What the reference's potential routines mean, not what they do (DESIGN.md §8 lists their defects).
 * Built-in laws with a wired potential companion: NGRAVS_LAW_NEWTON / NGRAVS_LAW_NEG_NEWTON (newtonian_pot, neg_newtonian_pot) with
 * NGRAVS_SPLINE_PLUMMER / NGRAVS_SPLINE_NEG_PLUMMER (plummer_pot, neg_plummer_pot; ngravs.c:368-489); a pair wired NONE gives 0.
 * Every other law, and a Newton pair whose companion is to be replaced, takes the model's own functions from an entry of
 * ngravs_create_with_potentials: Pfn(m, r) = m pot(1, 1, 0, r, 1) and Pspl(m, h, r) = m pot_spline(1, 1, h, r, 1) from their
 * tables, its lattice_pot(x) / BoxSize in the place of sign(law) ewald_psi / BoxSize in step 1 (the origin of the table
 * lattice_zero / BoxSize), - m pot_spline[g][g](1, 1, h, 0, 1) in the place of step 2 for a row of species g (plummer_pot gives
 * the reference's m / SofteningTable; a lone particle's potential is 0 under every law), and its lattice_zero[g][g] in step 3.  The
 * long-range share removed in a TreePM run is that of the pair's law_normed, the mesh part that of its law_greens, built in or
 * user, as for the force.  The mesh's k = 0 is 0: for a screened law, whose Green's function is finite there, this leaves a
 * constant per target species (G sum of the source masses x greens(0) / volume) out of the column.
 * For ALL own rows, whatever their active flags, in the order of potential.c:244-337:
 *   1. the potential walk of the built tree with the context's opening criterion (the strict walk's traversal): per source of mass
 *      m at distance r, h = max(h_target, h_source):  r >= h: -= Pfn(m, r);  r < h: += Pspl(m, h, r);  periodic tree-only: += m x
 *      the trilinear lookup of sign(law) ewald_psi / BoxSize in the same visit;  TreePM, for r < 6 Asmth: the long-range share
 *      m erf(r / 2 Asmth) / r of the pair is removed from both branches, from the row's own visit too (the mesh holds it)
 *   2. += m / SofteningTable[type] = 2.8 m / force_softening[type]
 *   3. comoving and periodic: -= LatticeZero[g][g] m^(2/3) (Omega0 3 H^2 / (8 pi G))^(1/3), LatticeZero = sign(law) 2.8372975
 *   4. *= G
 *   5. TreePM: += G / (pi BoxSize) x the CIC read-back of the mesh potential (deposit, transforms and Green multiply at the CURRENT
 *      positions; k = 0 is 0, as for the force)
 *   6. comoving, not periodic: += -0.5 Omega0 H^2 |pos|^2;  not comoving: += -0.5 OmegaLambda H^2 |pos|^2
 * par: the parameters of the time calls (comoving, omega0, omega_lambda, hubble are read), or NULL: neither comoving nor Lambda.
 * potential: the caller's column, stride in bytes, caller's row order; nint (may be NULL): the interactions of every row's walk,
 * int32, contiguous.  GravAccel, GravPM, OldAcc and the costs of the last force computation stay as they are; with a mesh the call
 * rewrites the potential mesh: ngravs_pm_targets is refused until the next PM step, ngravs_potential_targets is served until the
 * next PM step or hand-over of particles.
 * NGRAVS_ERR_ARG for a NULL ctx.  Refused with a message and nothing written: NGRAVS_ERR_ARG for a NULL potential, world_size > 1 or
 * a multi-task working set, adaptive gas softening, a BAM law in a wired pair, a wired pair that has neither a built-in companion
 * nor an entry of ngravs_create_with_potentials (the first such pair is named), a mesh without periodic boundaries; NGRAVS_ERR_STATE without a built tree of the current particle set (after ngravs_update_particles it is refit first). */
int ngravs_compute_potential(ngravs_ctx *ctx, const ngravs_time_params_t *par, double *potential, int64_t potential_stride,
                             int32_t on_device, int32_t *nint);
/* Step 1 x G, plus step 5 with a mesh, at nt target records (the records of ngravs_gravity_tree_targets, any order, any finite
 * position when not periodic): no self term, no cosmological term -- the potential of this engine's particles at the targets, so
 * that the potential of a set split over engines is the sum over the engines.  pot[nt] and nint[nt] (may be NULL), contiguous,
 * of the kind of the records.  With a mesh the mesh of the last ngravs_compute_potential is read: NGRAVS_ERR_STATE without one.
 * Other refusals as above and as for ngravs_gravity_tree_targets' records. */
int ngravs_potential_targets(ngravs_ctx *ctx, const ngravs_grav_targets_t *targets, int64_t nt, double *pot, int32_t *nint);
/* The lattice potential table of the pair (target, source) as the periodic tree-only walk reads it: out[65^3] (host),
 * [i][j][k] = sign(law) ewald_psi(i / 128, j / 128, k / 128) / BoxSize, the origin sign(law) 2.8372975 / BoxSize.  Tabulated on the
 * device at the first use.  A pair with an entry of ngravs_create_with_potentials: its lattice_pot / BoxSize, the origin its
 * lattice_zero / BoxSize, sampled on the host. NGRAVS_ERR_ARG unless the configuration is periodic without a mesh and the pair is wired. */
int ngravs_lattice_potential_table(ngravs_ctx *ctx, int32_t target, int32_t source, double *out);
/* device milliseconds of the walk kernel of the last ngravs_compute_potential (HIP events) */
int ngravs_last_potential_ms(ngravs_ctx *ctx, double *walk_ms);

#ifdef __cplusplus
}
#endif
#endif /* NGRAVS_HIP_H */
