"""ctypes mirror of include/ngravs_hip.h (plain-C ABI types shared by the engine and the tests).

Field order/types must match the header exactly; tests/test_abi.py checks sizeof against the
compiled library (ngravs_build_info) so that a drift is caught on CPU.
"""
import ctypes as C

ABI_VERSION = 3
MAX_GRAVS = 3
NTYPES = 6
NTAB = 2048
ASMTH = 1.25
RCUT = 4.5
BITS_PER_DIMENSION = 18

LAW_NONE, LAW_NEWTON, LAW_NEG_NEWTON, LAW_YUKAWA, LAW_COLOYUK, LAW_BAMBAM, LAW_SOURCEBAM, LAW_TARGETBAM = range(8)
SPLINE_NONE, SPLINE_PLUMMER, SPLINE_NEG_PLUMMER, SPLINE_BAMBAM, SPLINE_SOURCEBAM, SPLINE_TARGETBAM = range(6)
WALK_STRICT, WALK_GROUP = 0, 1
# user-defined laws (ngravs_create_with_laws): registry entry k is LAW_USER0 + k / SPLINE_USER0 + k
LAW_USER0 = 64
SPLINE_USER0 = 64
MAX_USER_FNS = 8
USER_ACCEL, USER_SPLINE, USER_GREENS, USER_NORMED = range(4)
USER_POT, USER_POT_SPLINE = 4, 5   # user_table_eval only: potentials travel in user_potentials (ngravs_create_with_potentials)
KERNEL_NONE, KERNEL_STRICT, KERNEL_STRICT_USER, KERNEL_GROUP, KERNEL_GROUP_USER, KERNEL_STRICT_ADAPTIVE, KERNEL_GROUP_ADAPTIVE = range(7)
# the reference's `gravity` type (allvars.h:134): double f(double target, double source, double r2_or_h_or_k2, double r_or_k, long N)
GravityFn = C.CFUNCTYPE(C.c_double, C.c_double, C.c_double, C.c_double, C.c_double, C.c_long)

LAW_NAMES = {"none": LAW_NONE, "newtonian": LAW_NEWTON, "neg_newtonian": LAW_NEG_NEWTON,
             "yukawa": LAW_YUKAWA, "coloyuk": LAW_COLOYUK}
SPLINE_NAMES = {"none": SPLINE_NONE, "plummer": SPLINE_PLUMMER, "neg_plummer": SPLINE_NEG_PLUMMER}

_G3 = (C.c_int32 * MAX_GRAVS) * MAX_GRAVS


class Config(C.Structure):
    _fields_ = [
        ("abi_version", C.c_int32), ("n_gravs", C.c_int32), ("periodic", C.c_int32), ("pmgrid", C.c_int32),
        ("box_size", C.c_double), ("G", C.c_double), ("err_tol_theta", C.c_double),
        ("err_tol_force_acc", C.c_double),
        ("force_softening", C.c_double * NTYPES), ("type_to_grav", C.c_int32 * NTYPES),
        ("law_accel", _G3), ("law_spline", _G3), ("law_greens", _G3), ("law_normed", _G3),
        ("yukawa_imass", C.c_double), ("asmth", C.c_double), ("rcut", C.c_double),
        ("tree_alloc_factor", C.c_double), ("group_reach", C.c_double),
        ("walk_mode", C.c_int32), ("device", C.c_int32), ("rank", C.c_int32), ("world_size", C.c_int32),
        ("bam_epsilon", C.c_double), ("reserved", C.c_int32 * 6),
    ]


class Particles(C.Structure):
    _fields_ = [
        ("n", C.c_int64),
        ("pos", C.c_void_p), ("pos_stride", C.c_int64),
        ("mass", C.c_void_p), ("mass_stride", C.c_int64),
        ("type", C.c_void_p), ("type_stride", C.c_int64),
        ("old_acc", C.c_void_p), ("old_acc_stride", C.c_int64),
        ("active", C.c_void_p), ("active_stride", C.c_int64),
        ("grav_pm", C.c_void_p), ("grav_pm_stride", C.c_int64),
        ("grav_cost", C.c_void_p), ("grav_cost_stride", C.c_int64),
        ("on_device", C.c_int32), ("reserved", C.c_int32),
    ]


class UserFn(C.Structure):
    _fields_ = [("kind", C.c_int32), ("reserved", C.c_int32), ("fn", GravityFn)]


# the model's lattice corrections (ngravs_create_with_lattice): the reference's latforce, fn(i, j, k, x[3], force[3])
LATTICE_FN = C.CFUNCTYPE(None, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_double), C.POINTER(C.c_double))
LAT_EN1 = 65   # NGRAVS_EN + 1 points per dimension of a lattice table


class UserLattice(C.Structure):
    _fields_ = [("target", C.c_int32), ("source", C.c_int32), ("fn", LATTICE_FN)]


def lattice_fn(fn):
    """a LATTICE_FN instance as it is, a Python callable fn(i, j, k, x, force) wrapped (x and force are ctypes double pointers)"""
    if fn is None:
        return LATTICE_FN()   # NULL: the library refuses the entry
    return fn if isinstance(fn, LATTICE_FN) else LATTICE_FN(fn)


def lattice_registry(user_lattice):
    """[(target, source, fn), ...] -> (ctypes array of UserLattice, its length, the callback wrappers, which must outlive
    every use of the array)"""
    user_lattice = list(user_lattice or [])
    arr = (UserLattice * max(len(user_lattice), 1))()
    keep = []
    for k, (t, s, fn) in enumerate(user_lattice):
        w = lattice_fn(fn)
        keep.append(w)
        arr[k].target, arr[k].source, arr[k].fn = int(t), int(s), w
    return arr, len(user_lattice), keep


# the model's potential companions (ngravs_create_with_potentials): the reference's latpot, double fn(double x[3])
LATTICE_POT_FN = C.CFUNCTYPE(C.c_double, C.POINTER(C.c_double))


class UserPotential(C.Structure):
    _fields_ = [("target", C.c_int32), ("source", C.c_int32), ("pot", GravityFn), ("pot_spline", GravityFn),
                ("lattice_pot", LATTICE_POT_FN), ("lattice_zero", C.c_double)]


def potential_registry(user_potentials):
    """[(target, source, pot, pot_spline, lattice_pot or None, lattice_zero), ...] -> (ctypes array of UserPotential, its length,
    the callback wrappers, which must outlive every use of the array); None for pot or pot_spline is NULL, which the library refuses"""
    user_potentials = list(user_potentials or [])
    arr = (UserPotential * max(len(user_potentials), 1))()
    keep = []
    for k, (t, s, pot, spl, lat, zero) in enumerate(user_potentials):
        wp = GravityFn() if pot is None else (pot if isinstance(pot, GravityFn) else GravityFn(pot))
        ws = GravityFn() if spl is None else (spl if isinstance(spl, GravityFn) else GravityFn(spl))
        wl = LATTICE_POT_FN() if lat is None else (lat if isinstance(lat, LATTICE_POT_FN) else LATTICE_POT_FN(lat))
        keep += [wp, ws, wl]
        arr[k].target, arr[k].source, arr[k].pot, arr[k].pot_spline, arr[k].lattice_pot = int(t), int(s), wp, ws, wl
        arr[k].lattice_zero = float(zero)
    return arr, len(user_potentials), keep


def user_registry(user_fns):
    """[(kind, callable), ...] -> (ctypes array of UserFn, the callback wrappers, which must outlive every use of the array)"""
    user_fns = list(user_fns or [])
    if len(user_fns) > MAX_USER_FNS:
        raise ValueError("at most %d user-defined laws" % MAX_USER_FNS)
    arr = (UserFn * max(len(user_fns), 1))()
    keep = []
    for k, (kind, fn) in enumerate(user_fns):
        w = fn if isinstance(fn, GravityFn) else GravityFn(fn)
        keep.append(w)
        arr[k].kind = int(kind)
        arr[k].fn = w
    return arr, len(user_fns), keep


class Stats(C.Structure):
    _fields_ = [
        ("n_active", C.c_int64), ("n_nodes", C.c_int64), ("interactions", C.c_double),
        ("t_domain", C.c_double), ("t_peano", C.c_double), ("t_treebuild", C.c_double),
        ("t_treewalk", C.c_double), ("t_pm", C.c_double), ("walk_kernel_ms", C.c_double),
        ("reserved", C.c_double * 7),
    ]


class SphIn(C.Structure):
    _fields_ = [
        ("vel_pred", C.c_void_p), ("vel_stride", C.c_int64),
        ("hsml", C.c_void_p), ("hsml_stride", C.c_int64),
        ("des_num_ngb", C.c_double), ("max_num_ngb_deviation", C.c_double), ("min_gas_hsml", C.c_double),
        ("on_device", C.c_int32), ("reserved", C.c_int32),
    ]


SPH_OUT_NAMES = ("density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor")


class SphOut(C.Structure):
    _fields_ = [(k, C.c_void_p) for k in SPH_OUT_NAMES] + [(k + "_stride", C.c_int64) for k in SPH_OUT_NAMES]


# int ngravs_sph_hsml_guess(ctx, des_num_ngb, hsml, hsml_stride, only_unset, on_device, kernel_ms)
SPH_HSML_GUESS_ARGTYPES = [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]


HYDRO_IN_NAMES = ("vel_pred", "hsml", "density", "pressure", "dhsml_factor", "div_vel", "curl_vel", "timestep")
HYDRO_OUT_NAMES = ("hydro_accel", "dt_entropy", "max_signal_vel")


class HydroIn(C.Structure):
    """ngravs_hydro_in_t"""
    _fields_ = [f for k in HYDRO_IN_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))] + [
        ("art_bulk_visc_const", C.c_double), ("timebase_interval", C.c_double), ("gamma", C.c_double),
        ("hubble_a2", C.c_double), ("fac_mu", C.c_double), ("fac_vsic_fix", C.c_double),
        ("viscosity_limiter", C.c_int32), ("comoving", C.c_int32), ("on_device", C.c_int32), ("reserved", C.c_int32),
    ]


class HydroOut(C.Structure):
    """ngravs_hydro_out_t"""
    _fields_ = [(k, C.c_void_p) for k in HYDRO_OUT_NAMES] + [(k + "_stride", C.c_int64) for k in HYDRO_OUT_NAMES]


GAS_IN_NAMES = ("vel_pred", "entropy", "dt_entropy", "ti_begstep", "ti_endstep")
GAS_INOUT_NAMES = ("hsml", "density", "pressure", "dhsml_factor", "div_vel", "curl_vel")
GAS_OUT_NAMES = ("num_ngb", "hydro_accel", "dt_entropy_out", "max_signal_vel")


class GasIn(C.Structure):
    """ngravs_gas_in_t"""
    _fields_ = [f for k in GAS_IN_NAMES + GAS_INOUT_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))] + [
        ("des_num_ngb", C.c_double), ("max_num_ngb_deviation", C.c_double), ("min_gas_hsml", C.c_double),
        ("art_bulk_visc_const", C.c_double), ("timebase_interval", C.c_double), ("gamma", C.c_double),
        ("hubble_a2", C.c_double), ("fac_mu", C.c_double), ("fac_vsic_fix", C.c_double),
        ("ti_current", C.c_int32), ("viscosity_limiter", C.c_int32), ("comoving", C.c_int32), ("on_device", C.c_int32),
    ]


class GasOut(C.Structure):
    """ngravs_gas_out_t"""
    _fields_ = [(k, C.c_void_p) for k in GAS_OUT_NAMES] + [(k + "_stride", C.c_int64) for k in GAS_OUT_NAMES]


SPH_TARGET_NAMES = ("pos", "vel", "hsml")
HYDRO_TARGET_NAMES = ("pos", "vel", "hsml", "mass", "density", "pressure", "dhsml_factor", "f1", "timestep")
SPH_SUM_NAMES = ("rho", "num_ngb", "dhsmlrho", "div", "rot_x", "rot_y", "rot_z")          # a row of ngravs_sph_density_sums
HYDRO_SUM_NAMES = ("acc_x", "acc_y", "acc_z", "dt_entropy", "max_signal_vel")             # a row of ngravs_sph_hydro_sums
SPH_UPDATE_NAMES = ("hsml",) + SPH_OUT_NAMES


class SphTargets(C.Structure):
    """ngravs_sph_targets_t"""
    _fields_ = [f for k in SPH_TARGET_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))]


class HydroTargets(C.Structure):
    """ngravs_hydro_targets_t"""
    _fields_ = [f for k in HYDRO_TARGET_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))]


class SphUpdateOut(C.Structure):
    """ngravs_sph_update_out_t"""
    _fields_ = [("accepted", C.c_void_p)] + [(k, C.c_void_p) for k in SPH_UPDATE_NAMES]


# int ngravs_sph_density_sums(ctx, own_vel_pred, own_vel_stride, targets, nt, sums, on_device, kernel_ms)
SPH_DENSITY_SUMS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
# int ngravs_sph_hydro_sums(ctx, own, targets, nt, sums, on_device, kernel_ms)
SPH_HYDRO_SUMS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
# int64 ngravs_sph_density_update(n, sums, hsml, left, right, rounds, des, dev, minh, out, on_device)
SPH_DENSITY_UPDATE_ARGTYPES = [C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double, C.c_double,
                               C.c_void_p, C.c_int32]

GRAV_TARGET_NAMES = ("pos", "type", "old_acc", "mass")

# ---- time integration (ngravs_next_sync_point ... ngravs_advance_and_find_timesteps) ----
TIMEBASE = 1 << 28
DRIFT_TABLE_LENGTH = 1000
TIME_COL_NAMES = ("type", "pos", "vel", "mass", "ti_begstep", "ti_endstep", "grav_accel", "grav_pm", "vel_pred", "hydro_accel", "entropy",
                  "dt_entropy", "density", "hsml", "pressure", "div_vel", "max_signal_vel")
TIME_INT_COLS = ("type", "ti_begstep", "ti_endstep")
TIME_VEC_COLS = ("pos", "vel", "grav_accel", "grav_pm", "vel_pred", "hydro_accel")
TIME_PARAM_DOUBLES = ("timebase_interval", "time_begin", "time_max", "omega0", "omega_lambda", "omega_baryon", "hubble", "gamma",
                      "min_gas_hsml", "err_tol_int_accuracy", "courant_fac", "max_size_timestep", "min_size_timestep",
                      "max_rms_displacement_fac", "min_egy_spec", "timestep_scale")
TIME_PARAM_TABLES = ("drift_table", "gravkick_table", "hydrokick_table")
TIME_PARAM_INTS = ("comoving", "adaptive_gravsoft", "synchronization", "stop_below_min_timestep")


class TimeCols(C.Structure):
    """ngravs_time_cols_t"""
    _fields_ = [f for k in TIME_COL_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))] + [
        ("n", C.c_int64), ("on_device", C.c_int32), ("reserved", C.c_int32)]


class TimeParams(C.Structure):
    """ngravs_time_params_t"""
    _fields_ = [(k, C.c_double) for k in TIME_PARAM_DOUBLES] + [(k, C.c_void_p) for k in TIME_PARAM_TABLES] + [
        (k, C.c_int32) for k in TIME_PARAM_INTS]


class SyncPoint(C.Structure):
    """ngravs_sync_t"""
    _fields_ = [("ti_next", C.c_int32), ("full_step", C.c_int32), ("n_active", C.c_int64)]


def make_time_params(tables=None, **kw):
    """ngravs_time_params_t: gamma 5/3, timestep_scale 1, synchronization and stop_below_min_timestep on (the reference's
    Makefile), everything else 0 unless given by field name.  tables: (drift, gravkick, hydrokick) float64 numpy arrays of
    DRIFT_TABLE_LENGTH from Engine.time_tables / time_tables(); they are kept alive with the struct."""
    par = TimeParams()
    par.gamma, par.timestep_scale, par.synchronization, par.stop_below_min_timestep = 5.0 / 3, 1.0, 1, 1
    for k, v in kw.items():
        if k not in TIME_PARAM_DOUBLES + TIME_PARAM_INTS:
            raise TypeError("ngravs_time_params_t has no field %r" % k)
        setattr(par, k, int(v) if k in TIME_PARAM_INTS else float(v))
    if tables is not None:
        import numpy as np
        keep = [np.ascontiguousarray(t, dtype=np.float64) for t in tables]
        assert len(keep) == 3 and all(t.shape == (DRIFT_TABLE_LENGTH,) for t in keep)
        par.drift_table, par.gravkick_table, par.hydrokick_table = (t.ctypes.data for t in keep)
        par._tables = keep
    return par


GLOBAL_NSUMS = 78   # NGRAVS_GLOBAL_NSUMS: 13 sums for each of the 6 types


class SysState(C.Structure):
    """ngravs_sysstate_t: struct state_of_system of the reference (allvars.h), 119 doubles"""
    _fields_ = [(k, C.c_double) for k in ("Mass", "EnergyKin", "EnergyPot", "EnergyInt", "EnergyTot")] + [
        (k, C.c_double * 4) for k in ("Momentum", "AngMomentum", "CenterOfMass")] + [
        (k, C.c_double * 6) for k in ("MassComp", "EnergyKinComp", "EnergyPotComp", "EnergyIntComp", "EnergyTotComp")] + [
        (k, C.c_double * 4 * 6) for k in ("MomentumComp", "AngMomentumComp", "CenterOfMassComp")]


# ---- snapshot files (ngravs_snapshot_plan ... ngravs_find_next_outputtime) ----
SNAP_BLOCKS = ("POS", "VEL", "ID", "MASS", "U", "RHO", "HSML", "POT", "ACCE", "ENDT", "TSTP")   # enum iofields (allvars.h)
(SNAP_POS, SNAP_VEL, SNAP_ID, SNAP_MASS, SNAP_U, SNAP_RHO, SNAP_HSML, SNAP_POT, SNAP_ACCE, SNAP_ENDT, SNAP_TSTP) = range(11)
SNAP_LABELS = ("POS ", "VEL ", "ID  ", "MASS", "U   ", "RHO ", "HSML", "POT ", "ACCE", "ENDT", "TSTP")   # fill_Tab_IO_Labels
SNAP_VECTOR_BLOCKS = (SNAP_POS, SNAP_VEL, SNAP_ACCE)
SNAP_GAS_BLOCKS = (SNAP_U, SNAP_RHO, SNAP_HSML, SNAP_ENDT)
SNAP_ALWAYS = 0x7F   # blockpresent: POS VEL ID MASS U RHO HSML


def snap_mask(*names):
    """the blocks_mask of ngravs_snapshot_write for the optional blocks given by label: snap_mask("POT", "ACCE", "ENDT", "TSTP")"""
    m = SNAP_ALWAYS
    for k in names:
        m |= 1 << SNAP_BLOCKS.index(k.strip())
    return m


class Snapshot(C.Structure):
    """ngravs_snapshot_t"""
    _fields_ = [("ti_current", C.c_int32), ("reserved", C.c_int32), ("pm_ti", C.c_void_p), ("mass_table", C.c_double * 6),
                ("ids", C.c_void_p), ("ids_stride", C.c_int64), ("potential", C.c_void_p), ("potential_stride", C.c_int64),
                ("box_size", C.c_double), ("hubble_param", C.c_double)]


class OutputRule(C.Structure):
    """ngravs_output_rule_t"""
    _fields_ = [("output_list_on", C.c_int32), ("output_list_length", C.c_int32), ("output_list_times", C.c_void_p),
                ("time_of_first_snapshot", C.c_double), ("time_bet_snapshot", C.c_double)]


def make_output_rule(output_list=None, time_of_first_snapshot=0.0, time_bet_snapshot=0.0):
    """ngravs_output_rule_t: output_list (All.OutputListTimes; OutputListOn) or TimeOfFirstSnapshot / TimeBetSnapshot"""
    r = OutputRule()
    if output_list is not None:
        import numpy as np
        keep = np.ascontiguousarray(output_list, dtype=np.float64)
        r.output_list_on, r.output_list_length, r.output_list_times = 1, len(keep), keep.ctypes.data
        r._keep = keep
    r.time_of_first_snapshot, r.time_bet_snapshot = float(time_of_first_snapshot), float(time_bet_snapshot)
    return r


class GravTargets(C.Structure):
    """ngravs_grav_targets_t"""
    _fields_ = [f for k in GRAV_TARGET_NAMES for f in ((k, C.c_void_p), (k + "_stride", C.c_int64))] + [("on_device", C.c_int32)]


# int ngravs_gravity_tree_targets(ctx, targets, nt, acc, nint, kernel_ms)
GRAVITY_TREE_TARGETS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p, C.c_void_p]
# int ngravs_pm_targets(ctx, targets, nt, grav_pm)
PM_TARGETS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
# int ngravs_compute_potential(ctx, par, potential, potential_stride, on_device, nint)
COMPUTE_POTENTIAL_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.c_void_p]
# int ngravs_potential_targets(ctx, targets, nt, pot, nint)
POTENTIAL_TARGETS_ARGTYPES = [C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
# int ngravs_lattice_potential_table(ctx, target, source, out)
LATTICE_POTENTIAL_TABLE_ARGTYPES = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
LATTICE_ZERO = 2.8372975     # ngravs.c:133


def make_config(n_gravs=1, periodic=0, pmgrid=0, box_size=0.0, G=1.0, theta=0.5, err_tol_force_acc=0.005,
                softening=None, type_to_grav=None, wiring="newton", yukawa_imass=60.0, walk_mode=WALK_STRICT,
                tree_alloc_factor=0.0, device=0, rank=0, world_size=1, group_reach=0.0):
    """Build a Config the way init_grav_maps()+wire_grav_maps() would (ngravs_core.c:201, ngravs.c:64).

    softening: Plummer-equivalent eps per type (SofteningTable); ForceSoftening = 2.8*eps (gravtree.c:514).
    wiring: 'newton'    all pairs Newtonian            (NGRAVS_STOCK_TESTING, ngravs.c:98-146)
            'coloyuk'   all pairs Newton+Yukawa        (NGRAVS_COMBINED_TESTING_UNIFORM, ngravs.c:284-320)
            'yukawa_offdiag' diagonal none, off-diagonal Yukawa (NGRAVS_YUKAWA_FORCETEST, ngravs.c:213-283)
            'c4'        diagonal Newton, off-diagonal Newton+Yukawa (SURVEY.md 8(d) research wiring for C4/C5)
            'bam'       N_GRAVS=2: species 0 baryons, species 1 BAM (NGRAVS_ACCUMULATOR_TESTING, ngravs.c:163-210): [0][0]
                        newtonian/plummer, [0][1] sourcebambaryon, [1][0] sourcebaryonbam, [1][1] bambam; tree-only
    """
    cfg = Config()
    cfg.abi_version = ABI_VERSION
    cfg.n_gravs = n_gravs
    cfg.periodic = int(periodic)
    cfg.pmgrid = int(pmgrid)
    cfg.box_size = float(box_size)
    cfg.G = float(G)
    cfg.err_tol_theta = float(theta)
    cfg.err_tol_force_acc = float(err_tol_force_acc)
    softening = softening if softening is not None else [0.0] * NTYPES
    for t in range(NTYPES):
        cfg.force_softening[t] = 2.8 * float(softening[t])
    type_to_grav = type_to_grav if type_to_grav is not None else [0] * NTYPES
    for t in range(NTYPES):
        cfg.type_to_grav[t] = int(type_to_grav[t])
    for i in range(n_gravs):
        for j in range(n_gravs):
            if wiring == "newton":
                law, spl = LAW_NEWTON, SPLINE_PLUMMER
            elif wiring == "coloyuk":
                law, spl = LAW_COLOYUK, SPLINE_PLUMMER
            elif wiring == "yukawa_offdiag":
                law, spl = (LAW_NONE, SPLINE_NONE) if i == j else (LAW_YUKAWA, SPLINE_PLUMMER)
            elif wiring == "c4":
                law, spl = (LAW_NEWTON if i == j else LAW_COLOYUK), SPLINE_PLUMMER
            elif wiring == "bam":
                law, spl = {(0, 0): (LAW_NEWTON, SPLINE_PLUMMER), (0, 1): (LAW_SOURCEBAM, SPLINE_SOURCEBAM),
                            (1, 0): (LAW_TARGETBAM, SPLINE_TARGETBAM), (1, 1): (LAW_BAMBAM, SPLINE_BAMBAM)}[(i, j)]
            elif isinstance(wiring, dict):
                # explicit ids (built-in or LAW_USER0 + k / SPLINE_USER0 + k):
                # {"accel": [[..]], "spline": [[..]], "greens": [[..]] (default none), "normed": [[..]] (default greens)}
                law, spl = wiring["accel"][i][j], wiring["spline"][i][j]
            else:
                raise ValueError("unknown wiring %r" % wiring)
            cfg.law_accel[i][j] = law
            cfg.law_spline[i][j] = spl
            if isinstance(wiring, dict):
                none = [[LAW_NONE] * n_gravs] * n_gravs
                cfg.law_greens[i][j] = wiring.get("greens", none)[i][j]
                cfg.law_normed[i][j] = wiring.get("normed", wiring.get("greens", none))[i][j]
                continue
            cfg.law_greens[i][j] = law if wiring != "bam" else LAW_NONE
            cfg.law_normed[i][j] = law if wiring != "bam" else LAW_NONE
    cfg.yukawa_imass = float(yukawa_imass)
    cfg.tree_alloc_factor = float(tree_alloc_factor)
    cfg.group_reach = float(group_reach)
    cfg.walk_mode = int(walk_mode)
    cfg.device = int(device)
    cfg.rank = int(rank)
    cfg.world_size = int(world_size)
    return cfg
