"""Time integration on the device: ngravs_time_tables / _factors, ngravs_next_sync_point, ngravs_move_particles,
ngravs_displacement_sums, ngravs_dt_displacement, ngravs_advance_and_find_timesteps and timeline.Timeline.

The truth is the numpy restatement below of the reference's driftfac.c, predict.c, timestep.c and run.c:161-191, written from those
files (line references beside each rule), operation for operation in their order; numpy does not fuse multiply-adds.

Tolerances.  Integer columns exactly.  A row may be left out of the integer comparison only if, by the restatement's OWN values,
dt / Timebase_interval lies within 1e-10 relative of a power of two, dt within 1e-10 of MaxSizeTimestep, dt_displacement or
MinSizeTimestep, or its two candidate steps (acceleration, Courant) agree to 1e-10: at most 1 % of the active rows of a set, asserted.
Float columns: 1e-13 x the column's largest magnitude -- each output is a handful of fp64 operations and at most one exp, pow or sqrt,
a fused multiply-add against numpy is worth a few ulp (2.2e-16 each), so 1e-13 leaves two orders of magnitude.
"""
import ctypes as C
import math
import re
import types

import numpy as np
import pytest

TB = 1 << 28            # TIMEBASE (allvars.h)
LEN = 1000              # DRIFT_TABLE_LENGTH
GAMMA = 5.0 / 3
FTOL = 1e-13
NEAR = 1e-10
CAP = 0.01
COSMO = dict(eds=dict(omega0=1.0, omega_lambda=0.0), lcdm=dict(omega0=0.3, omega_lambda=0.7))
NEW = ["ngravs_time_tables", "ngravs_time_factors", "ngravs_next_sync_point", "ngravs_move_particles", "ngravs_displacement_sums",
       "ngravs_dt_displacement", "ngravs_advance_and_find_timesteps"]
VEC = ("pos", "vel", "grav_accel", "grav_pm", "vel_pred", "hydro_accel")
INTS = ("type", "ti_begstep", "ti_endstep")
GASF = ("vel_pred", "hydro_accel", "entropy", "dt_entropy", "density", "hsml", "pressure", "div_vel", "max_signal_vel")


# ---- the restatement ----------------------------------------------------------------------------------------------------
def hubble_of(P, a):
    """driftfac.c:183-184, timestep.c:53-56"""
    return P["hubble"] * np.sqrt(P["omega0"] / (a * a * a) + (1 - P["omega0"] - P["omega_lambda"]) / (a * a) + P["omega_lambda"])


def ref_tables(P, nodes):
    """driftfac.c:26-60 with the integrands of :179-212, Gauss-Legendre in log a with `nodes` nodes per table cell"""
    x, w = np.polynomial.legendre.leggauss(nodes)
    ltb, ltm = math.log(P["time_begin"]), math.log(P["time_max"])
    edges = ltb + (ltm - ltb) / LEN * np.arange(LEN + 1)
    mid, half = 0.5 * (edges[1:] + edges[:-1]), 0.5 * (edges[1:] - edges[:-1])
    a = np.exp(mid[:, None] + half[:, None] * x[None, :])
    h = hubble_of(P, a)
    f = [1 / (h * a * a * a), 1 / (h * a * a), 1 / (h * np.power(a, 3 * (P["gamma"] - 1)) * a)]
    return tuple(np.cumsum(half * np.sum(w[None, :] * g * a, axis=1)) for g in f)


def ref_factor(T, P, t0, t1):
    """get_drift_factor and its two sisters, driftfac.c:67-174, for arrays of integer times"""
    ltb, ltm, tbi = math.log(P["time_begin"]), math.log(P["time_max"]), P["timebase_interval"]

    def df(t):
        t = np.asarray(t, dtype=np.float64)
        a = ltb + t * tbi                                         # :74
        u = (a - ltb) / (ltm - ltb) * LEN                         # :77
        i = np.minimum(u.astype(np.int64), LEN - 1)               # :78-80
        j = np.maximum(i, 1)
        return np.where(i <= 1, u * T[0], T[j - 1] + (T[j] - T[j - 1]) * (u - i))   # :82-85
    return df(t1) - df(t0)                                        # :98


def ref_sync(tie, pm_end):
    """run.c:161-191"""
    mn = int(tie.min())
    full = not np.any(tie > mn)
    if pm_end is not None and mn >= pm_end:                       # :175-181
        mn, full = pm_end, True
    return mn, full, int(np.sum(tie == mn))


def ref_move(c, P, t0, t1, mesh, wrap_box=0.0):
    """predict.c:31-76, then the two while loops of :124-132 when wrap_box > 0"""
    c = {k: v.copy() for k, v in c.items()}
    if P["comoving"]:
        dd, dg, dh = (float(ref_factor(T, P, t0, t1)) for T in P["tables"])     # :42-44
    else:
        dd = dg = dh = (t1 - t0) * P["timebase_interval"]                        # :48
    c["pos"] = c["pos"] + c["vel"] * dd                                          # :54
    g = np.flatnonzero(c["type"] == 0)
    if len(g):
        acc = c["grav_accel"][g] + c["grav_pm"][g] if mesh else c["grav_accel"][g]
        c["vel_pred"][g] = c["vel_pred"][g] + (acc * dg + c["hydro_accel"][g] * dh)            # :60-64
        c["density"][g] = c["density"][g] * np.exp(-c["div_vel"][g] * dd)                      # :66
        c["hsml"][g] = np.maximum(c["hsml"][g] * np.exp(0.333333333333 * c["div_vel"][g] * dd), P["min_gas_hsml"])   # :67-70
        mid = (c["ti_begstep"][g].astype(np.int64) + c["ti_endstep"][g]) // 2
        dt_entr = (t1 - mid) * P["timebase_interval"]                                          # :72
        c["pressure"][g] = (c["entropy"][g] + c["dt_entropy"][g] * dt_entr) * np.power(c["density"][g], P["gamma"])   # :74
    if wrap_box > 0:
        x = c["pos"]
        while np.any(x < 0):
            x[x < 0] += wrap_box
        while np.any(x >= wrap_box):
            x[x >= wrap_box] -= wrap_box
    return c


def ref_factors_of_time(P, ti):
    """timestep.c:48-61"""
    if not P["comoving"]:
        return types.SimpleNamespace(fac1=1.0, fac2=1.0, fac3=1.0, hubble_a=1.0, a3inv=1.0, atime=1.0)
    t = P["time_begin"] * math.exp(ti * P["timebase_interval"])
    return types.SimpleNamespace(fac1=1 / (t * t), fac2=1 / math.pow(t, 3 * P["gamma"] - 2), fac3=math.pow(t, 3 * (1 - P["gamma"]) / 2.0),
                                 hubble_a=float(hubble_of(P, t)), a3inv=1 / (t * t * t), atime=t)


class Fatal(Exception):
    pass


def ref_get_timestep(c, P, ti, dt_disp, mesh, soft):
    """get_timestep, timestep.c:427-576, for the rows on the sync point: (rows, ti_step before the power-of-two floor, rows that may
    be left out of the integer comparison, dt / Timebase_interval)"""
    f = ref_factors_of_time(P, ti)
    act = np.flatnonzero(c["ti_endstep"] == ti)
    ty = c["type"][act]
    gas = ty == 0
    a = f.fac1 * c["grav_accel"][act]                                            # :442-444
    if mesh:
        a = a + f.fac1 * c["grav_pm"][act]                                       # :449-451
    if gas.any():
        a[gas] = a[gas] + f.fac2 * c["hydro_accel"][act][gas]                    # :456-458
    ac = np.sqrt(a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1] + a[:, 2] * a[:, 2])      # :461
    ac[ac == 0] = 1.0e-30
    ac = ac * (P["timestep_scale"] or 1.0)                                       # :493
    dt_accel = np.sqrt(2 * P["err_tol_int_accuracy"] * f.atime * soft[ty] / ac)  # :494
    nan = np.full(len(c["type"]), np.nan)
    h, msv = c.get("hsml", nan)[act], c.get("max_signal_vel", nan)[act]          # (a set without gas need not have the gas columns)
    with np.errstate(all="ignore"):
        if P["adaptive_gravsoft"]:
            dt_accel = np.where(gas, np.sqrt(2 * P["err_tol_int_accuracy"] * f.atime * h / 2.8 / ac), dt_accel)   # :497-499
        if P["comoving"]:
            dt_courant = 2 * P["courant_fac"] * f.atime * h / (f.fac3 * msv)     # :512
        else:
            dt_courant = 2 * P["courant_fac"] * h / msv                          # :514
    dt = np.where(gas & (dt_courant < dt_accel), dt_courant, dt_accel)           # :516-517
    dt = dt * f.hubble_a                                                         # :523
    dt0 = dt.copy()
    dt = np.where(dt >= P["max_size_timestep"], P["max_size_timestep"], dt)      # :525
    dt = np.where(dt >= dt_disp, dt_disp, dt)                                    # :528
    low = dt < P["min_size_timestep"]                                            # :531
    bad888 = low & bool(P["stop_below_min_timestep"])
    dt = np.where(low, P["min_size_timestep"], dt)                               # :553
    q = dt / P["timebase_interval"]                                              # :556
    bad818 = ~bad888 & ~((q >= 1) & (q < TB))                                    # :558
    if bad888.any() or bad818.any():
        first = int(np.flatnonzero(bad888 | bad818)[0])
        raise Fatal(888 if bad888[first] else 818, int(act[first]))
    # rows whose integers rounding may decide
    near = np.zeros(len(act), dtype=bool)
    p2 = 2.0 ** np.round(np.log2(q))
    near |= (np.abs(q / p2 - 1) < NEAR) & (dt == dt0)             # (a row that took a limit holds the limit's own quotient: one division)
    for lim in (P["max_size_timestep"], dt_disp, P["min_size_timestep"]):
        if lim > 0:
            near |= np.abs(dt0 / lim - 1) < NEAR
    with np.errstate(all="ignore"):
        near |= gas & (np.abs(dt_courant / dt_accel - 1) < NEAR)
    return act, q.astype(np.int64), near, q


def ref_advance(c, P, ti, dt_disp, mesh, soft, pm_ti=None):
    """advance_and_find_timesteps, timestep.c:24-413: (the columns afterwards, pm_ti afterwards, the rows that may be left out of
    the integer comparison, the active rows, dt / Timebase_interval of the active rows)"""
    c = {k: v.copy() for k, v in c.items()}
    tbi, comoving = P["timebase_interval"], P["comoving"]
    f = ref_factors_of_time(P, ti)
    act, ti_step, near, q = ref_get_timestep(c, P, ti, dt_disp, mesh, soft)
    gk = (lambda t0, t1: ref_factor(P["tables"][1], P, t0, t1)) if comoving else None
    hk = (lambda t0, t1: ref_factor(P["tables"][2], P, t0, t1)) if comoving else None
    if mesh:                                                                     # :70-76
        pmb, pme = pm_ti
        dt_gravkickB = float(gk(pmb, ti) - gk(pmb, (pmb + pme) // 2)) if comoving else (ti - (pmb + pme) // 2) * tbi
    beg, end = c["ti_begstep"][act].astype(np.int64), c["ti_endstep"][act].astype(np.int64)
    ti_step = 1 << (np.frexp(ti_step.astype(np.float64))[1].astype(np.int64) - 1)              # :190-194
    if P["synchronization"]:                                                     # :240-246
        keep = (ti_step > end - beg) & (((TB - end) % ti_step) > 0)
        ti_step = np.where(keep, end - beg, ti_step)
    if ti == TB:                                                                 # :249
        ti_step = np.zeros_like(ti_step)
    ti_step = np.where(TB - ti < ti_step, TB - ti, ti_step)                      # :252
    tstart, tend = (beg + end) // 2, end + ti_step // 2                          # :255-256
    if comoving:                                                                 # :258-271
        dt_entr = (tend - tstart) * tbi
        dt_gravkick, dt_hydrokick = gk(tstart, tend), hk(tstart, tend)
        dt_gravkick2, dt_hydrokick2 = gk(end, tend), hk(end, tend)
    else:
        dt_entr = dt_gravkick = dt_hydrokick = (tend - tstart) * tbi
        dt_gravkick2 = dt_hydrokick2 = (tend - end) * tbi
    c["ti_begstep"][act] = end                                                   # :273-274
    c["ti_endstep"][act] = end + ti_step
    c["vel"][act] = c["vel"][act] + c["grav_accel"][act] * dt_gravkick[:, None]  # :281-282
    g = c["type"][act] == 0
    r = act[g]
    if len(r):
        ga, ha = c["grav_accel"][r], c["hydro_accel"][r]
        c["vel"][r] = c["vel"][r] + ha * dt_hydrokick[g, None]                   # :290
        vp = c["vel"][r] - dt_gravkick2[g, None] * ga - dt_hydrokick2[g, None] * ha            # :292-293
        if mesh:
            vp = vp + c["grav_pm"][r] * dt_gravkickB                             # :295
        c["vel_pred"][r] = vp
        A, dA = c["entropy"][r], c["dt_entropy"][r]
        A = np.where(dA * dt_entr[g] > -0.5 * A, A + dA * dt_entr[g], A * 0.5)   # :302-305
        if P["min_egy_spec"]:                                                    # :307-315
            minent = P["min_egy_spec"] * (P["gamma"] - 1) / np.power(c["density"][r] * f.a3inv, P["gamma"] - 1)
            dA = np.where(A < minent, 0.0, dA)
            A = np.where(A < minent, minent, A)
        dt2 = (ti_step[g] // 2) * tbi                                            # :323
        with np.errstate(all="ignore"):
            dA = np.where(A + dA * dt2 < 0.5 * A, -0.5 * A / dt2, dA)            # :324-325
        c["entropy"][r], c["dt_entropy"][r] = A, dA
    if mesh and pm_ti[1] == ti:                                                  # :351-408
        pmb, pme = pm_ti
        s = TB
        while s > 0 and s > dt_disp / tbi:
            s >>= 1
        if s > pme - pmb and s > 0 and ((TB - pme) % s) > 0:
            s = pme - pmb
        if ti == TB:
            s = 0
        tstart, tend = (pmb + pme) // 2, pme + s // 2
        dt_gk = float(gk(tstart, tend)) if comoving else (tend - tstart) * tbi
        pm_ti = [pme, pme + s]
        mid = (pm_ti[0] + pm_ti[1]) // 2
        dtB = -float(gk(pm_ti[0], mid)) if comoving else -(mid - pm_ti[0]) * tbi
        c["vel"] = c["vel"] + c["grav_pm"] * dt_gk                               # :387
        r = np.flatnonzero(c["type"] == 0)
        if len(r):
            b, e = c["ti_begstep"][r].astype(np.int64), c["ti_endstep"][r].astype(np.int64)
            if comoving:                                                         # :393-396
                dtA = gk(b, ti) - gk(b, (b + e) // 2)
                dth = hk(b, ti) - hk(b, (b + e) // 2)
            else:
                dtA = dth = (ti - (b + e) // 2) * tbi
            c["vel_pred"][r] = c["vel"][r] + c["grav_accel"][r] * dtA[:, None] + c["hydro_accel"][r] * dth[:, None] + c["grav_pm"][r] * dtB
    return c, pm_ti, act[near], act, q


def ref_dt_displacement(P, sums, G, asmth, time):
    """timestep.c:595-659"""
    dt_disp = P["max_size_timestep"]
    if P["comoving"]:
        hfac = float(hubble_of(P, time)) * time * time
        for t in range(6):
            if sums[12 + t] > 0:
                om = P["omega_baryon"] if t == 0 else P["omega0"] - P["omega_baryon"]
                dmean = math.pow(sums[6 + t] / (om * 3 * P["hubble"] * P["hubble"] / (8 * math.pi * G)), 1.0 / 3)
                dt = P["max_rms_displacement_fac"] * hfac * dmean / math.sqrt(sums[t] / sums[12 + t])
                if asmth > 0 and asmth < dmean:
                    dt = P["max_rms_displacement_fac"] * hfac * asmth / math.sqrt(sums[t] / sums[12 + t])
                dt_disp = min(dt, dt_disp)
    return dt_disp


def ref_sums(c):
    """timestep.c:606-612"""
    out = np.zeros(18)
    for t in range(6):
        m = c["type"] == t
        out[t] = np.sum(np.sum(c["vel"][m] ** 2, axis=1))
        out[6 + t] = c["mass"][m].min() if m.any() else 1.0e30
        out[12 + t] = m.sum()
    return out


# ---- parameters and sets --------------------------------------------------------------------------------------------------
def params(comoving, cosmo="lcdm", **kw):
    P = dict(timebase_interval=(math.log(10.0) if comoving else 1.0) / TB, time_begin=0.1 if comoving else 0.0,
             time_max=1.0, omega0=0.3, omega_lambda=0.7, omega_baryon=0.04, hubble=0.1, gamma=GAMMA, min_gas_hsml=0.0,
             err_tol_int_accuracy=0.025, courant_fac=0.15, max_size_timestep=0.01, min_size_timestep=1e-7, max_rms_displacement_fac=0.2,
             min_egy_spec=0.0, timestep_scale=1.0, comoving=int(comoving), adaptive_gravsoft=0, synchronization=1,
             stop_below_min_timestep=1, tables=None)
    P.update(COSMO[cosmo])
    P.update(kw)
    if comoving:
        P["tables"] = ref_tables(P, 24)
    return P


def c_params(pkg, P):
    return pkg.abi.make_time_params(tables=P["tables"], **{k: v for k, v in P.items() if k != "tables"})


SOFT = np.array([0.02, 0.05, 0.03, 0.05, 0.04, 0.05])   # All.SofteningTable[]
BOX = 100.0
TI = 3 << 22                                             # All.Ti_Current of the sets
STEP_A, STEP_B = 1 << 17, 1 << 19                        # the two populated rungs


def engine(pkg, mesh, G=1.0):
    cfg = pkg.make_config(n_gravs=1, periodic=1, pmgrid=16 if mesh else 0, box_size=BOX, G=G, softening=list(SOFT))
    return pkg.Engine(cfg)


def make_set(n, seed, P, mesh):
    """types 0-5 mixed with about 40 % gas; one third of the rows on the rung that ends at TI, the others half-way through a longer
    step; seeded accelerations over three decades, scaled so that the median step lands near 2^17.5 ticks (the criterion spans more
    than four powers of two, asserted); a Courant step within a factor three of the acceleration step; NaN in the gas columns of the
    rows of other types"""
    rng = np.random.default_rng(seed)
    c = {}
    c["type"] = np.where(rng.uniform(size=n) < 0.4, 0, rng.integers(1, 6, n)).astype(np.int32)
    if n >= 6:
        c["type"][:6] = np.arange(6)
    gas = c["type"] == 0
    c["pos"] = rng.uniform(0, BOX, (n, 3))
    c["vel"] = rng.normal(0, 3.0, (n, 3))
    c["mass"] = rng.uniform(1.0, 2.0, n)
    act = rng.uniform(size=n) < 1.0 / 3
    act[0] = True
    c["ti_endstep"] = np.where(act, TI, TI + STEP_B // 2).astype(np.int32)
    c["ti_begstep"] = np.where(act, TI - STEP_A, TI - STEP_B // 2).astype(np.int32)

    def vec(lo, hi):
        d = rng.normal(size=(n, 3))
        return d / np.linalg.norm(d, axis=1)[:, None] * (10.0 ** rng.uniform(lo, hi, n))[:, None]
    c["grav_accel"], c["grav_pm"], c["hydro_accel"] = vec(0, 3), vec(-1, 2), vec(-1, 2)
    c["vel_pred"] = c["vel"] + rng.normal(0, 0.1, (n, 3))
    c["entropy"] = 10.0 ** rng.uniform(-0.5, 0.5, n)
    c["dt_entropy"] = c["entropy"] * rng.uniform(-1, 1, n) * 0.2 / (STEP_A * P["timebase_interval"])
    c["density"] = 10.0 ** rng.uniform(-1, 1, n)
    c["hsml"] = rng.uniform(0.5, 2.0, n)
    c["pressure"] = c["entropy"] * c["density"] ** GAMMA
    c["div_vel"] = rng.normal(0, 1.0, n) / (STEP_B * P["timebase_interval"]) * 0.1
    c["max_signal_vel"] = np.ones(n)
    # scale the accelerations: dt goes as 1 / sqrt(ac)
    big = dict(P, max_size_timestep=1e30, min_size_timestep=0.0, stop_below_min_timestep=0)
    _, _, _, q = ref_get_timestep(dict(c, max_signal_vel=np.full(n, 1e-300)), big, TI, 1e30, mesh, SOFT)
    s = (np.median(q) / 2.0 ** 17.5) ** 2
    for k in ("grav_accel", "grav_pm", "hydro_accel"):
        c[k] = c[k] * s
    f = ref_factors_of_time(P, TI)
    a = f.fac1 * (c["grav_accel"] + (c["grav_pm"] if mesh else 0)) + f.fac2 * c["hydro_accel"]
    dt_accel = np.sqrt(2 * P["err_tol_int_accuracy"] * f.atime * SOFT[c["type"]] / np.linalg.norm(a, axis=1))
    c["max_signal_vel"] = 2 * P["courant_fac"] * c["hsml"] * (f.atime / f.fac3 if P["comoving"] else 1.0) / (dt_accel * 10.0 ** rng.uniform(-0.5, 0.5, n))
    for k in GASF:
        c[k][~gas] = np.nan
    return c


def copy_of(c):
    return {k: v.copy() for k, v in c.items()}


def assert_float(got, want, what):
    scale = np.nanmax(np.abs(want)) if np.isfinite(want).any() else 0.0
    both_nan = np.isnan(got) & np.isnan(want)
    err = np.where(both_nan, 0.0, np.abs(got - want))
    assert not np.isnan(err).any(), what
    worst = err.max() / scale if scale > 0 else err.max()
    print("%-40s max deviation / max magnitude = %.3g" % (what, worst))
    assert worst <= FTOL, (what, worst)
    return worst


def assert_state(got, want, skip_rows, n_active, what):
    """floats to FTOL, integers exactly except the rows the restatement itself cannot decide (at most CAP of the active rows; their
    kicks follow their step, so they are left out of the float columns too)"""
    assert len(skip_rows) <= max(CAP * n_active, 0), (what, len(skip_rows), n_active)
    keep = np.ones(len(want["type"]), dtype=bool)
    keep[skip_rows] = False
    for k in want:
        if k in INTS:
            assert np.array_equal(got[k][keep], want[k][keep]), (what, k)
        else:
            assert_float(got[k][keep], want[k][keep], what + " " + k)


def handler(pkg, eng):
    seen = []
    fn = C.CFUNCTYPE(None, C.c_int, C.c_char_p)(lambda code, msg: seen.append((code, msg.decode())))
    pkg.lib().ngravs_set_fatal_handler.argtypes = [C.c_void_p, C.c_void_p]
    pkg.lib().ngravs_set_fatal_handler(eng._h, C.cast(fn, C.c_void_p))
    eng._fatal_keep = fn
    return seen


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_exported_declared_and_laid_out_as_the_header_says(pkg, have_lib):
    for name in NEW:
        assert name in pkg.EXPORTS and hasattr(have_lib, name), name
    root = pkg.__file__.replace("gadget-2.0.7-ngravs_amd/__init__.py", "")
    hdr = open(root + "include/ngravs_hip.h").read()
    for name in NEW:
        assert "int %s(" % name in hdr
    for cname, cls in (("ngravs_time_cols_t", pkg.abi.TimeCols), ("ngravs_time_params_t", pkg.abi.TimeParams), ("ngravs_sync_t", pkg.abi.SyncPoint)):
        body = hdr[:hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
        names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    # 17 pointer + stride pairs, n, two ints; 16 doubles, 3 pointers, 4 ints; two ints and a count
    assert C.sizeof(pkg.abi.TimeCols) == 288 and C.sizeof(pkg.abi.TimeParams) == 168 and C.sizeof(pkg.abi.SyncPoint) == 16
    capi = open(root + "gadget-2.0.7-ngravs_amd/csrc/capi.hip").read()
    assert "static_assert(sizeof(ngravs_time_cols_t) == 288 && sizeof(ngravs_time_params_t) == 168 && sizeof(ngravs_sync_t) == 16" in capi
    assert pkg.abi.TIMEBASE == TB and pkg.abi.DRIFT_TABLE_LENGTH == LEN
    assert "#define NGRAVS_TIMEBASE (1 << 28)" in hdr and "#define NGRAVS_DRIFT_TABLE_LENGTH 1000" in hdr
    assert have_lib.ngravs_abi_version() == 3
    L = have_lib
    assert L.ngravs_time_tables(None, 0, None, None, None) == -1
    assert L.ngravs_time_factors(None, 0, 0, None) == -1
    assert L.ngravs_next_sync_point(None, None, -1, None) == -1
    assert L.ngravs_move_particles(None, None, None, 0, 0, 0) == -1
    assert L.ngravs_displacement_sums(None, None, None) == -1
    assert L.ngravs_dt_displacement(None, None, 1.0, 0.0, 1.0, None) == -1
    assert L.ngravs_advance_and_find_timesteps(None, None, None, 0, 0.0, None, None) == -1
    assert hasattr(pkg, "timeline") and hasattr(pkg.timeline, "Timeline")
    for m in ("time_tables", "next_sync_point", "move_particles", "displacement_sums", "dt_displacement", "advance_and_find_timesteps"):
        assert hasattr(pkg.Engine, m), m


@pytest.mark.parametrize("cosmo", ["eds", "lcdm"])
def test_tables(pkg, have_lib, cosmo):
    P = params(True, cosmo)
    par = c_params(pkg, dict(P, tables=None))
    lib0, lib1 = pkg.time_tables(par, 0), pkg.time_tables(par, 1)
    fine = ref_tables(P, 96)                                      # 8 x the library's 12 nodes per cell
    for name, a, b, f in zip(("drift", "gravkick", "hydrokick"), lib0, lib1, fine):
        print(cosmo, name, "against 96 nodes %.3g, rule 0 against rule 1 %.3g" % (np.max(np.abs(a / f - 1)), np.max(np.abs(a / b - 1))))
        assert np.max(np.abs(a / f - 1)) < 1e-10
        assert np.max(np.abs(a / b - 1)) < 1e-12
    if cosmo == "eds":
        # H = H0 a^-3/2: the drift integrand is a^-3/2 / H0
        a1 = np.exp(math.log(P["time_begin"]) + (math.log(P["time_max"]) - math.log(P["time_begin"])) / LEN * np.arange(1, LEN + 1))
        exact = 2 / P["hubble"] * (P["time_begin"] ** -0.5 - a1 ** -0.5)
        assert np.max(np.abs(lib0[0] / exact - 1)) < 1e-10
    with pytest.raises(pkg.NgravsError):
        pkg.time_tables(par, 2)


@pytest.mark.parametrize("cosmo", ["eds", "lcdm"])
def test_factors_are_the_lookup_of_driftfac(pkg, have_lib, cosmo):
    P = params(True, cosmo)
    par = c_params(pkg, dict(P, tables=None))
    P["tables"] = pkg.time_tables(par, 0)
    par = c_params(pkg, P)
    rng = np.random.default_rng(5)
    cell = TB // LEN
    t0 = np.concatenate([[0, 0, 0, 1, cell // 2, cell, cell + 7, 2 * cell - 1, 2 * cell, TB - cell, TB - 1, 0],
                         rng.integers(0, TB, 188)]).astype(np.int64)
    t1 = np.concatenate([[0, 1, cell, cell // 3, 2 * cell - 1, 2 * cell + 1, 3 * cell, TB, TB, TB, TB, TB], rng.integers(0, TB + 1, 188)]).astype(np.int64)
    t0, t1 = np.minimum(t0, t1), np.maximum(t0, t1)
    assert len(t0) == 200
    worst = 0.0
    for a, b in zip(t0, t1):
        got = pkg.time_factors(par, int(a), int(b))
        for k in range(3):
            want = float(ref_factor(P["tables"][k], P, a, b))
            assert abs(got[k] - want) <= 1e-15 * abs(want), (a, b, k, got[k], want)
            worst = max(worst, abs(got[k] - want) / abs(want) if want else 0.0)
    print("largest relative deviation", worst)


def test_dt_displacement(pkg, have_lib):
    G = 43007.1
    P = params(True)
    base = np.zeros(18)
    base[6:12] = 1.0e30
    sets = []
    s = base.copy(); s[1], s[7], s[13] = 5.0e8, 0.9, 1000; sets.append((s, 0.0))                       # one type, the others empty
    s = base.copy(); s[0], s[6], s[12] = 4.0e8, 0.13, 500; s[1], s[7], s[13] = 5.0e8, 0.9, 1000; sets.append((s, 0.0))   # gas: OmegaBaryon
    s = s.copy(); sets.append((s, 10.0))                                                               # Asmth < dmean with a mesh
    sets.append((s.copy(), 0.0))                                                                       # ... and the same without
    s = s.copy(); sets.append((s, 1.0e6))                                                              # a mesh with Asmth > dmean
    s = base.copy(); s[:6], s[6:12], s[12:] = 1.0e-4, 1.0, 10; sets.append((s, 0.0))                   # slow: MaxSizeTimestep stays
    par = c_params(pkg, dict(P, tables=None, comoving=1))
    seen = set()
    for sums, asmth in sets:
        for time in (0.1, 0.7):
            got = pkg.dt_displacement(par, sums, G, asmth, time)
            want = ref_dt_displacement(P, sums, G, asmth, time)
            assert abs(got - want) <= 1e-15 * want, (sums, asmth, got, want)
            seen.add(round(math.log(got), 6))
    assert len(seen) >= 6                                          # the sets do exercise different rules
    assert pkg.dt_displacement(par, sets[2][0], G, 10.0, 0.1) < pkg.dt_displacement(par, sets[3][0], G, 0.0, 0.1)
    par = c_params(pkg, params(False))
    assert pkg.dt_displacement(par, sets[1][0], G, 0.0, 0.0) == 0.01   # no comoving integration: MaxSizeTimestep


def test_sets_stay_within_the_cap_by_the_restatement_alone():
    """the seeds of the GPU tests: the rows the restatement cannot decide, and the span of the criterion"""
    for n, seed, comoving, mesh in ALL_SETS:
        P = params(comoving)
        c = make_set(n, seed, P, mesh)
        _, _, near, act, q = ref_advance(c, P, TI, DT_DISP, mesh, SOFT, [TI - (1 << 20), TI] if mesh else None)
        assert len(near) <= CAP * len(act), (n, seed, len(near))
        if n >= 1000:
            assert np.log2(q.max() / q.min()) >= 4, (n, seed)
            assert len(np.unique(c["ti_endstep"])) == 2 and abs(len(act) / n - 1 / 3) < 0.05


DT_DISP = 0.008
SIZES = (1, 63, 65, 1037)
MODES = [(False, False), (False, True), (True, False), (True, True)]      # (comoving, mesh)
ALL_SETS = [(n, 100 + n, cm, mesh) for n in SIZES for cm, mesh in MODES]


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("comoving,mesh", MODES)
def test_move_and_advance_on_the_sets(pkg, comoving, mesh):
    eng = engine(pkg, mesh)
    P = params(comoving)
    par = c_params(pkg, P)
    for n in SIZES:
        c0 = make_set(n, 100 + n, P, mesh)
        # sync point and sums
        for pm_end in (None, TI - 5, TI, TI + 5):
            assert eng.next_sync_point(c0["ti_endstep"], pm_end) == ref_sync(c0["ti_endstep"], pm_end), (n, pm_end)
        got, want = eng.displacement_sums(c0["type"], c0["vel"], c0["mass"]), ref_sums(c0)
        assert np.array_equal(got[6:], want[6:]) and np.all(np.abs(got[:6] - want[:6]) <= FTOL * np.abs(want[:6]))
        # move: TI - STEP_A / 2 -> TI, every column
        c = copy_of(c0)
        eng.move_particles(c, par, TI - STEP_A // 2, TI)
        want = ref_move(c0, P, TI - STEP_A // 2, TI, mesh)
        assert_state(c, want, [], 0, "move n=%d" % n)
        assert all(np.isnan(c[k][c0["type"] != 0]).all() for k in GASF)
        # advance, without and with the long-range kick
        for pm_ti in ([TI - (1 << 20), TI + (1 << 20)], [TI - (1 << 20), TI]) if mesh else (None,):
            c = copy_of(c0)
            kicked, pm_new = eng.advance_and_find_timesteps(c, par, TI, DT_DISP, pm_ti)
            want, pm_want, near, act, _ = ref_advance(c0, P, TI, DT_DISP, mesh, SOFT, pm_ti)
            assert kicked == len(act) and pm_new == pm_want
            assert_state(c, want, near, len(act), "advance n=%d pm=%s" % (n, pm_ti))
            idle = c0["ti_endstep"] != TI
            if not (mesh and pm_ti[1] == TI):
                for k in c0:
                    assert np.array_equal(c[k][idle], c0[k][idle], equal_nan=True), k     # inactive rows: the same bits
            else:
                assert np.all(c["vel"] != c0["vel"]) and np.all((c["vel_pred"] != c0["vel_pred"])[c0["type"] == 0])
                for k in ("ti_begstep", "ti_endstep", "entropy", "dt_entropy", "pos", "grav_accel"):
                    assert np.array_equal(c[k][idle], c0[k][idle], equal_nan=True), k


@pytest.mark.gpu
def test_wrap(pkg):
    eng = engine(pkg, False)
    P = params(False)
    c = make_set(1037, 7, P, False)
    c["pos"] = np.random.default_rng(8).uniform(-3 * BOX, 4 * BOX, (1037, 3))
    c["pos"][0] = [-3 * BOX, 0.0, BOX]
    c0 = copy_of(c)
    eng.move_particles(c, c_params(pkg, P), TI, TI + 1000, wrap=True)
    want = ref_move(c0, P, TI, TI + 1000, False, wrap_box=BOX)
    assert np.all((c["pos"] >= 0) & (c["pos"] < BOX))
    assert_float(c["pos"], want["pos"], "wrapped pos")
    c = copy_of(c0)
    eng.move_particles(c, c_params(pkg, P), TI, TI + 1000, wrap=False)
    assert_float(c["pos"], ref_move(c0, P, TI, TI + 1000, False)["pos"], "unwrapped pos")


@pytest.mark.gpu
@pytest.mark.parametrize("what", ["end_of_line", "past_the_end", "entropy_guards", "adaptive", "scale4", "nosync"])
def test_advance_cases(pkg, what):
    mesh, n = False, 257
    kw = dict(adaptive=dict(adaptive_gravsoft=1), scale4=dict(timestep_scale=4.0), nosync=dict(synchronization=0),
              entropy_guards=dict(min_egy_spec=2.0)).get(what, {})
    P = params(what == "entropy_guards", **kw)
    eng = engine(pkg, mesh)
    c0 = make_set(n, 300, P, mesh)
    ti = TI
    if what == "end_of_line":
        ti = TB
        c0["ti_endstep"][c0["ti_endstep"] == TI] = TB
        c0["ti_begstep"][c0["ti_endstep"] == TB] = TB - STEP_A
    elif what == "past_the_end":
        ti = TB - (1 << 10)                                        # every step wanted is longer than what is left
        act = c0["ti_endstep"] == TI
        c0["ti_endstep"][act], c0["ti_begstep"][act] = ti, ti - (1 << 10)
        c0["ti_endstep"][~act] = TB
    elif what == "entropy_guards":
        gas = np.flatnonzero((c0["type"] == 0) & (c0["ti_endstep"] == TI))
        assert len(gas) >= 30
        dt = STEP_A * P["timebase_interval"]
        c0["dt_entropy"][gas[:10]] = -5.0 * c0["entropy"][gas[:10]] / dt          # the factor-0.5 guard
        c0["dt_entropy"][gas[10:20]] = -0.2 * c0["entropy"][gas[10:20]] / dt      # the over-cooling limit of a longer new step
        c0["entropy"][gas[20:30]] *= 1e-6                                         # MinEgySpec
        c0["dt_entropy"][gas[20:30]] = -1e-3 * c0["entropy"][gas[20:30]] / dt
    if what == "nosync":
        ti = TI + (1 << 12)                                       # a sync point no longer step ends on: SYNCHRONIZATION keeps the old step
        act = c0["ti_endstep"] == TI
        c0["ti_endstep"][act], c0["ti_begstep"][act] = ti, ti - (1 << 12)
    c = copy_of(c0)
    kicked, _ = eng.advance_and_find_timesteps(c, c_params(pkg, P), ti, DT_DISP)
    want, _, near, act, q = ref_advance(c0, P, ti, DT_DISP, mesh, SOFT)
    assert kicked == len(act) > 0
    assert_state(c, want, near, len(act), what)
    step = (want["ti_endstep"] - want["ti_begstep"])[act]
    if what == "end_of_line":
        assert np.all(step == 0)
    elif what == "past_the_end":
        assert np.all(step == 1 << 10) and np.all(c["ti_endstep"][act] == TB)
    elif what == "entropy_guards":
        assert np.all(want["entropy"][gas[:10]] == 0.5 * c0["entropy"][gas[:10]])
        assert np.any(want["dt_entropy"][gas[10:20]] != c0["dt_entropy"][gas[10:20]])
        assert np.all(want["dt_entropy"][gas[20:30]] == 0) and np.all(want["entropy"][gas[20:30]] > c0["entropy"][gas[20:30]])
    elif what == "nosync":
        assert np.all(step > 1 << 12)
        c2 = copy_of(c0)
        eng.advance_and_find_timesteps(c2, c_params(pkg, dict(P, synchronization=1)), ti, DT_DISP)
        assert np.all((c2["ti_endstep"] - c2["ti_begstep"])[act] == 1 << 12)
    elif what == "scale4":
        _, _, _, _, q1 = ref_advance(c0, dict(P, timestep_scale=1.0), ti, DT_DISP, mesh, SOFT)
        assert np.any(q < 0.51 * q1)


@pytest.mark.gpu
def test_fatal_cases_and_refusals_write_nothing(pkg):
    eng = engine(pkg, True)
    seen = handler(pkg, eng)
    P = params(False)
    c0 = make_set(257, 300, P, True)
    pm_ti = [TI - (1 << 20), TI]
    act = np.flatnonzero(c0["ti_endstep"] == TI)

    def unchanged(c):
        return all(np.array_equal(c[k], c0[k], equal_nan=True) for k in c0)
    # below MinSizeTimestep: 888 names the lowest failing row; with the switch off the row gets MinSizeTimestep
    c = copy_of(c0)
    c["grav_accel"][act[3]] *= 1e12
    c["grav_accel"][act[7]] *= 1e12
    c0 = copy_of(c)
    with pytest.raises(pkg.NgravsError):
        eng.advance_and_find_timesteps(c, c_params(pkg, P), TI, DT_DISP, pm_ti)
    assert seen[-1][0] == 888 and "row %d" % act[3] in seen[-1][1] and unchanged(c)
    P0 = dict(P, stop_below_min_timestep=0)
    eng.advance_and_find_timesteps(c, c_params(pkg, P0), TI, DT_DISP, pm_ti)
    want, _, near, _, _ = ref_advance(c0, P0, TI, DT_DISP, True, SOFT, pm_ti)
    assert_state(c, want, near, len(act), "MinSizeTimestep")
    assert (c["ti_endstep"] - c["ti_begstep"])[act[3]] == 1 << int(math.log2(1e-7 * TB))
    # a zero MaxSizeTimestep: 818
    c = copy_of(c0)
    with pytest.raises(pkg.NgravsError):
        eng.advance_and_find_timesteps(c, c_params(pkg, dict(P0, max_size_timestep=0.0, min_size_timestep=0.0)), TI, DT_DISP, pm_ti)
    assert seen[-1][0] == 818 and "row %d" % act[0] in seen[-1][1] and unchanged(c)
    # a quotient no int holds: 818, not undefined behaviour
    c = copy_of(c0)
    with pytest.raises(pkg.NgravsError):
        eng.advance_and_find_timesteps(c, c_params(pkg, dict(P0, max_size_timestep=1e30, timebase_interval=1e-30)), TI, 1e30, pm_ti)
    assert seen[-1][0] == 818 and unchanged(c)
    # refusals
    par = c_params(pkg, P)
    n_seen = len(seen)

    def refused(fn, *a, **k):
        with pytest.raises(pkg.NgravsError) as e:
            fn(*a, **k)
        assert "status -1" in str(e.value), str(e.value)
    for call, args in ((eng.advance_and_find_timesteps, (TI, DT_DISP, pm_ti)), (eng.move_particles, (TI, TI + 10))):
        c = copy_of(c0)
        c["type"][5] = 6
        keep = c["type"].copy()
        refused(call, c, par, *args)                                                             # a type outside 0..5
        c["type"][5] = c0["type"][5]
        assert unchanged(c) and keep[5] == 6
        refused(call, {k: v for k, v in c.items() if k != "hydro_accel"}, par, *args)            # a gas column missing, gas present
        refused(call, {k: v for k, v in c.items() if k != "vel"}, par, *args)                    # a required column
        refused(call, {k: v for k, v in c.items() if k != "grav_pm"}, par, *args)                # ... which GravPM is with a mesh
        refused(call, c, c_params(pkg, dict(P, timebase_interval=0.0)), *args)
        refused(call, c, c_params(pkg, dict(P, gamma=0.9)), *args)
        refused(call, c, c_params(pkg, dict(P, comoving=1)), *args)                              # comoving without tables
        assert unchanged(c)
    refused(eng.move_particles, c, par, TI, TI - 1)                                              # time1 < time0
    refused(eng.advance_and_find_timesteps, c, par, TI, DT_DISP, None)                           # a mesh, no PM step
    c["type"][5] = -1
    refused(eng.displacement_sums, c["type"], c["vel"], c["mass"])
    c["type"][5] = c0["type"][5]
    assert unchanged(c) and len(seen) > n_seen
    # without gas rows the gas columns are not needed
    nogas = {k: v[c0["type"] != 0].copy() for k, v in c0.items() if k not in GASF}
    eng.move_particles(nogas, par, TI, TI + 10)
    eng.advance_and_find_timesteps(nogas, c_params(pkg, P0), TI, DT_DISP, pm_ti)


@pytest.mark.gpu
def test_device_tensors_give_the_host_result_bit_for_bit(pkg):
    import torch
    for comoving, mesh in ((False, False), (True, True)):
        eng = engine(pkg, mesh)
        P = params(comoving)
        par = c_params(pkg, P)
        c0 = make_set(1037, 1137, P, mesh)
        pm_ti = [TI - (1 << 20), TI] if mesh else None
        h, d = copy_of(c0), {k: torch.from_numpy(v).cuda() for k, v in c0.items()}
        assert eng.next_sync_point(h["ti_endstep"], TI) == eng.next_sync_point(d["ti_endstep"], TI)
        assert np.array_equal(eng.displacement_sums(h["type"], h["vel"], h["mass"]), eng.displacement_sums(d["type"], d["vel"], d["mass"]))
        for c in (h, d):
            eng.move_particles(c, par, TI - 999, TI, wrap=True)
            eng.advance_and_find_timesteps(c, par, TI, DT_DISP, pm_ti)
        for k in h:
            assert np.array_equal(h[k], d[k].cpu().numpy(), equal_nan=True), k
        assert not np.array_equal(h["vel"], c0["vel"])


@pytest.mark.gpu
def test_c_abi_with_an_interleaved_layout_gives_the_same_bits(pkg):
    """P[] and SphP[] as arrays of structs, through the raw C ABI"""
    P = params(True)
    eng = engine(pkg, True)
    par = c_params(pkg, P)
    n = 1037
    c0 = make_set(n, 1137, P, True)
    pm_ti = [TI - (1 << 20), TI]
    ref = copy_of(c0)
    eng.move_particles(ref, par, TI - 999, TI, wrap=True)
    eng.advance_and_find_timesteps(ref, par, TI, DT_DISP, pm_ti)
    fields = [(k, np.int32 if k in INTS else np.float64, (3,) if k in VEC else ()) for k in c0]
    rec = np.zeros(n, dtype=np.dtype([("pad0", np.float64)] + fields + [("pad1", np.int32, (3,))], align=True))
    for k in c0:
        rec[k] = c0[k]
    tc = pkg.abi.TimeCols()
    for k in c0:
        setattr(tc, k, rec.ctypes.data + rec.dtype.fields[k][1])
        setattr(tc, k + "_stride", rec.dtype.itemsize)
    tc.n = n
    L = pkg.lib()
    assert rec.dtype.itemsize not in (8, 24)
    assert L.ngravs_move_particles(eng._h, C.byref(tc), C.byref(par), TI - 999, TI, 1) == 0
    pm = (C.c_int32 * 2)(*pm_ti)
    kicked = C.c_int64(0)
    assert L.ngravs_advance_and_find_timesteps(eng._h, C.byref(tc), C.byref(par), TI, DT_DISP, pm, C.byref(kicked)) == 0
    out = pkg.abi.SyncPoint()
    assert L.ngravs_next_sync_point(eng._h, C.byref(tc), -1, C.byref(out)) == 0
    assert (out.ti_next, bool(out.full_step), out.n_active) == ref_sync(ref["ti_endstep"], None)
    sums = np.zeros(18)
    assert L.ngravs_displacement_sums(eng._h, C.byref(tc), sums.ctypes.data) == 0
    assert np.array_equal(sums, eng.displacement_sums(ref["type"], ref["vel"], ref["mass"]))
    for k in c0:
        assert np.array_equal(rec[k], ref[k], equal_nan=True), k
    assert kicked.value == int(np.sum(c0["ti_endstep"] == TI)) and list(pm) == [TI, pm[1]] and pm[1] > TI
    assert np.all(rec["pad0"] == 0) and np.all(rec["pad1"] == 0)


# ---- the loop -------------------------------------------------------------------------------------------------------------
def snapshot(cols):
    return {k: (v.cpu().numpy() if hasattr(v, "cpu") else v.copy()) for k, v in cols.items() if k in TIME_KEYS}


TIME_KEYS = ("type", "pos", "vel", "mass", "ti_begstep", "ti_endstep", "grav_accel", "grav_pm") + GASF


def run_and_compare(pkg, eng, cols, P, sph, steps, mesh, soft, freq=0.0):
    """every station of the device loop is held against the restatement applied to the loop's OWN state in front of that station"""
    state, rungs, kicks = {}, set(), 0

    def on_station(name, tl):
        nonlocal kicks
        now = snapshot(tl.cols)
        if name == "moved":
            want = ref_move(state["drift"], P, tl.ti_previous, tl.ti_current, mesh, wrap_box=tl.eng.cfg.box_size if tl.wrapped else 0.0)
            assert_state(now, want, [], 0, "step %d drift" % tl.steps)
        if name == "advance":
            state["pm_ti"], state["dt_disp"] = tl.pm_ti and list(tl.pm_ti), tl.dt_displacement
            assert tl.disp_sums is not None
        if name == "end":
            want, pm_want, near, act, _ = ref_advance(state["advance"], P, tl.ti_current, state["dt_disp"], mesh, soft, state["pm_ti"])
            assert_state(now, want, near, len(act), "step %d advance" % tl.steps)
            assert tl.n_kicked == len(act) == tl.n_active and tl.pm_ti == pm_want
            kicks += mesh and state["pm_ti"][1] == tl.ti_current
            rungs.update(np.unique(now["ti_endstep"] - now["ti_begstep"]).tolist())
        state[name] = now
    tl = pkg.timeline.Timeline(eng, cols, c_params(pkg, P), sph=sph, on_station=on_station, tree_domain_update_frequency=freq)
    for _ in range(steps):
        tl.step()
        assert tl.ti_current < TB
    return tl, rungs, kicks


@pytest.mark.gpu
@pytest.mark.parametrize("freq", [0.0, 0.1])
def test_loop_collisionless(pkg, freq):
    import torch
    n = 1500
    pos, mass, _ = pkg.ic.plummer_sphere(n, seed=11)
    rng = np.random.default_rng(12)
    ptype = np.where(np.arange(n) % 3 == 0, 2, 1).astype(np.int32)
    r = np.linalg.norm(pos, axis=1)
    vel = rng.normal(size=(n, 3)) * (0.4 * (1 + r * r) ** -0.25)[:, None]
    soft = np.array([0, 0.02, 0.01, 0, 0, 0.0])
    cfg = pkg.make_config(n_gravs=1, G=1.0, softening=list(soft), theta=0.0, err_tol_force_acc=0.005)
    eng = pkg.Engine(cfg)
    P = params(False, time_max=8.0, timebase_interval=8.0 / TB, max_size_timestep=0.25, min_size_timestep=0.0, err_tol_int_accuracy=0.025)
    host = dict(type=ptype, pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    cols = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    tl, rungs, _ = run_and_compare(pkg, eng, cols, P, None, 12, False, soft, freq)
    assert len(rungs) >= 3, rungs
    assert tl.ti_current > 0
    if freq == 0.0:
        # gravity is undisturbed: the final state in the loop's engine and in a fresh one
        fin = {k: v.cpu().numpy() for k, v in cols.items()}
        acc = []
        for e in (eng, pkg.Engine(cfg)):
            e.set_particles(fin["pos"], fin["mass"], fin["type"], old_acc=fin["old_acc"])
            e.compute_accelerations(False)
            acc.append(e.get_accel()[0])
        assert np.array_equal(acc[0], acc[1])


@pytest.mark.gpu
def test_loop_gas_comoving_treepm(pkg):
    import torch
    ngas = ndm = 1000
    n = ngas + ndm
    box, G, hub = 50000.0, 43007.1, 0.1
    P = params(True, hubble=hub, min_size_timestep=0.0, max_size_timestep=0.01, max_rms_displacement_fac=0.25, err_tol_int_accuracy=1e-4)
    rng = np.random.default_rng(21)
    rho_crit = 3 * hub * hub / (8 * math.pi * G)
    ptype = np.concatenate([np.zeros(ngas), np.ones(ndm)]).astype(np.int32)
    mass = np.where(ptype == 0, P["omega_baryon"], P["omega0"] - P["omega_baryon"]) * rho_crit * box ** 3 / 1000
    soft = np.array([100.0, 150.0, 0, 0, 0, 0])
    cfg = pkg.make_config(n_gravs=1, periodic=1, pmgrid=16, box_size=box, G=G, softening=list(soft), theta=0.5)
    eng = pkg.Engine(cfg)
    host = dict(type=ptype, pos=rng.uniform(0, box, (n, 3)), vel=rng.normal(0, 20.0, (n, 3)), mass=mass,
                ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32), grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)),
                old_acc=np.zeros(n))
    eng.set_particles(host["pos"], mass, ptype)
    eng.domain_Decomposition()
    eng.force_treebuild()
    gasf = lambda v: np.where(ptype == 0, v, np.nan)   # noqa: E731
    host.update(vel_pred=host["vel"] * gasf(1.0)[:, None], hydro_accel=np.zeros((n, 3)) * gasf(1.0)[:, None],
                entropy=gasf(10.0 ** rng.uniform(1.5, 2.5, n)), dt_entropy=gasf(0.0), density=gasf(1.0), hsml=eng.sph_hsml_guess(33.0),
                pressure=gasf(1.0), div_vel=gasf(0.0), curl_vel=gasf(0.0), dhsml_factor=gasf(1.0), max_signal_vel=gasf(1.0))
    cols = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in host.items()}
    sph = dict(des_num_ngb=33.0, max_num_ngb_deviation=2.0, art_bulk_visc_const=0.8)
    tl, rungs, kicks = run_and_compare(pkg, eng, cols, P, sph, 8, True, soft)
    print("rungs", sorted(rungs), "long-range kicks", kicks)
    assert kicks >= 1 and tl.ti_current > 0 and tl.pm_ti[1] > 0
    fin = snapshot(cols)
    gas = ptype == 0
    assert np.isfinite(fin["pressure"][gas]).all() and np.all(fin["density"][gas] > 0) and np.all(fin["entropy"][gas] > 0)
    assert all(np.isnan(fin[k][~gas]).all() for k in GASF)


@pytest.mark.gpu
def test_momentum_is_kept(pkg):
    """64 equal masses, every node opened, one rung: pair forces are antisymmetric, only the row sums round"""
    n = 64
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(n, 3))
    vel = rng.normal(size=(n, 3)) * 0.3
    vel -= vel.mean(axis=0)
    mass = np.full(n, 1.0 / n)
    soft = np.array([0, 0.05, 0, 0, 0, 0.0])
    cfg = pkg.make_config(n_gravs=1, G=1.0, softening=list(soft), theta=0.0, err_tol_force_acc=0.0)
    eng = pkg.Engine(cfg)
    step = 1 << 18
    P = params(False, time_max=64.0, timebase_interval=64.0 / TB, max_size_timestep=step * 64.0 / TB, min_size_timestep=0.0,
               err_tol_int_accuracy=1e6)
    cols = dict(type=np.ones(n, np.int32), pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    p0 = np.abs((mass[:, None] * vel).sum(axis=0)).max()
    tl = pkg.timeline.Timeline(eng, cols, c_params(pkg, P))
    for k in range(16):
        tl.step()
        cols["old_acc"][:] = 0                                    # OldAcc = 0: the relative criterion opens every node
        assert np.all(cols["ti_endstep"] - cols["ti_begstep"] == step) and tl.full_step
    assert tl.ti_current == 15 * step
    mom = np.linalg.norm((mass[:, None] * cols["vel"]).sum(axis=0))
    scale = np.sum(mass * np.linalg.norm(cols["vel"], axis=1))
    print("|sum m v| = %.3g, sum m |v| = %.3g, at the start %.3g" % (mom, scale, p0))
    assert mom < 1e-12 * scale
