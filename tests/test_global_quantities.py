"""Energy statistics on the device: ngravs_global_sums, ngravs_global_finish, ngravs_energy_line and the "statistics" station of
timeline.Timeline -- compute_global_quantities_of_system() (global.c:22-198) and the energy.txt line of energy_statistics()
(run.c:413-433).

The truth is ref_global() below, a numpy restatement of global.c:32-114 written from that file (line references beside each
rule); it returns the 6 x 13 sums and, per entry, A = the sum of the magnitudes of its terms.  tests/golden/global_reference.npz
(tests/golden/make_global_golden.py) pins the restatement to the reference's own global.c, compiled in place: inputs and the
119 recorded doubles of SysState for PMGRID with a potential column, no mesh, ISOTHERM_EQS, and PMGRID again with a PM step
whose middle is not the current time.  The comoving branch differs from those only in a1..a3 and the factor calls, which
test_time_integration.py pins.

Tolerance.  Every one of the 78 sums: |got - want| <= 1e-13 A (FTOL of test_time_integration.py).  A blocked fp64 sum of up to
2.7e5 rows is bounded by about 20 roundings of A (2e-15), a term adds a few ulp for pow and fused multiply-adds: a margin of about
30.  An entry with A == 0 must be exactly 0.  The fields of SysState derived from the sums are compared at 1e-13 x the scale that A
gives them (state_scale).  ngravs_global_finish is compared with finish() bit for bit: the same operations in the same order.
"""
import ctypes as C
import functools
import io
import math
import os
import re

import numpy as np
import pytest

import test_time_integration as T

FTOL, TI, TB = T.FTOL, T.TI, T.TB
NEW = ["ngravs_global_sums", "ngravs_global_finish", "ngravs_energy_line"]
PM_TI = [TI - (1 << 20), TI + (1 << 20)]         # (its middle is TI: the long-range prediction is over no time)
PM_TI_KICK = [TI - (1 << 20), TI + (1 << 18)]    # a PM step whose middle lies before TI: GravPM enters the predicted velocity
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "global_reference.npz")
# struct state_of_system (allvars.h), in its order
FIELDS = [(k, ()) for k in ("Mass", "EnergyKin", "EnergyPot", "EnergyInt", "EnergyTot")] + [
    (k, (4,)) for k in ("Momentum", "AngMomentum", "CenterOfMass")] + [
    (k, (6,)) for k in ("MassComp", "EnergyKinComp", "EnergyPotComp", "EnergyIntComp", "EnergyTotComp")] + [
    (k, (6, 4)) for k in ("MomentumComp", "AngMomentumComp", "CenterOfMassComp")]
GAS_READ = ("hydro_accel", "entropy", "dt_entropy", "density")
READ = ("type", "pos", "vel", "mass", "ti_begstep", "ti_endstep", "grav_accel", "grav_pm") + GAS_READ


# ---- the restatement ----------------------------------------------------------------------------------------------------
def ref_global(c, P, ti, pm_ti=None, potential=None):
    """global.c:32-114 for one task: (sums [6, 13], A [6, 13]); pm_ti: [PM_Ti_begstep, PM_Ti_endstep] of a build with PMGRID,
    else None; potential: P[].Potential or None (0)"""
    tbi, comoving = P["timebase_interval"], P["comoving"]
    ty, m, pos = c["type"], c["mass"], c["pos"]
    n, gas = len(ty), c["type"] == 0
    if comoving:                                                                 # :32-41
        a1 = P["time_begin"] * math.exp(ti * tbi)
        a2, a3 = a1 * a1, a1 * a1 * a1
    else:
        a1 = a2 = a3 = 1.0
    beg = c["ti_begstep"].astype(np.int64)
    mid = (beg + c["ti_endstep"]) // 2
    dt_entr = (ti - mid) * tbi                                                   # :60, :67-68
    if comoving:                                                                 # :61-64
        gk, hk = P["tables"][1], P["tables"][2]
        dt_gravkick = T.ref_factor(gk, P, beg, ti) - T.ref_factor(gk, P, beg, mid)
        dt_hydrokick = T.ref_factor(hk, P, beg, ti) - T.ref_factor(hk, P, beg, mid)
    else:
        dt_gravkick = dt_hydrokick = dt_entr
    vel = c["vel"] + c["grav_accel"] * dt_gravkick[:, None]                      # :72
    if gas.any():
        vel[gas] = vel[gas] + c["hydro_accel"][gas] * dt_hydrokick[gas, None]    # :73-74
    if pm_ti is not None:                                                        # :79-88
        pmb, pmid = pm_ti[0], (pm_ti[0] + pm_ti[1]) // 2
        dt_pm = float(T.ref_factor(gk, P, pmb, ti) - T.ref_factor(gk, P, pmb, pmid)) if comoving else (ti - pmid) * tbi
        vel = vel + c["grav_pm"] * dt_pm
    t = np.zeros((n, 13))
    t[:, 0] = m                                                                  # :54
    t[:, 1] = 0.5 * m * (vel[:, 0] * vel[:, 0] + vel[:, 1] * vel[:, 1] + vel[:, 2] * vel[:, 2]) / a2   # :90-91
    if gas.any():
        entr = c["entropy"][gas] + c["dt_entropy"][gas] * dt_entr[gas]           # :77
        gm1 = P["gamma"] - 1
        egyspec = entr if P["gamma"] == 1 else entr / gm1 * np.power(c["density"][gas] / a3, gm1)      # :95-99
        t[gas, 2] = m[gas] * egyspec                                             # :100
    if potential is not None:
        t[:, 3] = 0.5 * m * potential / a1                                       # :56
    t[:, 4:7] = m[:, None] * vel                                                 # :107
    t[:, 7] = m * (pos[:, 1] * vel[:, 2] - pos[:, 2] * vel[:, 1])                # :111-113
    t[:, 8] = m * (pos[:, 2] * vel[:, 0] - pos[:, 0] * vel[:, 2])
    t[:, 9] = m * (pos[:, 0] * vel[:, 1] - pos[:, 1] * vel[:, 0])
    t[:, 10:13] = m[:, None] * pos                                               # :108
    sums, A = np.zeros((6, 13)), np.zeros((6, 13))
    for k in range(6):   # (added up in extended precision: a plain fp64 sum of 2.6e5 terms would be the larger error of the comparison)
        tk = t[ty == k].astype(np.longdouble)
        sums[k], A[k] = tk.sum(axis=0), np.abs(tk).sum(axis=0)
    assert np.isfinite(sums).all()
    return sums, A


def finish(sums):
    """global.c:130-194 on the (all-reduced) sums, operation for operation in Python floats: the 119 doubles of SysState"""
    sums = np.asarray(sums, dtype=np.float64).reshape(6, 13)
    s = {k: np.zeros(shape) for k, shape in FIELDS}
    for i in range(6):
        s["MassComp"][i], s["EnergyKinComp"][i], s["EnergyIntComp"][i], s["EnergyPotComp"][i] = (float(x) for x in sums[i, :4])
        s["MomentumComp"][i, :3], s["AngMomentumComp"][i, :3], s["CenterOfMassComp"][i, :3] = sums[i, 4:7], sums[i, 7:10], sums[i, 10:13]
        s["EnergyTotComp"][i] = float(sums[i, 1]) + float(sums[i, 3]) + float(sums[i, 2])                  # :133-134
    tot = {k: 0.0 for k in ("Mass", "EnergyKin", "EnergyPot", "EnergyInt", "EnergyTot")}
    vec = {k: [0.0, 0.0, 0.0, 0.0] for k in ("Momentum", "AngMomentum", "CenterOfMass")}
    for i in range(6):                                                                                     # :141-155
        for k in tot:
            tot[k] += float(s[k + "Comp"][i])
        for j in range(3):
            for k in vec:
                vec[k][j] += float(s[k + "Comp"][i, j])
    for i in range(6):                                                                                     # :157-160
        for j in range(3):
            if s["MassComp"][i] > 0:
                s["CenterOfMassComp"][i, j] = float(s["CenterOfMassComp"][i, j]) / float(s["MassComp"][i])
    for j in range(3):                                                                                     # :162-164
        if tot["Mass"] > 0:
            vec["CenterOfMass"][j] /= tot["Mass"]
    for k in vec:                                                                                          # :166-193
        for i in range(6):
            x = 0.0
            for j in range(3):
                x += float(s[k + "Comp"][i, j]) * float(s[k + "Comp"][i, j])
            s[k + "Comp"][i, 3] = math.sqrt(x)
        x = 0.0
        for j in range(3):
            x += vec[k][j] * vec[k][j]
        vec[k][3] = math.sqrt(x)
        s[k][:] = vec[k]
    for k in tot:
        s[k] = np.float64(tot[k])
    return np.concatenate([np.ravel(s[k]) for k, _ in FIELDS])


def state_scale(sums, A):
    """what an error of A in every sum is worth in each of the 119 fields: A itself for the sums and their totals, A / mass for the
    centres of mass, and for a norm the norm of its components' scales"""
    mass = sums[:, 0]
    s = {k: np.zeros(shape) for k, shape in FIELDS}
    s["MassComp"], s["EnergyKinComp"], s["EnergyIntComp"], s["EnergyPotComp"] = A[:, 0], A[:, 1], A[:, 2], A[:, 3]
    s["EnergyTotComp"] = A[:, 1] + A[:, 2] + A[:, 3]
    s["MomentumComp"][:, :3], s["AngMomentumComp"][:, :3] = A[:, 4:7], A[:, 7:10]
    s["CenterOfMassComp"][:, :3] = A[:, 10:13] / np.where(mass > 0, mass, 1.0)[:, None]
    for k in ("Mass", "EnergyKin", "EnergyPot", "EnergyInt", "EnergyTot"):
        s[k] = s[k + "Comp"].sum()
    for k in ("Momentum", "AngMomentum"):
        s[k][:3] = s[k + "Comp"][:, :3].sum(axis=0)
    s["CenterOfMass"][:3] = A[:, 10:13].sum(axis=0) / (mass.sum() if mass.sum() > 0 else 1.0)
    for k in ("Momentum", "AngMomentum", "CenterOfMass"):
        s[k][3] = np.linalg.norm(s[k][:3])
        s[k + "Comp"][:, 3] = np.linalg.norm(s[k + "Comp"][:, :3], axis=1)
    return np.concatenate([np.ravel(s[k]) for k, _ in FIELDS])


def flat(state):
    """an abi.SysState as its 119 doubles"""
    return np.frombuffer(bytes(state), dtype=np.float64).copy()


def assert_sums(got, want, A, what):
    got = np.asarray(got).reshape(6, 13)
    err = np.abs(got - want)
    worst = float(np.max(err[A > 0] / A[A > 0])) if (A > 0).any() else 0.0
    print("%-50s max |got - want| / sum |term| = %.3g" % (what, worst))
    assert np.all(got[A == 0] == 0), what
    assert np.all(err <= FTOL * A), (what, worst)
    return worst


def assert_state(got, sums, A, what):
    want, scale = finish(sums), state_scale(sums, A)
    err = np.abs(got - want)
    worst = float(np.max(err[scale > 0] / scale[scale > 0])) if (scale > 0).any() else 0.0
    print("%-50s max deviation / scale = %.3g" % (what, worst))
    assert np.all(got[scale == 0] == 0), what
    assert np.all(err <= FTOL * scale), (what, worst)


def potential_of(n, seed):
    return -10.0 ** np.random.default_rng(seed).uniform(0, 2, n)


@functools.lru_cache(maxsize=None)
def case(n, comoving, mesh, with_pot, gamma=T.GAMMA):
    """(parameters, columns, potential, the restatement's sums, A) of one seeded set; computed once, never changed"""
    P = T.params(comoving, gamma=gamma)
    c = T.make_set(n, 1000 + n, P, mesh)
    pot = potential_of(n, 2000 + n) if with_pot else None
    sums, A = ref_global(c, P, TI, PM_TI_KICK if mesh else None, pot)
    for v in c.values():
        v.setflags(write=False)
    return P, c, pot, sums, A


def read_cols(c, mesh=True):
    return {k: v for k, v in c.items() if k in READ and (mesh or k != "grav_pm")}


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_exported_declared_and_laid_out_as_the_header_says(pkg, have_lib):
    root = pkg.__file__.replace("gadget-2.0.7-ngravs_amd/__init__.py", "")
    hdr = open(root + "include/ngravs_hip.h").read()
    for name in NEW:
        assert name in pkg.EXPORTS and hasattr(have_lib, name), name
        assert "int %s(" % name in hdr
    body = hdr[:hdr.index("} ngravs_sysstate_t;")]
    body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
    decl = [re.match(r"\s*(?:double\s+)?(\w+)((?:\[\d+\])*)\s*$", piece).groups() for d in body.split(";") if d.strip() for piece in d.split(",")]
    want = [(k, "".join("[%d]" % x for x in shape)) for k, shape in FIELDS]
    assert decl == want, decl
    def dims(t):
        return "[%d]" % t._length_ + dims(t._type_) if hasattr(t, "_length_") else ""
    got = [(k, dims(t)) for k, t in pkg.abi.SysState._fields_]
    assert got == want, got
    assert C.sizeof(pkg.abi.SysState) == 952 == 8 * len(finish(np.zeros(78)))
    assert "#define NGRAVS_GLOBAL_NSUMS 78" in hdr and pkg.abi.GLOBAL_NSUMS == 78
    capi = open(root + "gadget-2.0.7-ngravs_amd/csrc/capi.hip").read()
    assert "static_assert(sizeof(ngravs_sysstate_t) == 952" in capi
    assert have_lib.ngravs_abi_version() == 3
    assert C.sizeof(pkg.abi.TimeCols) == 288 and C.sizeof(pkg.abi.TimeParams) == 168
    L = have_lib
    assert L.ngravs_global_sums(None, None, None, 0, None, None, 0, None) == -1
    assert L.ngravs_global_finish(None, None) == -1
    assert L.ngravs_energy_line(None, 0.0, None, 0) == -1
    for m in ("global_sums", "global_quantities"):
        assert hasattr(pkg.Engine, m), m
    assert callable(pkg.global_finish) and callable(pkg.energy_line)


def test_restatement_against_the_reference(pkg):
    """ref_global + finish against the 119 doubles the reference's own global.c gave for the recorded sets"""
    z = np.load(GOLDEN)
    variants = [str(v) for v in z["variants"]]
    assert variants == ["pmgrid", "nomesh", "isotherm", "pmgrid_kick"]
    for v in variants:
        c = {k: z["%s_%s" % (z["%s_set" % v], k)] for k in READ}
        P = T.params(False, gamma=float(z[v + "_gamma"]), timebase_interval=float(z[v + "_tbi"]))
        pm_ti = [int(x) for x in z[v + "_pm_ti"]] if v.startswith("pmgrid") else None
        pot = z["%s_%s" % (z["%s_set" % v], "potential")]
        sums, A = ref_global(c, P, int(z[v + "_ti"]), pm_ti, pot)
        ref = z[v + "_state"]
        assert ref.shape == (119,) and np.isfinite(ref).all()
        assert_state(ref, sums, A, "reference, " + v)
        assert np.all(ref[[1, 2, 3]] != 0)                                       # kinetic, potential and internal energy are there
    # the variants do differ where their switches act
    assert z["pmgrid_kick_state"][1] != z["nomesh_state"][1] and z["pmgrid_state"][2] == z["nomesh_state"][2]
    assert [int(x) for x in z["pmgrid_pm_ti"]] == PM_TI and [int(x) for x in z["pmgrid_kick_pm_ti"]] == PM_TI_KICK


def test_finish_is_the_rule_of_the_reference(pkg, have_lib):
    P, c, pot, sums, A = case(1037, False, True, True)
    got = flat(pkg.global_finish(sums.ravel()))
    want = finish(sums)
    assert np.array_equal(got, want), np.flatnonzero(got != want)
    assert got[0] == sums[:, 0].sum() and got[4] != 0
    # a type without mass keeps its undivided centre of mass
    s = sums.copy()
    s[3] = 0
    s[3, 10:13] = [1.0, 2.0, 3.0]
    st = pkg.global_finish(s.ravel())
    assert list(st.CenterOfMassComp[3])[:3] == [1.0, 2.0, 3.0] and st.MassComp[3] == 0
    assert np.array_equal(flat(st), finish(s))
    zero = flat(pkg.global_finish(np.zeros(78)))
    assert np.all(zero == 0)
    # three parts, one of them empty: the sums add up
    n = len(c["type"])
    parts = [np.arange(0, 400), np.arange(400, 400), np.arange(400, n)]
    add, A_add = np.zeros((6, 13)), np.zeros((6, 13))
    for rows in parts:
        ps, pa = ref_global({k: v[rows] for k, v in c.items()}, P, TI, PM_TI_KICK, pot[rows])
        add, A_add = add + ps, A_add + pa
    assert np.all(ref_global({k: v[parts[1]] for k, v in c.items()}, P, TI, PM_TI_KICK, pot[parts[1]])[0] == 0)
    assert_state(flat(pkg.global_finish(add.ravel())), sums, A, "three parts")


def test_energy_line(pkg, have_lib):
    P, c, pot, sums, A = case(1037, False, True, True)
    st = pkg.global_finish(sums.ravel())
    time = 0.3125
    fields = [time, st.EnergyInt, st.EnergyPot, st.EnergyKin]
    for i in range(6):
        fields += [st.EnergyIntComp[i], st.EnergyPotComp[i], st.EnergyKinComp[i]]
    fields += list(st.MassComp)
    want = " ".join("%g" % v for v in fields) + "\n"
    assert len(fields) == 28 and pkg.energy_line(st, time) == want
    buf = C.create_string_buffer(len(want) + 1)
    assert have_lib.ngravs_energy_line(C.byref(st), time, buf, len(want)) == -1 and buf.raw == bytes(len(want) + 1)
    assert have_lib.ngravs_energy_line(C.byref(st), time, buf, len(want) + 1) == len(want) and buf.value.decode() == want
    assert have_lib.ngravs_energy_line(C.byref(st), time, None, 1000) == -1


# ---- GPU ------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("comoving,mesh", T.MODES)
def test_sums_on_the_sets(pkg, comoving, mesh):
    eng = T.engine(pkg, mesh)
    worst = 0.0
    for n in T.SIZES:
        for with_pot in (False, True):
            P, c, pot, sums, A = case(n, comoving, mesh, with_pot)
            got = eng.global_sums(read_cols(c, mesh), T.c_params(pkg, P), TI, PM_TI_KICK if mesh else None, pot)
            worst = max(worst, assert_sums(got, sums, A, "n=%d comoving=%d mesh=%d pot=%d" % (n, comoving, mesh, with_pot)))
            if n >= 6:
                assert np.all(got.reshape(6, 13)[:, 0] > 0) and np.all((got.reshape(6, 13)[:, 3] < 0) == with_pot)
            st = eng.global_quantities(read_cols(c, mesh), T.c_params(pkg, P), TI, PM_TI_KICK if mesh else None, pot)
            assert np.array_equal(flat(st), flat(pkg.global_finish(got)))
    print("worst of the mode %.3g" % worst)


@pytest.mark.gpu
def test_sums_where_the_grid_stride_loop_takes_a_second_trip(pkg):
    n = 1024 * 256 + 257
    P, c, pot, sums, A = case(n, True, True, True)
    eng = T.engine(pkg, True)
    got = eng.global_sums(read_cols(c), T.c_params(pkg, P), TI, PM_TI_KICK, pot)
    assert_sums(got, sums, A, "n=%d comoving, mesh, potential" % n)
    assert np.array_equal(got, eng.global_sums(read_cols(c), T.c_params(pkg, P), TI, PM_TI_KICK, pot))


@pytest.mark.gpu
def test_isothermal_no_gas_and_the_start_state(pkg):
    eng = T.engine(pkg, False)
    # gamma = 1 (ISOTHERM_EQS): m entr, no division by gamma - 1
    P, c, pot, sums, A = case(1037, False, False, False, gamma=1.0)
    got = eng.global_sums(read_cols(c, False), T.c_params(pkg, P), TI)
    assert_sums(got, sums, A, "gamma = 1")
    assert np.isfinite(got).all() and got[2] > 0
    # no type-0 row, the gas columns absent
    P, c, pot, sums, A = case(1037, True, False, True)
    rows = c["type"] != 0
    nogas = {k: v[rows].copy() for k, v in c.items() if k in READ and k not in GAS_READ and k != "grav_pm"}
    want, A1 = ref_global(nogas, P, TI, None, pot[rows])
    got = eng.global_sums(nogas, T.c_params(pkg, P), TI, potential=pot[rows].copy())
    assert_sums(got, want, A1, "no gas")
    assert np.all(got[:13] == 0)
    # the start: ti_begstep = ti_endstep = ti_current = 0, the prediction is over no time at all
    for comoving in (False, True):
        P, c, pot, _, _ = case(1037, comoving, False, False)
        start = {k: v.copy() for k, v in read_cols(c, False).items()}
        start["ti_begstep"][:] = 0
        start["ti_endstep"][:] = 0
        want, A1 = ref_global(start, P, 0)
        got = eng.global_sums(start, T.c_params(pkg, P), 0)
        assert_sums(got, want, A1, "start state, comoving=%d" % comoving)
        mv = (start["mass"][:, None] * start["vel"])[start["type"] == 1].sum(axis=0)
        assert np.all(np.abs(got[13 + 4:13 + 7] - mv) <= FTOL * A1[1, 4:7])    # momentum is m Vel itself


def time_cols_of(pkg, rec, names, n, on_device=0):
    tc = pkg.abi.TimeCols()
    for k in names:
        setattr(tc, k, rec.ctypes.data + rec.dtype.fields[k][1])
        setattr(tc, k + "_stride", rec.dtype.itemsize)
    tc.n, tc.on_device = n, on_device
    return tc


@pytest.mark.gpu
def test_the_same_bits(pkg):
    import torch
    P, c, pot, sums, A = case(1037, True, True, True)
    eng = T.engine(pkg, True)
    par = T.c_params(pkg, P)
    host = eng.global_sums(read_cols(c), par, TI, PM_TI_KICK, pot)
    assert np.array_equal(host, eng.global_sums(read_cols(c), par, TI, PM_TI_KICK, pot))             # twice
    d = {k: torch.from_numpy(v.copy()).cuda() for k, v in read_cols(c).items()}
    dev = eng.global_sums(d, par, TI, PM_TI_KICK, torch.from_numpy(pot.copy()).cuda())
    assert np.array_equal(host, dev)                                                            # device tensors
    assert all(np.array_equal(d[k].cpu().numpy(), c[k], equal_nan=True) for k in d)             # ... which are only read
    # P[]-like records through the raw C ABI: odd strides, the potential inside the record
    n = 1037
    fields = [(k, np.int32 if k in T.INTS else np.float64, (3,) if k in T.VEC else ()) for k in READ]
    rec = np.zeros(n, dtype=np.dtype([("pad0", np.float64)] + fields + [("potential", np.float64), ("pad1", np.int32, (3,))], align=True))
    for k in READ:
        rec[k] = c[k]
    rec["potential"] = pot
    assert rec.dtype.itemsize not in (8, 24) and rec.dtype.itemsize % 16 != 0
    tc = time_cols_of(pkg, rec, READ, n)
    pm = (C.c_int32 * 2)(*PM_TI_KICK)
    out = np.full(78, 7.0)
    L = pkg.lib()
    assert L.ngravs_global_sums(eng._h, C.byref(tc), C.byref(par), TI, pm, rec.ctypes.data + rec.dtype.fields["potential"][1],
                                rec.dtype.itemsize, out.ctypes.data) == 0
    assert np.array_equal(out, host) and list(pm) == PM_TI_KICK
    # no rows
    none = {k: v[:0].copy() for k, v in read_cols(c).items()}
    assert np.array_equal(eng.global_sums(none, par, TI, PM_TI_KICK), np.zeros(78))
    tc.n = 0
    out[:] = 7.0
    assert L.ngravs_global_sums(eng._h, C.byref(tc), C.byref(par), TI, pm, None, 0, out.ctypes.data) == 0 and np.all(out == 0)


@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    P, c, pot, sums, A = case(257, False, True, True)
    eng = T.engine(pkg, True)
    par = T.c_params(pkg, P)
    L = pkg.lib()
    pm = (C.c_int32 * 2)(*PM_TI_KICK)

    def refused(cols, par=par, pm=pm, what=""):
        tc, keep = eng._time_cols(cols)
        out = np.full(78, 7.0)
        assert L.ngravs_global_sums(eng._h, C.byref(tc), C.byref(par), TI, pm, None, 0, out.ctypes.data) == -1, what
        assert np.all(out == 7.0), what
    cols = {k: v.copy() for k, v in read_cols(c).items()}
    refused(dict(cols, type=np.where(np.arange(257) == 5, 6, cols["type"]).astype(np.int32)), what="a type outside 0..5")
    refused(dict(cols, type=np.where(np.arange(257) == 5, -1, cols["type"]).astype(np.int32)), what="a negative type")
    refused({k: v for k, v in cols.items() if k != "density"}, what="a gas column missing with gas")
    refused({k: v for k, v in cols.items() if k != "grav_accel"}, what="a required column")
    refused({k: v for k, v in cols.items() if k != "grav_pm"}, what="GravPM with a mesh")
    refused(cols, pm=None, what="a mesh without pm_ti")
    refused(cols, par=T.c_params(pkg, dict(P, comoving=1)), what="comoving without tables")
    refused(cols, par=T.c_params(pkg, dict(P, gamma=0.9)), what="gamma < 1")
    with pytest.raises(pkg.NgravsError) as e:
        eng.global_sums(cols, par, TI, None)
    assert "status -1" in str(e.value) and "pm_ti" in str(e.value)
    out = np.full(78, 7.0)
    tc, keep = eng._time_cols(cols)
    assert L.ngravs_global_sums(eng._h, C.byref(tc), C.byref(par), TI, pm, None, 0, out.ctypes.data) == 0 and np.all(out != 7.0)
    assert all(np.array_equal(cols[k], c[k], equal_nan=True) for k in cols)


# ---- the loop -------------------------------------------------------------------------------------------------------------
def momentum_run(pkg, steps, **kw):
    """the 64 bodies of test_time_integration.test_momentum_is_kept: equal masses, every node opened, one rung"""
    n = 64
    rng = np.random.default_rng(3)
    pos = rng.normal(size=(n, 3))
    vel = rng.normal(size=(n, 3)) * 0.3
    vel -= vel.mean(axis=0)
    mass = np.full(n, 1.0 / n)
    soft = np.array([0, 0.05, 0, 0, 0, 0.0])
    eng = pkg.Engine(pkg.make_config(n_gravs=1, G=1.0, softening=list(soft), theta=0.0, err_tol_force_acc=0.0))
    step = 1 << 18
    P = T.params(False, time_max=64.0, timebase_interval=64.0 / TB, max_size_timestep=step * 64.0 / TB, min_size_timestep=0.0,
                 err_tol_int_accuracy=1e6)
    cols = dict(type=np.ones(n, np.int32), pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    tl = pkg.timeline.Timeline(eng, cols, T.c_params(pkg, P), **kw)
    times = []
    for _ in range(steps):
        tl.step()
        cols["old_acc"][:] = 0
        times.append(tl.time)
    return tl, cols, P, times


@pytest.mark.gpu
def test_timeline_statistics_on_every_step(pkg):
    states = []

    def hook(name, tl):
        if name == "statistics":
            states.append([T.snapshot(tl.cols), tl.ti_current, None])
        if name == "advance" and states and states[-1][2] is None:
            states[-1][2] = flat(tl.sys_state)
    out = io.StringIO()
    tl, cols, P, times = momentum_run(pkg, 16, time_bet_statistics=0, energy_file=out, on_station=hook)
    assert len(tl.energy_lines) == 16 == len(states) and out.getvalue() == "".join(tl.energy_lines)
    assert [float(line.split()[0]) for line in tl.energy_lines] == [float("%g" % t) for t in times]
    assert all(len(line.split()) == 28 and line.endswith("\n") for line in tl.energy_lines)
    assert tl.energy_lines[-1] == pkg.energy_line(tl.sys_state, tl.time)
    # every station against the restatement on the columns as the hook saw them
    for k, (snap, ti, got) in enumerate(states):
        sums, A = ref_global(snap, P, ti)
        assert_state(got, sums, A, "step %d" % (k + 1))
        scale = np.sum(snap["mass"] * np.linalg.norm(snap["vel"], axis=1))
        assert got[8] < 1e-12 * scale, (k, got[8], scale)                        # Momentum[3], the bound of test_momentum_is_kept
    print("|Momentum| = %.3g, sum m |v| = %.3g" % (got[8], scale))


@pytest.mark.gpu
def test_timeline_without_statistics_is_the_loop_as_it_was(pkg):
    a, cols_a, _, _ = momentum_run(pkg, 4)
    b, cols_b, _, _ = momentum_run(pkg, 4, time_bet_statistics=None)
    assert a.energy_lines == [] == b.energy_lines and b.sys_state is None
    assert all(np.array_equal(cols_a[k], cols_b[k]) for k in cols_a)
    c, cols_c, _, _ = momentum_run(pkg, 4, time_bet_statistics=0)
    assert all(np.array_equal(cols_a[k], cols_c[k]) for k in cols_a) and len(c.energy_lines) == 4   # the station only reads


@pytest.mark.gpu
def test_timeline_spacing_of_several_steps(pkg):
    bet = 0.2                                                                    # a step is 1/16
    tl, cols, P, times = momentum_run(pkg, 12, time_bet_statistics=bet)
    last, want = P["time_begin"] - bet, []                                       # init.c:94
    for t in times:                                                              # run.c:52-58
        if t - last >= bet:
            want.append("%g" % t)
            last += bet
    assert 2 <= len(want) < 12
    assert [line.split()[0] for line in tl.energy_lines] == want
    assert tl.time_last_statistics == last


@pytest.mark.gpu
def test_timeline_gas_comoving_treepm(pkg):
    """the configuration of test_time_integration.test_loop_gas_comoving_treepm: the internal energy of the gas at each station"""
    import torch
    ngas = ndm = 1000
    n = ngas + ndm
    box, G, hub = 50000.0, 43007.1, 0.1
    P = T.params(True, hubble=hub, min_size_timestep=0.0, max_size_timestep=0.01, max_rms_displacement_fac=0.25, err_tol_int_accuracy=1e-4)
    rng = np.random.default_rng(21)
    rho_crit = 3 * hub * hub / (8 * math.pi * G)
    ptype = np.concatenate([np.zeros(ngas), np.ones(ndm)]).astype(np.int32)
    mass = np.where(ptype == 0, P["omega_baryon"], P["omega0"] - P["omega_baryon"]) * rho_crit * box ** 3 / 1000
    soft = np.array([100.0, 150.0, 0, 0, 0, 0])
    eng = pkg.Engine(pkg.make_config(n_gravs=1, periodic=1, pmgrid=16, box_size=box, G=G, softening=list(soft), theta=0.5))
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
    states = []

    def hook(name, tl):
        if name == "statistics":
            states.append([T.snapshot(tl.cols), tl.ti_current, list(tl.pm_ti), None])
        if name == "advance" and states and states[-1][3] is None:
            states[-1][3] = flat(tl.sys_state)
    pot = torch.from_numpy(potential_of(n, 77)).cuda()
    tl = pkg.timeline.Timeline(eng, cols, T.c_params(pkg, P), sph=dict(des_num_ngb=33.0, max_num_ngb_deviation=2.0, art_bulk_visc_const=0.8),
                               on_station=hook, time_bet_statistics=0, potential=lambda tl: pot)
    for _ in range(4):
        tl.step()
    assert len(states) == 4 == len(tl.energy_lines)
    for k, (snap, ti, pm_ti, got) in enumerate(states):
        sums, A = ref_global(snap, P, ti, pm_ti, pot.cpu().numpy())
        assert_state(got, sums, A, "gas step %d" % (k + 1))
        eint = got[5 + 12 + 18]                                                  # EnergyIntComp[0]
        assert eint > 0 and abs(eint - sums[0, 2]) <= FTOL * A[0, 2]
    assert states[-1][1] > 0 and len({s[3][5 + 12 + 18] for s in states}) > 1    # the gas did evolve
