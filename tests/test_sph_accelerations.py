"""The gas side of compute_accelerations() in one call (ngravs_sph_accelerations / Engine.sph_accelerations, csrc/kernels_sph.hip).

The call is density() with its pressure line, force_update_hmax() and hydro_force() for one task.  Its two walks are the kernels
of ngravs_sph_density and ngravs_sph_hydro, so three kinds of check suffice:
  * bit for bit against the existing calls: the density columns against Engine.sph_density on the same inputs, the hydro columns
    against Engine.sph_hydro fed the new call's own returned columns (pressure included).  Derivable, not measured: the same kernels
    see the same inputs, and the per-particle derivation is one __device__ function for both preparations;
  * the pressure line, the only new arithmetic, against numpy at TOL = 1e-11 relative (the project's figure; device pow against
    libm's), with a DtEntropy that is not 0 and Ti_begstep + Ti_endstep odd for a third of the rows, so that the reference's
    integer / 2 matters;
  * the whole chain against the reference's own density() -> pressure line -> hydro_force() in one run (oracle/_ref/ where the
    executables are present, the recorded tests/golden/sph_reference_*.npz otherwise: they hold the chain with entropy), every
    column, every gas row, with the scales and the flagging rule of tests/test_sph_reference.py (0 rows flagged on these inputs).
Columns of rows that are no gas hold NaN: they must not be read.  Sets: 3 000 gas + 1 000 others unless a case says otherwise.
"""
import ctypes as C
import importlib.util
import os
import re
import sys
import types

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))


def _load(name, path):
    if name in sys.modules:
        return sys.modules[name]
    spec = importlib.util.spec_from_file_location(name, path)
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    return mod


REF = _load("test_sph_reference", os.path.join(HERE, "test_sph_reference.py"))
H, D, R = REF.H, REF.D, REF.R
TOL, DES, DEV, GAMMA, VISC = D.TOL, D.DES, D.DEV, H.GAMMA, H.VISC
COLS = H.COLS                                   # hsml, density, pressure, dhsml_factor, div_vel, curl_vel: in/out
DENS = ("hsml", "density", "dhsml_factor", "div_vel", "curl_vel")
OUTS = ("num_ngb", "hydro_accel", "dt_entropy_out", "max_signal_vel")
TI = 1 << 20                                    # All.Ti_Current
SENTINEL = -3.25


# ---- inputs -------------------------------------------------------------------------------------------------------------
def gas_set(pkg, kind, n=4000, ngas=3000, seed=31):
    """gas_mix of the density tests with the converging flow of the hydro tests, an entropy spread over a decade, a DtEntropy that
    moves it by up to 20 %, and steps of 0 .. 65 ticks that end at TI: a third of them odd (Ti_begstep + Ti_endstep is odd)"""
    pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, kind, n=n, ngas=ngas, seed=seed)
    vel = vel - (0.02 * (pos - 500.0) if kind == "uniform" else 2.0 * pos)
    rng = np.random.default_rng(seed + 200)
    s = types.SimpleNamespace(pos=pos, mass=mass, ptype=ptype, vel=vel, gas=gas, n=len(pos), box=1000.0 if kind == "uniform" else 0.0,
                              periodic=kind == "uniform", tbi=H.KIND_TBI[kind])
    s.hsml0 = H.full(s.n, gas, hsml0[gas])
    s.A = H.full(s.n, gas, 10.0 ** rng.uniform(-0.5, 0.5, len(gas)))
    s.dA = s.A * 0.2 * rng.uniform(-1.0, 1.0, s.n) / (64 * s.tbi)
    ts = (rng.choice([0, 1, 2, 4, 8], s.n) * 2 ** rng.integers(0, 4, s.n)).astype(np.int32)
    ts = np.where(rng.uniform(size=s.n) < 1.0 / 3, ts | 1, ts).astype(np.int32)
    ts = np.where(ptype == 0, ts, -12345).astype(np.int32)          # rows of other types are not read
    s.end = np.full(s.n, TI, dtype=np.int32)
    s.beg = (s.end - ts).astype(np.int32)
    return s


def start_columns(s):
    col = {k: np.full(s.n, np.nan) for k in COLS}
    col["hsml"][s.gas] = s.hsml0[s.gas]
    return col


def sentinels(n, xp=np):
    return {k: xp.full((n, 3) if k == "hydro_accel" else (n,), SENTINEL) for k in OUTS}


def gas_call(eng, s, col, out=None, gamma=GAMMA, **kw):
    args = dict(dt_entropy=s.dA, ti_begstep=s.beg, ti_endstep=s.end, ti_current=TI, timebase_interval=s.tbi, des_num_ngb=DES,
                max_num_ngb_deviation=DEV, art_bulk_visc_const=VISC, gamma=gamma, out=out)
    args.update(kw)
    return eng.sph_accelerations(s.vel, s.A, *(col[k] for k in COLS), **args)


def dt_entr_of(s):
    """density.c:305 with the reference's integer division (the sums are positive: truncation is floor)"""
    return (TI - (s.beg.astype(np.int64) + s.end) // 2) * s.tbi


def sequence(eng, s, hsml_before, col_after, gamma=GAMMA):
    """what a caller did before this call existed: Engine.sph_density, (the pressure line), Engine.sph_hydro"""
    dens = eng.sph_density(s.vel, hsml_before, DES, DEV)
    hyd = H.call(eng, s.vel, col_after, art_bulk_visc_const=VISC, timestep=(s.end - s.beg).astype(np.int32), timebase_interval=s.tbi, gamma=gamma)
    return dens, hyd


def assert_is_the_sequence(res, col, dens, hyd, rows, what=""):
    assert len(rows) > 0
    for k in DENS:
        assert np.array_equal(col[k][rows], dens[k][rows]), (what, k)
    assert np.array_equal(res["num_ngb"][rows], dens["num_ngb"][rows]), what
    assert np.array_equal(res["hydro_accel"][rows], hyd["hydro_accel"][rows]), what
    assert np.array_equal(res["dt_entropy_out"][rows], hyd["dt_entropy"][rows]), what
    assert np.array_equal(res["max_signal_vel"][rows], hyd["max_signal_vel"][rows]), what
    assert np.isfinite(res["hydro_accel"][rows]).all() and np.any(res["hydro_accel"][rows] != 0) and np.all(res["max_signal_vel"][rows] > 0)


_CACHE = {}


def full_run(pkg, kind, **kw):
    """one all-active run per set, shared (and left unchanged) by the tests that need every gas row's SphP columns"""
    key = (kind,) + tuple(sorted(kw.items()))
    if key not in _CACHE:
        s = gas_set(pkg, kind, **kw)
        eng = D.make_engine(pkg, s.periodic, s.pos, s.mass, s.ptype)
        col = start_columns(s)
        res = gas_call(eng, s, col)
        dens, hyd = sequence(eng, s, s.hsml0, col)
        eng.close()
        _CACHE[key] = (s, col, res, dens, hyd)
    s, col, res, dens, hyd = _CACHE[key]
    return s, {k: a.copy() for k, a in col.items()}, res, dens, hyd


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_exported_declared_and_laid_out_as_the_header_says(pkg, have_lib):
    assert "ngravs_sph_accelerations" in pkg.EXPORTS and hasattr(have_lib, "ngravs_sph_accelerations")
    root = pkg.__file__.replace("gadget-2.0.7-ngravs_amd/__init__.py", "")
    hdr = open(root + "include/ngravs_hip.h").read()
    assert "int ngravs_sph_accelerations(" in hdr
    for cname, cls in (("ngravs_gas_in_t", pkg.abi.GasIn), ("ngravs_gas_out_t", pkg.abi.GasOut)):
        body = hdr[:hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
        names = [re.search(r"(\w+)\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    # 11 pointer + stride pairs, 9 doubles, 4 ints; 4 pointers, 4 strides -- capi.hip holds a static_assert of the same figures
    assert C.sizeof(pkg.abi.GasIn) == 264 and C.sizeof(pkg.abi.GasOut) == 64
    capi = open(root + "gadget-2.0.7-ngravs_amd/csrc/capi.hip").read()
    assert "static_assert(sizeof(ngravs_gas_in_t) == 264 && sizeof(ngravs_gas_out_t) == 64" in capi
    assert pkg.abi.GAS_INOUT_NAMES == COLS and pkg.abi.GAS_OUT_NAMES == OUTS
    # the one refusal that needs no context, hence no GPU
    assert have_lib.ngravs_sph_accelerations(None, None, None, None, None) == -1


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "plummer"])
def test_equal_to_the_existing_calls_bit_for_bit(pkg, kind):
    s, col, res, dens, hyd = full_run(pkg, kind)
    assert_is_the_sequence(res, col, dens, hyd, s.gas, kind)
    assert res["max_rounds"] == dens["max_rounds"] > 1
    other = np.ones(s.n, dtype=bool)
    other[s.gas] = False
    for k in COLS:
        assert np.isnan(col[k][other]).all(), k         # rows of other types: neither read (NaN in) nor written
    for k in OUTS:
        assert np.all(res[k][other] == 0), k
    assert len(res["kernel_ms"]) == 3 and all(t > 0 for t in res["kernel_ms"])


@pytest.mark.gpu
@pytest.mark.parametrize("gamma", [GAMMA, 1.0])
def test_pressure_line(pkg, gamma):
    s = gas_set(pkg, "uniform")
    eng = D.make_engine(pkg, True, s.pos, s.mass, s.ptype)
    col = start_columns(s)
    res = gas_call(eng, s, col, gamma=gamma)
    g = s.gas
    dt_entr = dt_entr_of(s)
    want = (s.A[g] + s.dA[g] * dt_entr[g]) * col["density"][g] ** gamma
    err = np.max(np.abs(col["pressure"][g] - want) / want)
    # the inputs exercise the line: the integer midpoint differs from the exact one on the odd steps, DtEntropy moves the entropy
    odd = ((s.beg[g].astype(np.int64) + s.end[g]) % 2) == 1
    exact = (s.A[g] + s.dA[g] * (TI - 0.5 * (s.beg[g].astype(np.float64) + s.end[g])) * s.tbi) * col["density"][g] ** gamma
    print("pressure line gamma %.4f: worst relative %.2e; %d odd midpoints of %d move the pressure by up to %.2e" %
          (gamma, err, odd.sum(), len(g), np.max(np.abs(exact - want) / want)))
    assert odd.sum() > 0.2 * len(g) and np.max((np.abs(exact - want) / want)[odd]) > 1e6 * TOL
    assert np.max(np.abs(s.A[g] * col["density"][g] ** gamma - want) / want) > 1e6 * TOL
    assert np.all(want > 0) and err <= TOL, err
    # and the hydro stage saw this pressure and this gamma
    dens, hyd = sequence(eng, s, s.hsml0, col, gamma=gamma)
    assert_is_the_sequence(res, col, dens, hyd, g, "gamma %g" % gamma)
    if gamma == 1.0:
        assert np.all(res["dt_entropy_out"][g] == 0)          # GAMMA_MINUS1 = 0 (hydra.c:320)
    # no ti columns: dt_entr = 0 and every timestep 0; no DtEntropy: 0
    col2 = start_columns(s)
    res2 = gas_call(eng, s, col2, gamma=gamma, dt_entropy=None, ti_begstep=None, ti_endstep=None)
    want2 = s.A[g] * col2["density"][g] ** gamma
    assert np.max(np.abs(col2["pressure"][g] - want2) / want2) <= TOL
    hyd2 = H.call(eng, s.vel, col2, art_bulk_visc_const=VISC, timestep=None, timebase_interval=s.tbi, gamma=gamma)
    assert np.array_equal(res2["hydro_accel"][g], hyd2["hydro_accel"][g]) and np.array_equal(res2["dt_entropy_out"][g], hyd2["dt_entropy"][g])
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("name", REF.FIXTURES)
def test_against_the_references_own_chain(pkg, name):
    """density() -> pressure line -> hydro_force() of the reference in ONE run (the executables where present, else their recorded
    output on the same inputs) against ONE call of the device.  Every output column, every gas row, TOL of sum |terms|; flagged
    rows (the rule of tests/test_sph_reference.py) on these inputs: 0, so no row is left out.

    (The driver starts SphP.DtEntropy at 0; the DtEntropy term and the integer midpoint are held to numpy in test_pressure_line.)"""
    f = REF.fixture(name)
    pos, mass, ptype, vel, gas, box = f["pos"], f["mass"], f["ptype"], f["vel"], f["gas"], float(f["box"])
    n = len(pos)
    minh, tbi = float(f["min_gas_hsml"]), float(f["tbi"])
    hsml0, A = REF.fixture_full(f, "hsml0"), REF.fixture_full(f, "entropy")
    keys = REF.DENS_KEYS + ("pressure", "hydro_accel", "dt_entropy", "max_signal_vel")
    if R.available():
        out = R.run(pos, mass, ptype, vel, hsml0, box=box, min_gas_hsml=minh, entropy=A, visc=VISC, timestep=f["timestep"], tbi=tbi, timeout=REF.T_SMALL)
        passes, source = out["passes"], "executables"
    else:
        out, passes, source = {k: REF.fixture_full(f, "ref_" + k) for k in keys}, int(f["ref_passes"]), "recorded"
    # the timeline marks as the driver sets them for rows that are all active (oracle/ref_sph.py)
    ts = np.where(ptype == 0, f["timestep"], 0).astype(np.int32)
    end = np.full(n, R.TI_CURRENT, dtype=np.int32)
    beg = (end - ts).astype(np.int32)
    other = np.ones(n, dtype=bool)
    other[gas] = False
    col = {k: np.full(n, np.nan) for k in COLS}
    col["hsml"][gas] = hsml0[gas]
    eng = D.make_engine(pkg, bool(box), pos, mass, ptype)
    res = eng.sph_accelerations(vel, np.where(other, np.nan, A), *(col[k] for k in COLS), ti_begstep=beg, ti_endstep=end, ti_current=R.TI_CURRENT,
                                timebase_interval=tbi, des_num_ngb=DES, max_num_ngb_deviation=DEV, min_gas_hsml=minh, art_bulk_visc_const=VISC)
    eng.close()
    print("sph accelerations, fixture %s against the reference (%s): max_rounds %d, passes %d" % (name, source, res["max_rounds"], passes))
    assert res["max_rounds"] == passes
    dev = dict(col, num_ngb=res["num_ngb"])
    REF.device_density_vs_reference(dev, out, pos, mass, vel, ptype, gas, box, "one call, fixture " + name)
    p_err = REF.rel(col["pressure"][gas], out["pressure"][gas])
    print("sph accelerations, fixture %s: pressure %.2e" % (name, p_err))
    assert p_err <= TOL
    ref_col = {k: H.full(n, gas, out[k][gas]) for k in COLS}
    hyd = {"hydro_accel": res["hydro_accel"], "dt_entropy": res["dt_entropy_out"], "max_signal_vel": res["max_signal_vel"]}
    REF.device_hydro_vs_reference(hyd, out, pos, mass, vel, ptype, gas, ref_col, box, "one call, fixture " + name, timestep=f["timestep"], tbi=tbi)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["uniform", "plummer"])
def test_active_subset_on_a_refit_tree(pkg, kind):
    s, col0, _, _, _ = full_run(pkg, kind)
    rng = np.random.default_rng(3)
    active = (rng.uniform(size=s.n) < 1.0 / 3).astype(np.uint8)
    targets = s.gas[active[s.gas] != 0]
    idle = s.gas[active[s.gas] == 0]
    assert len(targets) > 800 and len(idle) > 1800
    eng = D.make_engine(pkg, s.periodic, s.pos, s.mass, s.ptype, active=active)
    pos2 = s.pos + 0.02 * (s.box if s.periodic else 1.0) / 20 * rng.normal(size=s.pos.shape)
    if s.periodic:
        pos2 = np.mod(pos2, s.box)
    eng.update_particles(pos2, s.mass, s.ptype, active=active)        # the kept tree is refit by the call
    col = {k: a.copy() for k, a in col0.items()}
    out = sentinels(s.n)
    res = gas_call(eng, s, col, out=out)
    other = np.ones(s.n, dtype=bool)
    other[targets] = False
    for k in COLS:       # every row that is no target keeps its SphP columns bit for bit (NaN where it is no gas)
        assert np.array_equal(col[k][other], col0[k][other], equal_nan=True), k
        assert k == "hsml" or np.mean(col[k][targets] != col0[k][targets]) > 0.99, k        # the drift moved them (a length may stay accepted)
    for k in OUTS:
        assert np.all(res[k][other] == SENTINEL) and np.all(res[k][targets] != SENTINEL), k
    # the targets: the existing calls on the same state (the idle rows' columns of the step before are their sources)
    dens, hyd = sequence(eng, s, col0["hsml"], col)
    assert_is_the_sequence(res, col, dens, hyd, targets, kind + " active, refit tree")
    assert np.array_equal(dens["hsml"][idle], col0["hsml"][idle])
    eng.close()


@pytest.mark.gpu
def test_a_partial_last_wave_of_targets(pkg):
    """4 099 = 64 * 64 + 3 gas targets among 1 000 others, interleaved in caller order"""
    s, col, res, dens, hyd = full_run(pkg, "uniform", n=5099, ngas=4099, seed=32)
    assert len(s.gas) == 4099 and np.any(np.diff(s.gas) > 1) and np.any(np.diff(s.gas) == 1)
    assert_is_the_sequence(res, col, dens, hyd, s.gas, "4099")
    g = s.gas
    want = (s.A[g] + s.dA[g] * dt_entr_of(s)[g]) * col["density"][g] ** GAMMA
    assert np.max(np.abs(col["pressure"][g] - want) / want) <= TOL


@pytest.mark.gpu
def test_fewer_than_a_wave_of_targets_and_none(pkg):
    s, col0, _, _, _ = full_run(pkg, "uniform")
    active = np.zeros(s.n, dtype=np.uint8)
    targets = s.gas[7::80]
    assert 0 < len(targets) < 64
    active[targets] = 1
    active[s.ptype != 0] = 1                         # active rows of other types are no targets
    eng = D.make_engine(pkg, True, s.pos, s.mass, s.ptype, active=active)
    col = {k: a.copy() for k, a in col0.items()}
    res = gas_call(eng, s, col, out=sentinels(s.n))
    dens, hyd = sequence(eng, s, col0["hsml"], col)
    assert_is_the_sequence(res, col, dens, hyd, targets, "%d targets" % len(targets))
    other = np.ones(s.n, dtype=bool)
    other[targets] = False
    for k in COLS:
        assert np.array_equal(col[k][other], col0[k][other], equal_nan=True), k
    for k in OUTS:
        assert np.all(res[k][other] == SENTINEL), k
    eng.close()
    # no type-0 target at all: success, nothing written, 0 rounds -- with no gas, and with gas that is not active
    for ptype, act in ((np.where(s.ptype == 0, 1, s.ptype).astype(np.int32), None), (s.ptype, (s.ptype != 0).astype(np.uint8))):
        eng = D.make_engine(pkg, True, s.pos, s.mass, ptype, active=act)
        col = {k: a.copy() for k, a in col0.items()}
        res = gas_call(eng, s, col, out=sentinels(s.n))
        assert res["max_rounds"] == 0 and res["kernel_ms"] == [0.0, 0.0, 0.0]
        for k in COLS:
            assert np.array_equal(col[k], col0[k], equal_nan=True), k
        for k in OUTS:
            assert np.all(res[k] == SENTINEL), k
        eng.close()


@pytest.mark.gpu
def test_device_tensors_give_the_host_result(pkg):
    """zero-copy hand-over: torch device tensors in, updated in place, device tensors out; bit for bit what host arrays give -- on an
    active subset, so that the rows that are no targets are read from the device columns and must stay as they are"""
    import torch
    s, col0, _, _, _ = full_run(pkg, "uniform")
    active = (np.random.default_rng(4).uniform(size=s.n) < 0.5).astype(np.uint8)
    targets = s.gas[active[s.gas] != 0]
    eng = D.make_engine(pkg, True, s.pos, s.mass, s.ptype, active=active)
    col = {k: a.copy() for k, a in col0.items()}
    host = gas_call(eng, s, col, out=sentinels(s.n))
    up = lambda a: torch.from_numpy(a).cuda()   # noqa: E731
    dcol = {k: up(a) for k, a in col0.items()}
    dout = {k: up(a) for k, a in sentinels(s.n).items()}
    dev = eng.sph_accelerations(up(s.vel), up(s.A), *(dcol[k] for k in COLS), dt_entropy=up(s.dA), ti_begstep=up(s.beg), ti_endstep=up(s.end),
                                ti_current=TI, timebase_interval=s.tbi, des_num_ngb=DES, max_num_ngb_deviation=DEV, art_bulk_visc_const=VISC,
                                out=dout)
    eng.close()
    assert dev["max_rounds"] == host["max_rounds"]
    for k in COLS:
        assert dcol[k].is_cuda and np.array_equal(dcol[k].cpu().numpy(), col[k], equal_nan=True), k
    for k in OUTS:
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), host[k]), k
    assert np.all(host["num_ngb"][targets] != SENTINEL) and (host["num_ngb"] == SENTINEL).sum() == s.n - len(targets)


@pytest.mark.gpu
def test_c_abi_with_interleaved_columns_is_bit_identical(pkg):
    """every column a strided view of ONE interleaved array (the Python front always passes contiguous columns)"""
    s, col0, res0, _, _ = full_run(pkg, "uniform")
    eng = D.make_engine(pkg, True, s.pos, s.mass, s.ptype)
    L, abi = pkg.lib(), pkg.abi
    # one row = [vel x 3, entropy, dt_entropy, (beg, end) as two int32 in one slot, pad, the six in/out, pad, num_ngb, accel x 3,
    #            dt_entropy_out, pad, max_signal_vel] doubles
    W = 21
    buf = np.full((s.n, W), SENTINEL)
    buf[:, 0:3], buf[:, 3], buf[:, 4] = s.vel, s.A, s.dA
    iv = buf.view(np.int32).reshape(s.n, 2 * W)
    iv[:, 10], iv[:, 11] = s.beg, s.end
    start = start_columns(s)
    for c, k in enumerate(COLS):
        buf[:, 7 + c] = start[k]
    before = buf.copy()
    at = lambda c: buf.ctypes.data + 8 * c   # noqa: E731
    gi, go = abi.GasIn(), abi.GasOut()
    for k, c in (("vel_pred", 0), ("entropy", 3), ("dt_entropy", 4), ("ti_begstep", 5)) + tuple((k, 7 + c) for c, k in enumerate(COLS)):
        setattr(gi, k, at(c))
        setattr(gi, k + "_stride", 8 * W)
    gi.ti_endstep, gi.ti_endstep_stride = at(5) + 4, 8 * W
    gi.des_num_ngb, gi.max_num_ngb_deviation, gi.art_bulk_visc_const, gi.timebase_interval, gi.gamma = DES, DEV, VISC, s.tbi, GAMMA
    gi.ti_current, gi.viscosity_limiter = TI, 1
    for k, c in (("num_ngb", 14), ("hydro_accel", 15), ("dt_entropy_out", 18), ("max_signal_vel", 20)):
        setattr(go, k, at(c))
        setattr(go, k + "_stride", 8 * W)
    rounds, ms = C.c_int32(0), (C.c_double * 3)()
    assert L.ngravs_sph_accelerations(eng._h, C.byref(gi), C.byref(go), C.byref(rounds), ms) == 0, L.ngravs_last_error(eng._h)
    eng.close()
    g = s.gas
    other = np.ones(s.n, dtype=bool)
    other[g] = False
    assert rounds.value == res0["max_rounds"]
    for c, k in enumerate(COLS):
        assert np.array_equal(buf[g, 7 + c], col0[k][g]), k
    assert np.array_equal(buf[g, 14], res0["num_ngb"][g]) and np.array_equal(buf[g, 15:18], res0["hydro_accel"][g])
    assert np.array_equal(buf[g, 18], res0["dt_entropy_out"][g]) and np.array_equal(buf[g, 20], res0["max_signal_vel"][g])
    assert np.array_equal(buf[other], before[other], equal_nan=True)           # rows of other types: untouched, all of the row
    assert np.array_equal(buf[:, [0, 1, 2, 3, 4, 5, 6, 13, 19]], before[:, [0, 1, 2, 3, 4, 5, 6, 13, 19]], equal_nan=True)   # inputs and padding


@pytest.mark.gpu
def test_refusals_write_nothing(pkg):
    s, col0, _, _, _ = full_run(pkg, "uniform")
    cfg_kw = dict(n_gravs=2, periodic=1, box_size=1000.0, softening=[0.01] * 6, type_to_grav=[0, 0, 1, 0, 0, 0], walk_mode=pkg.WALK_GROUP)
    active = np.ones(s.n, dtype=np.uint8)
    idle = s.gas[5::3]
    active[idle] = 0
    target = s.gas[3]
    assert active[target] == 1

    def refused(eng, match, edit=None, **kw):
        """the call raises `match`, and every in/out and out-only array is afterwards what it was before"""
        col = {k: a.copy() for k, a in col0.items()}
        if edit:
            col[edit[0]][edit[1]] = edit[2]
        keep = {k: a.copy() for k, a in col.items()}
        out = sentinels(s.n)
        with pytest.raises(pkg.NgravsError, match=match):
            gas_call(eng, s, col, out=out, **kw)
        for k in COLS:
            assert np.array_equal(col[k], keep[k], equal_nan=True), (match, k)
        for k in OUTS:
            assert np.all(out[k] == SENTINEL), (match, k)

    eng = pkg.Engine(pkg.make_config(**cfg_kw))
    eng.set_particles(s.pos, s.mass, s.ptype, active=active)
    refused(eng, "ngravs_sph_accelerations.*status -4.*built tree")
    eng.domain_Decomposition()
    eng.force_treebuild()
    two = pkg.Engine(pkg.make_config(world_size=2, rank=0, **cfg_kw))
    two.set_particles(s.pos, s.mass, s.ptype)
    refused(two, "status -4.*single task only")
    two.close()
    # arguments
    refused(eng, "status -1.*des_num_ngb", des_num_ngb=0.0)
    refused(eng, "status -1.*max_num_ngb_deviation", max_num_ngb_deviation=-1.0)
    refused(eng, "status -1.*gamma", gamma=0.5)
    refused(eng, "status -1.*art_bulk_visc_const", art_bulk_visc_const=-1.0)
    refused(eng, "status -1.*comoving", comoving=(0.0, 1.0, 1.0))
    refused(eng, "status -1.*ti_begstep and ti_endstep", ti_begstep=None)
    L = pkg.lib()
    assert L.ngravs_sph_accelerations(eng._h, None, None, None, None) == -1 and b"NULL" in L.ngravs_last_error(eng._h)
    gi = pkg.abi.GasIn()
    assert L.ngravs_sph_accelerations(eng._h, C.byref(gi), None, None, None) == -1 and b"NULL" in L.ngravs_last_error(eng._h)
    # a target's starting guess
    for value in (0.0, -1.0, np.inf, np.nan):
        refused(eng, "status -1.*target's starting hsml", edit=("hsml", target, value))
    # a gas row that is no target is a source with the columns given: the message names the column; a bad pressure is refused
    # before any density output is written (refused() checks hsml, density, ... of the targets too)
    for name, value in (("hsml", 0.0), ("hsml", np.inf), ("density", -1.0), ("density", np.nan), ("pressure", -1e-3), ("pressure", np.nan)):
        refused(eng, "status -1.*type-0 row's %s" % name, edit=(name, idle[11], value))
    # a target's other five columns are not read
    col = {k: a.copy() for k, a in col0.items()}
    for k in COLS[1:]:
        col[k][s.gas[active[s.gas] != 0]] = np.nan
    ok = gas_call(eng, s, col)
    assert np.isfinite(col["pressure"][s.gas]).all() and np.isfinite(ok["hydro_accel"]).all()
    # ... but its entropy makes its pressure
    bad = types.SimpleNamespace(**vars(s))
    bad.A = s.A.copy()
    bad.A[target] = np.nan
    col = {k: a.copy() for k, a in col0.items()}
    with pytest.raises(pkg.NgravsError, match="status -1.*type-0 row's pressure"):
        gas_call(eng, bad, col)
    assert all(np.array_equal(col[k], col0[k], equal_nan=True) for k in COLS)
    eng.close()


@pytest.mark.gpu
def test_maxiter_ends_in_the_fatal_handler_before_the_hydro_stage(pkg):
    """six gas particles in one place: NumNgb = 6 * NORM_COEFF * KC1 = 64 > DesNumNgb + MaxNumNgbDeviation at every h > 0, with no
    MinGasHsml the length is divided by 1.26 until MAXITER (density.c:416: endrun(1155))"""
    s, col0, _, _, _ = full_run(pkg, "uniform")
    pos = s.pos.copy()
    pos[s.gas[:6]] = pos[s.gas[0]]
    eng = D.make_engine(pkg, True, pos, s.mass, s.ptype)
    seen = []
    handler = pkg.lib().ngravs_set_fatal_handler
    FATAL = C.CFUNCTYPE(None, C.c_int, C.c_char_p)
    cb = FATAL(lambda code, msg: seen.append((code, msg)))
    handler.argtypes = [C.c_void_p, FATAL]
    handler.restype = None
    handler(eng._h, cb)
    col = start_columns(s)
    keep = {k: a.copy() for k, a in col.items()}
    out = sentinels(s.n)
    with pytest.raises(pkg.NgravsError, match="status -4.*failed to converge"):
        gas_call(eng, s, col, out=out)
    assert [c for c, _ in seen] == [1155]
    assert all(np.array_equal(col[k], keep[k], equal_nan=True) for k in COLS) and all(np.all(out[k] == SENTINEL) for k in OUTS)
    # the existing density call ends the same way on this set
    with pytest.raises(pkg.NgravsError, match="status -4.*failed to converge"):
        eng.sph_density(s.vel, s.hsml0, DES, DEV)
    assert [c for c, _ in seen] == [1155, 1155]
    eng.close()


@pytest.mark.gpu
def test_gravity_density_and_hydro_are_not_disturbed(pkg):
    s, col0, _, _, _ = full_run(pkg, "uniform")
    eng = D.make_engine(pkg, True, s.pos, s.mass, s.ptype)
    d0, h0 = sequence(eng, s, s.hsml0, col0)
    col = start_columns(s)
    gas_call(eng, s, col)
    d1, h1 = sequence(eng, s, s.hsml0, col0)
    # (hsml of a row that is no gas is the NaN that went in, on both sides: equal_nan; the gas rows hold numbers)
    for k in ("hsml",) + tuple(pkg.abi.SPH_OUT_NAMES):
        assert np.array_equal(d0[k], d1[k], equal_nan=True) and np.isfinite(d0[k][s.gas]).all() and np.all(d0[k][s.gas] != 0), k
    for k in pkg.abi.HYDRO_OUT_NAMES:
        assert np.array_equal(h0[k], h1[k]) and np.isfinite(h0[k]).all() and np.any(h0[k][s.gas] != 0), k
    eng.gravity_tree()
    acc1, _, cost1 = eng.get_accel()
    plain = D.make_engine(pkg, True, s.pos, s.mass, s.ptype)
    plain.gravity_tree()
    acc0, _, cost0 = plain.get_accel()
    assert np.array_equal(acc0, acc1) and np.array_equal(cost0, cost1)
    eng.close()
    plain.close()
