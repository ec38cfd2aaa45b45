"""SPH density and hydro force against the reference's OWN density() / hydro_force(), run single-task from oracle/_ref/.

tests/test_sph_density.py and tests/test_sph_hydro.py hold the device to numpy restatements of density.c / hydra.c.  Kernel and
restatement come from one reading of those files, so a shared misreading passes there.  Here the truth is the reference itself:
oracle/_ref/ref_sph_{open,periodic,periodic_isotherm,periodic_nolimiter} are density.c, hydra.c, ngb.c, forcetree.c, domain.c, ...
compiled unmodified (`make -C oracle ref`; MPI / GSL / FFTW-2 replaced by the stand-ins of oracle/ref_stubs/, through which nothing
numerical passes), driven by oracle/ref_sph_driver.c through the reference's own domain_Decomposition(), ngb_treebuild(),
density(), force_update_hmax(), hydro_force().

CPU tests hold the RESTATEMENTS to the reference on the inputs of the two existing modules; GPU tests hold the DEVICE to the
reference directly (the restatement only supplies the sum of |terms| that scales the error of a cancelling sum, never a value
that is compared).  tests/golden/sph_reference_{periodic,open}.npz (tests/golden/make_sph_reference_golden.py) record inputs and
reference outputs of two small mixed sets, so a checkout without the reference tree still pins restatement and device to it.

Tolerance: TOL = 1e-11, the figure and the scales of compare() of the two existing modules (relative for hsml, density, num_ngb,
dhsml_factor, pressure, max_signal_vel; against sum |terms| for div_vel, curl_vel, hydro_accel, dt_entropy).  The reference sums
in tree order, the restatement in index order, the device in leaf order.
Borderline targets (NumNgb of some round within 1e-9 relative of a decision bound; a pair within 1e-9 of r2 = h^2 for
max_signal_vel): flagged by the restatement, left out, at most 0.1 % (the existing rule and cap).  Counted on the CPU for every
input of this module: 0 flagged in all of them (parity 2 x 12 000, clamped and bracket-accept 2 x 2 x 4 000, active, coincident, hmax 12 000, degenerate,
both fixture sets 2 x 2 000).  The GPU tests therefore leave NOTHING out: every gas row is compared.  The large run is not run
through the restatement's iteration; it, too, leaves nothing out, which is the stricter reading.
Passes of density()'s outer loop: counted from the reference's own "ngb iteration K" progress lines (no change to the
reference) and compared with the restatement's rounds and the device's max_rounds.
Hydro alone (driver mode 1) is fed the same SphP columns on both sides, Pressure included; the reference's own pressure line
(density.c:307) is exercised by the chain tests, where Entropy = A and the reference's Pressure is compared with A rho^gamma.

Measured on the CPU (seconds, reference executable alone): parity 12 000 gas chain 5.2 (uniform) / 6.9 (Plummer), hydro alone on
12 000 gas 1.5 / 2.0, the 4 000-gas sets 1.0-1.8, fixture sets 0.6; large periodic run 2^16: 6.7, 2^18: 46.6, 2^19: 127.4, 2^20: 302.8;
the per-row scale sums of the large run (all_row_scales) 170 at 2^19.
The large run is 2^19: at 2^20 the reference alone takes longer than the rest of this module together, and with it the module would
not stay within the CPU-side time of the two existing SPH modules (about 500 s: their restatements at 24 s per 12 000-gas set).
Each subprocess gets three times its measured time, rounded up to 10 s (T_* below).
"""
import importlib.util
import os
import sys

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


H = _load("test_sph_hydro", os.path.join(HERE, "test_sph_hydro.py"))
D = H.D
R = _load("ngravs_ref_sph", os.path.join(HERE, "..", "oracle", "ref_sph.py"))
TOL, DES, DEV, GAMMA, VISC = D.TOL, D.DES, D.DEV, H.GAMMA, H.VISC
GOLDEN = os.path.join(HERE, "golden")
T_SMALL, T_CHAIN, T_LARGE = 10.0, 30.0, 390.0      # 3 x (<= 2.0 s), 3 x 6.9 s, 3 x 127.4 s: rounded up to 10 s
LARGE_LOG2 = 19

need_ref = pytest.mark.skipif(not R.available(), reason="oracle/_ref/ref_sph_* are absent: build them with `%s`" % R.MAKE_TARGET)


# ---- comparisons ----------------------------------------------------------------------------------------------------------
def rel(a, b):
    return float(np.max(np.abs(a - b) / np.abs(b))) if len(b) else 0.0


def density_vs_reference(out, ref, rows, what):
    """restatement `ref` (arrays over `rows`) against the reference's result `out` (arrays over all rows): compare() of
    test_sph_density.py, the same quantities on the same scales, with the reference in the place of the device"""
    return D.compare(out, ref, rows, what="restatement vs reference, " + what)


def hydro_vs_reference(out, ref, rows, what):
    return H.compare(out, ref, rows, what="restatement vs reference, " + what)


def device_density_vs_reference(res, out, pos, mass, vel, ptype, rows, box, what):
    """device `res` against reference `out` on `rows`; div / curl scales = sum |terms| of one brute-force evaluation AT the
    reference's lengths (a scale, not a value)"""
    sc, _ = D.restate(pos, mass, vel, ptype, rows, out["hsml"][rows], DES, DEV, box=box, one_round=True)
    ref = {k: out[k][rows] for k in ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor")}
    ref.update(div_scale=sc["div_scale"], curl_scale=sc["curl_scale"], flagged=np.zeros(len(rows), dtype=bool))
    return D.compare(res, ref, rows, what="device vs reference, " + what)


def device_hydro_vs_reference(res, out, pos, mass, vel, ptype, rows, col, box, what, **kw):
    sc, _ = H.hydro_restate(pos, mass, vel, ptype, rows, col, box, **kw)
    ref = {"hydro_accel": out["hydro_accel"][rows], "dt_entropy": out["dt_entropy"][rows], "max_signal_vel": out["max_signal_vel"][rows],
           "acc_scale": sc["acc_scale"], "dte_scale": sc["dte_scale"], "flagged": np.zeros(len(rows), dtype=bool)}
    return H.compare(res, ref, rows, what="device vs reference, " + what)


def all_row_scales(pos, mass, vel, col, box, timestep, tbi):
    """sum |terms| of div_vel, curl_vel, hydro_accel and dt_entropy for EVERY row of an all-gas periodic set, in O(N ngb): the box
    is cut into cells of side >= max(hsml); the rows of a block of 2 x 2 x 2 cells are the targets of the restatements' own scale
    sums (D.restate, one evaluation at col["hsml"]; H.hydro_restate) over the particles of the block and the one-cell layer
    around it, which holds every particle within max(hsml) of a target, i.e. every pair with r2 < h_i^2 or r2 < h_j^2.  The
    sums are the restatements' own code on a subset that contains all the terms, so the scales are those of compare(), on
    every row (checked against the direct O(N^2) sums on the CPU: equal to 1.3e-15).
    Returns div_scale, curl_scale, acc_scale [n, 3], dte_scale and the union of the hydro branch logs."""
    n = len(pos)
    nc = int(box // float(col["hsml"].max()))
    assert nc >= 4, "the box holds fewer than 4 cells of side max(hsml): a cell list gains nothing"
    ci = np.minimum((pos / (box / nc)).astype(np.int64), nc - 1)
    cell = (ci[:, 0] * nc + ci[:, 1]) * nc + ci[:, 2]
    order = np.argsort(cell, kind="stable")
    start = np.searchsorted(cell[order], np.arange(nc ** 3 + 1))
    sc = {"div_scale": np.zeros(n), "curl_scale": np.zeros(n), "acc_scale": np.zeros((n, 3)), "dte_scale": np.zeros(n)}
    log = set()
    in_block = np.zeros(n, dtype=bool)
    blocks = [np.arange(b, min(b + 2, nc)) for b in range(0, nc, 2)]
    for bx in blocks:
        for by in blocks:
            for bz in blocks:
                layer = [np.unique(np.arange(b[0] - 1, b[-1] + 2) % nc) for b in (bx, by, bz)]
                cells = ((layer[0][:, None, None] * nc + layer[1][None, :, None]) * nc + layer[2][None, None, :]).ravel()
                sub = np.concatenate([order[start[c]:start[c + 1]] for c in cells])
                own = ((bx[:, None, None] * nc + by[None, :, None]) * nc + bz[None, None, :]).ravel()
                rows = np.concatenate([order[start[c]:start[c + 1]] for c in own])
                if not len(rows):
                    continue
                in_block[rows] = True
                t = np.nonzero(in_block[sub])[0]
                in_block[rows] = False
                rows = sub[t]
                gas_type = np.zeros(len(sub), dtype=np.int32)
                d, _ = D.restate(pos[sub], mass[sub], vel[sub], gas_type, t, col["hsml"][rows], DES, DEV, box=box, one_round=True)
                sc["div_scale"][rows], sc["curl_scale"][rows] = d["div_scale"], d["curl_scale"]
                h, lg = H.hydro_restate(pos[sub], mass[sub], vel[sub], gas_type, t, {k: a[sub] for k, a in col.items()}, box,
                                        timestep=timestep[sub], tbi=tbi)
                sc["acc_scale"][rows], sc["dte_scale"][rows] = h["acc_scale"], h["dte_scale"]
                log |= lg
    return sc, log


def entropy_of(n, gas, seed):
    """the A of hydro_columns(): pressure = A rho^gamma"""
    return H.full(n, gas, 10.0 ** np.random.default_rng(seed).uniform(-0.5, 0.5, len(gas)), fill=0.0)


_CACHE = {}


def cached(key, fn):
    if key not in _CACHE:
        _CACHE[key] = fn()
    return _CACHE[key]


# ---- CPU: the density restatement against density() -----------------------------------------------------------------------
@need_ref
@pytest.mark.parametrize("kind,periodic", D.CASES)
def test_density_restatement_parity_inputs(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, kind)
    box = 1000.0 if periodic else 0.0
    ref, log = D.restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    for rule in ("left", "right", "bisect", "newton", "grow_1.26", "shrink_1.26"):
        assert rule in log, (rule, log)
    out = R.run(pos, mass, ptype, vel, hsml, box=box, timeout=T_CHAIN)
    assert ref["flagged"].sum() == 0
    density_vs_reference(out, ref, gas, kind)
    assert out["passes"] == ref["rounds"].max(), (out["passes"], ref["rounds"].max())


@need_ref
@pytest.mark.parametrize("kind,periodic", D.CASES)
def test_density_restatement_clamped(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=11)
    box = 1000.0 if periodic else 0.0
    free, _ = D.restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    minh = float(np.quantile(free["hsml"], 1.0 / 3))
    ref, log = D.restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, minh=minh, box=box)
    assert "clamp" in log and "accept_at_min" in log
    out = R.run(pos, mass, ptype, vel, hsml, box=box, min_gas_hsml=minh, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    density_vs_reference(out, ref, gas, kind + " clamped")
    assert out["passes"] == ref["rounds"].max()
    clamped = out["hsml"][gas] == minh
    assert 0.25 * len(gas) < clamped.sum() < 0.42 * len(gas) and np.any(out["num_ngb"][gas][clamped] > DES + DEV)


@need_ref
@pytest.mark.parametrize("kind,periodic", D.CASES)
def test_density_restatement_active_subset(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=12)
    box = 1000.0 if periodic else 0.0
    active = (np.random.default_rng(3).uniform(size=len(pos)) < 0.4).astype(np.uint8)
    targets = gas[active[gas] != 0]
    hsml = np.where(np.isin(np.arange(len(pos)), targets), hsml, -7.0)
    ref, _ = D.restate(pos, mass, vel, ptype, targets, hsml[targets], DES, DEV, box=box)
    out = R.run(pos, mass, ptype, vel, hsml, box=box, active=active, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    density_vs_reference(out, ref, targets, kind + " active")
    idle = gas[active[gas] == 0]
    assert np.all(out["hsml"][idle] == -7.0) and np.all(out["density"][idle] == 0)      # density() leaves the others alone


@need_ref
@pytest.mark.parametrize("periodic", [True, False])
def test_density_restatement_coincident_pair_and_three_faces(pkg, periodic):
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, "uniform", n=6000, ngas=4000, seed=13)
    box = 1000.0 if periodic else 0.0
    pos[gas[1]] = pos[gas[0]]
    pos[gas[2]] = [0.4, 999.7, 0.2]
    ref, _ = D.restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    out = R.run(pos, mass, ptype, vel, hsml, box=box, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    density_vs_reference(out, ref, gas, "coincident, periodic %d" % periodic)
    assert np.isfinite(out["div_vel"][gas[:3]]).all() and np.isfinite(out["curl_vel"][gas[:3]]).all()


TIGHT_DEV = 0.01      # a band of +-0.01 around DesNumNgb is ~1.3e-4 wide in h (dN/dlnh ~ 3 N): narrower than the 1e-3 bracket rule


@need_ref
@pytest.mark.parametrize("kind,periodic", D.CASES)
def test_density_restatement_bracket_accept(pkg, kind, periodic):
    """MaxNumNgbDeviation so small that the bisection bracket closes to 1e-3 before NumNgb reaches the band: the bracket-accept
    rule (density.c:321-328) decides the result, and its place BEFORE the bracket update matters (none of the inputs of the two
    existing modules fires it)"""
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=11)
    box = 1000.0 if periodic else 0.0
    ref, log = D.restate(pos, mass, vel, ptype, gas, hsml[gas], DES, TIGHT_DEV, box=box)
    assert "accept_bracket" in log and "bisect" in log
    out = R.run(pos, mass, ptype, vel, hsml, box=box, dev=TIGHT_DEV, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    density_vs_reference(out, ref, gas, kind + " bracket accept")
    assert out["passes"] == ref["rounds"].max()
    outside = np.abs(out["num_ngb"][gas] - DES) > TIGHT_DEV
    assert outside.sum() > 0.1 * len(gas), outside.sum()        # accepted by the bracket rule, not by the band


# ---- CPU: the hydro restatement against hydro_force() ---------------------------------------------------------------------
def parity_restatement(pkg, kind):
    def make():
        pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, kind)
        return H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=H.KIND_TBI[kind])
    return cached(("parity", kind), make)


@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_hydro_restatement_parity_inputs(pkg, kind, periodic):
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, kind)
    ref, log = parity_restatement(pkg, kind)
    for b in H.BRANCHES:
        assert b in log, (b, log)
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=H.KIND_TBI[kind], timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    hydro_vs_reference(out, ref, gas, kind)


def hmax_columns(pkg):
    """the columns of test_node_hmax_brings_in_the_large_neighbours: 12 gas particles with 5 x the smoothing length"""
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, "uniform")
    big = np.sort(np.random.default_rng(77).choice(len(gas), 12, replace=False))
    h5 = 5.0 * col["hsml"][gas[big]]
    one, _ = D.restate(pos, mass, vel, ptype, gas[big], h5, DES, DEV, box=L, one_round=True)
    col = {k: a.copy() for k, a in col.items()}
    A = col["pressure"][gas[big]] / col["density"][gas[big]] ** GAMMA
    for k in H.COLS:
        if k != "pressure":
            col[k][gas[big]] = one[k]
    col["pressure"][gas[big]] = A * one["density"] ** GAMMA
    return col, big


@need_ref
def test_hydro_restatement_hmax(pkg):
    pos, mass, ptype, vel, _, timestep, gas, L = H.hydro_set(pkg, "uniform")
    col, big = hmax_columns(pkg)
    tbi = H.KIND_TBI["uniform"]
    ref, log = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=tbi)
    assert "only_hj" in log
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=tbi, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    hydro_vs_reference(out, ref, gas, "hmax")


@need_ref
def test_hydro_restatement_switches(pkg):
    """ISOTHERM_EQS and NOVISCOSITYLIMITER exist as periodic builds: the uniform box"""
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, "uniform")
    tbi = H.KIND_TBI["uniform"]
    common = dict(box=L, visc=VISC, timeout=T_SMALL)
    ref, log = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=tbi, limiter=False)
    assert "limiter_active" not in log
    out = R.run(pos, mass, ptype, vel, col["hsml"], columns=col, timestep=timestep, tbi=tbi, limiter=False, **common)
    hydro_vs_reference(out, ref, gas, "no limiter")
    lim, _ = parity_restatement(pkg, "uniform")
    assert np.max(np.abs(lim["dt_entropy"] - ref["dt_entropy"]) / ref["dte_scale"]) > 1e5 * TOL
    iso = dict(col, pressure=3.0 * col["density"])
    ref, _ = H.hydro_restate(pos, mass, vel, ptype, gas, iso, L, timestep=timestep, tbi=tbi, gamma=1.0)
    out = R.run(pos, mass, ptype, vel, col["hsml"], columns=iso, timestep=timestep, tbi=tbi, gamma=1.0, **common)
    hydro_vs_reference(out, ref, gas, "isothermal")
    assert np.all(out["dt_entropy"][gas] == 0)
    zero = np.zeros(len(pos), dtype=np.int32)                      # timestep 0 everywhere: dt = 0, the limiter never acts
    ref, log = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=zero, tbi=tbi)
    assert "limiter_dt0" in log and "limiter_active" not in log
    out = R.run(pos, mass, ptype, vel, col["hsml"], columns=col, timestep=zero, tbi=tbi, **common)
    hydro_vs_reference(out, ref, gas, "timestep 0")
    ref, _ = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=tbi, visc=0.0)
    out = R.run(pos, mass, ptype, vel, col["hsml"], columns=col, timestep=timestep, tbi=tbi, **dict(common, visc=0.0))
    hydro_vs_reference(out, ref, gas, "no viscosity")


@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_hydro_restatement_comoving(pkg, kind, periodic):
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, kind)
    tbi = H.KIND_TBI[kind]
    cosmo = (0.5, 0.3, 0.7, 0.1 if kind == "uniform" else 10.0)
    ref, log = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=tbi, comoving=pkg.hydro_factors(*cosmo))
    assert "comoving_flip" in log and "vdotr2_neg" in log
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=tbi, comoving=cosmo, timeout=T_SMALL)
    hydro_vs_reference(out, ref, gas, kind + " comoving")


def degenerate_set(pkg, periodic):
    """the input of test_coincident_pair_three_faces_and_a_lonely_particle"""
    pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, "uniform", n=6000, ngas=4000, seed=13)
    L = 1000.0 if periodic else 0.0
    lonely = gas[3]
    if periodic:
        pos[lonely] = [500.0, 500.0, 500.0]
        near = (np.sum((pos - pos[lonely]) ** 2, axis=1) < 350.0 ** 2) & (ptype == 0)
        near[lonely] = False
        ptype = np.where(near, 1, ptype).astype(np.int32)
        gas = np.nonzero(ptype == 0)[0]
    else:
        pos[lonely] = [500.0, 500.0, 5000.0]
    a, b, corner = [g for g in gas if g != lonely][:3]
    pos[b] = pos[a]
    pos[corner] = [0.4, 999.7, 0.2]
    col = H.hydro_columns(pos, mass, vel, ptype, gas, hsml0[gas], L, seed=13)
    col["hsml"][lonely] = 100.0
    tbi = H.KIND_TBI["uniform"] * 3.0 ** (1.0 / 3)
    timestep = np.full(len(pos), 4, dtype=np.int32)
    return pos, mass, ptype, vel, col, timestep, gas, L, tbi, lonely


@need_ref
@pytest.mark.parametrize("periodic", [True, False])
def test_hydro_restatement_degenerate(pkg, periodic):
    pos, mass, ptype, vel, col, timestep, gas, L, tbi, lonely = degenerate_set(pkg, periodic)
    ref, _ = H.hydro_restate(pos, mass, vel, ptype, gas, col, L, timestep=timestep, tbi=tbi)
    assert ref["pairs"][gas == lonely][0] == 0 and ref["flagged"].sum() == 0
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=tbi, timeout=T_SMALL)
    hydro_vs_reference(out, ref, gas, "degenerate, periodic %d" % periodic)
    assert np.all(out["hydro_accel"][lonely] == 0) and out["dt_entropy"][lonely] == 0 and out["max_signal_vel"][lonely] == 0


@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_hydro_restatement_active_subset(pkg, kind, periodic):
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, kind, n=6000, ngas=4000, seed=12)
    tbi = H.KIND_TBI[kind]
    active = (np.random.default_rng(3).uniform(size=len(pos)) < 0.4).astype(np.uint8)
    targets = gas[active[gas] != 0]
    ref, _ = H.hydro_restate(pos, mass, vel, ptype, targets, col, L, timestep=timestep, tbi=tbi)
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=tbi, active=active, timeout=T_SMALL)
    assert ref["flagged"].sum() == 0
    hydro_vs_reference(out, ref, targets, kind + " active")
    idle = gas[active[gas] == 0]
    assert np.all(out["hydro_accel"][idle] == 0) and np.all(out["max_signal_vel"][idle] == 0)


# ---- CPU: the chain ---------------------------------------------------------------------------------------------------------
def chain_vs(out, col, hyd, gas, what):
    """reference density() -> pressure line -> hydro_force() in ONE run against restatement density feeding restatement hydro"""
    worst = {k: rel(out[k][gas], col[k][gas]) for k in ("hsml", "density", "dhsml_factor", "pressure")}
    print("sph chain %s: %s" % (what, ", ".join("%s %.2e" % kv for kv in worst.items())))
    for k, v in worst.items():
        assert v <= TOL, (what, k, v)
    return H.compare(out, hyd, gas, what="chain, " + what)


@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_chain_restatements_against_density_then_hydro_force(pkg, kind, periodic):
    pos, mass, ptype, vel, col, timestep, gas, L = H.hydro_set(pkg, kind)
    hsml0 = D.gas_mix(pkg, kind)[4]
    hyd, _ = parity_restatement(pkg, kind)
    out = R.run(pos, mass, ptype, vel, hsml0, box=L, entropy=entropy_of(len(pos), gas, 5), visc=VISC, timestep=timestep, tbi=H.KIND_TBI[kind],
                timeout=T_CHAIN)
    chain_vs(out, col, hyd, gas, kind)


# ---- fixtures: inputs and reference outputs recorded by tests/golden/make_sph_reference_golden.py --------------------------
FIXTURES = ("periodic", "open")
DENS_KEYS = ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor")


def fixture(name):
    z = np.load(os.path.join(GOLDEN, "sph_reference_%s.npz" % name))
    return {k: z[k] for k in z.files}


def fixture_full(f, key):
    """a recorded gas-row array as an array over all rows"""
    a = np.zeros((len(f["pos"]),) + f[key].shape[1:])
    a[f["gas"]] = f[key]
    return a


@pytest.mark.parametrize("name", FIXTURES)
def test_restatements_against_the_recorded_reference(pkg, name):
    f = fixture(name)
    pos, mass, ptype, vel, gas, box = f["pos"], f["mass"], f["ptype"], f["vel"], f["gas"], float(f["box"])
    n = len(pos)
    minh, tbi = float(f["min_gas_hsml"]), float(f["tbi"])
    ref, log = D.restate(pos, mass, vel, ptype, gas, f["hsml0"], DES, DEV, minh=minh, box=box)
    assert "clamp" in log and "accept_at_min" in log and "bisect" in log and ref["flagged"].sum() == 0
    rec = {k: fixture_full(f, "ref_" + k) for k in DENS_KEYS + ("pressure", "hydro_accel", "dt_entropy", "max_signal_vel")}
    density_vs_reference(rec, ref, gas, "fixture " + name)
    assert int(f["ref_passes"]) == ref["rounds"].max()
    col = {k: H.full(n, gas, ref[k]) for k in H.COLS if k != "pressure"}
    col["pressure"] = H.full(n, gas, f["entropy"] * ref["density"] ** GAMMA)
    hyd, log = H.hydro_restate(pos, mass, vel, ptype, gas, col, box, timestep=f["timestep"], tbi=tbi)
    assert "limiter_active" in log and "limiter_dmin_second" in log and "limiter_dt0" in log and hyd["flagged"].sum() == 0
    chain_vs(rec, col, hyd, gas, "fixture " + name)
    clamped = f["ref_hsml"] == minh
    assert 0.25 * len(gas) < clamped.sum() < 0.42 * len(gas)


@need_ref
@pytest.mark.parametrize("name", FIXTURES)
def test_the_recorded_reference_is_what_the_executables_give(pkg, name):
    """the fixtures are not stale: the executables reproduce them bit for bit"""
    f = fixture(name)
    out = R.run(f["pos"], f["mass"], f["ptype"], f["vel"], fixture_full(f, "hsml0"), box=float(f["box"]), min_gas_hsml=float(f["min_gas_hsml"]),
                entropy=fixture_full(f, "entropy"), visc=VISC, timestep=f["timestep"], tbi=float(f["tbi"]), timeout=T_SMALL)
    for k in DENS_KEYS + ("pressure", "hydro_accel", "dt_entropy", "max_signal_vel"):
        assert np.array_equal(out[k][f["gas"]], f["ref_" + k]), k
    assert out["passes"] == int(f["ref_passes"])


# ---- GPU: the device against the reference ------------------------------------------------------------------------------------
def device_chain(pkg, eng, vel, hsml0, A, timestep, tbi, min_gas_hsml=0.0):
    """Engine.sph_density, the host pressure line (density.c:307 with DtEntropy = 0), Engine.sph_hydro"""
    dens = eng.sph_density(vel, hsml0, DES, DEV, min_gas_hsml=min_gas_hsml)
    col = {k: dens[k] for k in H.COLS if k != "pressure"}
    col["pressure"] = A * dens["density"] ** GAMMA
    hyd = H.call(eng, vel, col, art_bulk_visc_const=VISC, timestep=timestep, timebase_interval=tbi)
    return dens, col, hyd


def device_chain_vs_reference(pkg, periodic, pos, mass, ptype, vel, hsml0, A, timestep, tbi, gas, what, min_gas_hsml=0.0, t=T_CHAIN):
    box = 1000.0 if periodic else 0.0
    out = R.run(pos, mass, ptype, vel, hsml0, box=box, min_gas_hsml=min_gas_hsml, entropy=A, visc=VISC, timestep=timestep, tbi=tbi, timeout=t)
    eng = D.make_engine(pkg, periodic, pos, mass, ptype)
    dens, col, hyd = device_chain(pkg, eng, vel, hsml0, A, timestep, tbi, min_gas_hsml)
    eng.close()
    assert dens["max_rounds"] == out["passes"], (dens["max_rounds"], out["passes"])
    device_density_vs_reference(dens, out, pos, mass, vel, ptype, gas, box, what)
    assert rel(col["pressure"][gas], out["pressure"][gas]) <= TOL
    ref_col = {k: H.full(len(pos), gas, out[k][gas]) for k in H.COLS}
    device_hydro_vs_reference(hyd, out, pos, mass, vel, ptype, gas, ref_col, box, what, timestep=timestep, tbi=tbi)
    return out, dens, hyd


@pytest.mark.gpu
@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_device_chain_against_the_reference(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, kind)
    vel = vel - (0.02 * (pos - 500.0) if kind == "uniform" else 2.0 * pos)          # the converging flow of hydro_set
    rng = np.random.default_rng(105)
    timestep = (rng.choice([0, 1, 2, 4, 8], len(pos)) * 2 ** rng.integers(0, 4, len(pos))).astype(np.int32)
    device_chain_vs_reference(pkg, periodic, pos, mass, ptype, vel, hsml0, entropy_of(len(pos), gas, 5), timestep, H.KIND_TBI[kind], gas, kind)


@pytest.mark.gpu
@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_device_clamped_chain_against_the_reference(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=11)
    box = 1000.0 if periodic else 0.0
    free = R.run(pos, mass, ptype, vel, hsml0, box=box, timeout=T_SMALL)
    minh = float(np.quantile(free["hsml"][gas], 1.0 / 3))
    timestep = np.full(len(pos), 2, dtype=np.int32)
    out, dens, _ = device_chain_vs_reference(pkg, periodic, pos, mass, ptype, vel, hsml0, entropy_of(len(pos), gas, 11), timestep,
                                             H.KIND_TBI[kind], gas, kind + " clamped", min_gas_hsml=minh, t=T_SMALL)
    clamped = out["hsml"][gas] == minh
    assert 0.25 * len(gas) < clamped.sum() < 0.42 * len(gas) and np.array_equal(dens["hsml"][gas] == minh, clamped)


@pytest.mark.gpu
@need_ref
@pytest.mark.parametrize("kind,periodic", D.CASES)
def test_device_bracket_accept_against_the_reference(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=11)
    box = 1000.0 if periodic else 0.0
    out = R.run(pos, mass, ptype, vel, hsml, box=box, dev=TIGHT_DEV, timeout=T_SMALL)
    assert (np.abs(out["num_ngb"][gas] - DES) > TIGHT_DEV).sum() > 0.1 * len(gas)
    eng = D.make_engine(pkg, periodic, pos, mass, ptype)
    dens = eng.sph_density(vel, hsml, DES, TIGHT_DEV)
    eng.close()
    assert dens["max_rounds"] == out["passes"], (dens["max_rounds"], out["passes"])
    device_density_vs_reference(dens, out, pos, mass, vel, ptype, gas, box, kind + " bracket accept")


@pytest.mark.gpu
@need_ref
def test_device_hmax_set_against_the_reference(pkg):
    pos, mass, ptype, vel, _, timestep, gas, L = H.hydro_set(pkg, "uniform")
    col, big = hmax_columns(pkg)
    tbi = H.KIND_TBI["uniform"]
    out = R.run(pos, mass, ptype, vel, col["hsml"], box=L, columns=col, visc=VISC, timestep=timestep, tbi=tbi, timeout=T_SMALL)
    eng = D.make_engine(pkg, True, pos, mass, ptype)
    res = H.call(eng, vel, col, art_bulk_visc_const=VISC, timestep=timestep, timebase_interval=tbi)
    eng.close()
    device_hydro_vs_reference(res, out, pos, mass, vel, ptype, gas, col, L, "hmax", timestep=timestep, tbi=tbi)


@pytest.mark.gpu
@need_ref
@pytest.mark.parametrize("kind,periodic", H.CASES)
def test_device_active_subset_on_a_refit_tree_against_the_reference(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, kind, n=6000, ngas=4000, seed=12)
    box = 1000.0 if periodic else 0.0
    rng = np.random.default_rng(3)
    active = (rng.uniform(size=len(pos)) < 0.4).astype(np.uint8)
    targets = gas[active[gas] != 0]
    timestep = (rng.choice([0, 1, 2, 4, 8], len(pos)) * 2 ** rng.integers(0, 4, len(pos))).astype(np.int32)
    tbi = H.KIND_TBI[kind]
    A = entropy_of(len(pos), gas, 12)
    eng = D.make_engine(pkg, periodic, pos, mass, ptype, active=active)
    # every gas particle needs SphP columns before a subset can be updated: one full density() on the reference's side
    # (all active) supplies them to both sides; then the positions drift, the device keeps and refits its tree, and the
    # active subset is redone by both
    base = R.run(pos, mass, ptype, vel, hsml0, box=box, entropy=A, timeout=T_SMALL)
    pos2 = pos + 0.02 * (box if periodic else 1.0) / 20 * rng.normal(size=pos.shape)
    if periodic:
        pos2 = np.mod(pos2, box)
    eng.update_particles(pos2, mass, ptype, active=active)
    out = R.run(pos2, mass, ptype, vel, base["hsml"], box=box, active=active, entropy=A, timeout=T_SMALL)
    dens = eng.sph_density(vel, base["hsml"], DES, DEV)
    device_density_vs_reference(dens, out, pos2, mass, vel, ptype, targets, box, kind + " active, refit tree")
    idle = gas[active[gas] == 0]
    assert np.array_equal(dens["hsml"][idle], base["hsml"][idle])
    # hydro on the mixed columns: the subset's new ones, the others' old ones, the same on both sides
    col = {k: base[k].copy() for k in H.COLS}
    for k in H.COLS:
        col[k][targets] = out[k][targets]
    hout = R.run(pos2, mass, ptype, vel, col["hsml"], box=box, columns=col, visc=VISC, timestep=timestep, tbi=tbi, active=active, timeout=T_SMALL)
    hyd = H.call(eng, vel, col, art_bulk_visc_const=VISC, timestep=timestep, timebase_interval=tbi)
    eng.close()
    device_hydro_vs_reference(hyd, hout, pos2, mass, vel, ptype, targets, col, box, kind + " active, refit tree", timestep=timestep, tbi=tbi)
    assert np.all(hyd["hydro_accel"][idle] == 0)


@pytest.mark.gpu
@need_ref
def test_device_large_run_every_row_against_the_reference(pkg):
    """2^LARGE_LOG2 gas particles, periodic, the chain: the reference is a tree code and checks EVERY row, and
    all_row_scales() gives every row its own sum |terms|: compare() of both existing modules on all rows, all quantities
    (dt_entropy included), nothing sampled, nothing left out."""
    n, box = 1 << LARGE_LOG2, 1000.0
    rng = np.random.default_rng(21)
    pos = rng.uniform(0.0, box, (n, 3))
    mass = rng.uniform(0.5, 1.5, n) / n
    vel = rng.normal(0.0, 1.0, (n, 3)) - 0.1 * (pos - 0.5 * box)
    ptype = np.zeros(n, dtype=np.int32)
    h_est = (DES / (D.NORM_COEFF * n / box ** 3)) ** (1.0 / 3)
    A = 10.0 ** rng.uniform(-0.5, 0.5, n)
    timestep = (rng.choice([0, 1, 2, 4, 8], n) * 2 ** rng.integers(0, 4, n)).astype(np.int32)
    tbi = 0.2
    hsml0 = np.full(n, h_est)
    out = R.run(pos, mass, ptype, vel, hsml0, box=box, entropy=A, visc=VISC, timestep=timestep, tbi=tbi, timeout=T_LARGE)
    cfg = pkg.make_config(n_gravs=1, periodic=1, box_size=box, softening=[0.01] * 6, walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.domain_Decomposition()
    eng.force_treebuild()
    dens, col, hyd = device_chain(pkg, eng, vel, hsml0, A, timestep, tbi)
    eng.close()
    print("sph large run 2^%d: reference %.1f s, %d passes; device max_rounds %d" % (LARGE_LOG2, out["seconds"], out["passes"], dens["max_rounds"]))
    assert dens["max_rounds"] == out["passes"]
    p_err = rel(col["pressure"], out["pressure"])
    print("sph large run, all %d rows: pressure %.2e" % (n, p_err))
    assert p_err <= TOL
    rows = np.arange(n)
    sc, log = all_row_scales(pos, mass, vel, {k: out[k] for k in H.COLS}, box, timestep, tbi)
    assert "only_hj" in log and "limiter_active" in log
    ref = {k: out[k] for k in DENS_KEYS}
    ref.update(div_scale=sc["div_scale"], curl_scale=sc["curl_scale"], flagged=np.zeros(n, dtype=bool))
    D.compare(dens, ref, rows, what="device vs reference, all rows of 2^%d" % LARGE_LOG2)
    ref = {"hydro_accel": out["hydro_accel"], "dt_entropy": out["dt_entropy"], "max_signal_vel": out["max_signal_vel"],
           "acc_scale": sc["acc_scale"], "dte_scale": sc["dte_scale"], "flagged": np.zeros(n, dtype=bool)}
    H.compare(hyd, ref, rows, what="device vs reference, all rows of 2^%d" % LARGE_LOG2)


@pytest.mark.gpu
def test_the_reference_executables_travelled_with_the_tree():
    """a GPU machine has no reference tree and cannot rebuild oracle/_ref/: if the executables did not arrive, every
    device-against-the-reference test above skips, and this one says so instead of staying silent"""
    assert R.available(), "oracle/_ref/ref_sph_* are absent on this machine: the device-against-the-reference tests skipped (%s where the reference tree is)" % R.MAKE_TARGET


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_device_against_the_recorded_reference(pkg, name):
    f = fixture(name)
    pos, mass, ptype, vel, gas, box = f["pos"], f["mass"], f["ptype"], f["vel"], f["gas"], float(f["box"])
    n = len(pos)
    minh, tbi = float(f["min_gas_hsml"]), float(f["tbi"])
    out = {k: fixture_full(f, "ref_" + k) for k in DENS_KEYS + ("pressure", "hydro_accel", "dt_entropy", "max_signal_vel")}
    eng = D.make_engine(pkg, bool(box), pos, mass, ptype)
    dens, col, hyd = device_chain(pkg, eng, vel, fixture_full(f, "hsml0"), fixture_full(f, "entropy"), f["timestep"], tbi, min_gas_hsml=minh)
    eng.close()
    assert dens["max_rounds"] == int(f["ref_passes"])
    device_density_vs_reference(dens, out, pos, mass, vel, ptype, gas, box, "fixture " + name)
    assert rel(col["pressure"][gas], out["pressure"][gas]) <= TOL
    ref_col = {k: H.full(n, gas, out[k][gas]) for k in H.COLS}
    device_hydro_vs_reference(hyd, out, pos, mass, vel, ptype, gas, ref_col, box, "fixture " + name, timestep=f["timestep"], tbi=tbi)


@pytest.mark.gpu
@pytest.mark.parametrize("name", FIXTURES)
def test_c_abi_with_interleaved_columns_is_bit_identical(pkg, name):
    """ngravs_sph_density / ngravs_sph_hydro through the C ABI structs with every column a strided view of ONE interleaved
    array (the Python front always passes contiguous columns): bit for bit the contiguous call"""
    import ctypes as C
    f = fixture(name)
    pos, mass, ptype, vel, gas, box = f["pos"], f["mass"], f["ptype"], f["vel"], f["gas"], float(f["box"])
    n = len(pos)
    eng = D.make_engine(pkg, bool(box), pos, mass, ptype)
    hsml0, A = fixture_full(f, "hsml0"), fixture_full(f, "entropy")
    minh, tbi = float(f["min_gas_hsml"]), float(f["tbi"])
    dens, col, hyd = device_chain(pkg, eng, vel, hsml0, A, f["timestep"], tbi, min_gas_hsml=minh)
    L, abi = pkg.lib(), pkg.abi
    # density: one row = [pad, vel x 3, pad, hsml, density, num_ngb, div_vel, curl_vel, dhsml_factor, pad] doubles
    W = 12
    buf = np.full((n, W), -3.25)
    buf[:, 1:4], buf[:, 5] = vel, hsml0
    at = lambda c: buf.ctypes.data + 8 * c   # noqa: E731
    si, so = abi.SphIn(), abi.SphOut()
    si.vel_pred, si.vel_stride, si.hsml, si.hsml_stride = at(1), 8 * W, at(5), 8 * W
    si.des_num_ngb, si.max_num_ngb_deviation, si.min_gas_hsml = DES, DEV, minh
    for c, k in enumerate(abi.SPH_OUT_NAMES):
        setattr(so, k, at(6 + c))
        setattr(so, k + "_stride", 8 * W)
    rounds, ms = C.c_int32(0), C.c_double(0)
    assert L.ngravs_sph_density(eng._h, C.byref(si), C.byref(so), C.byref(rounds), C.byref(ms)) == 0, L.ngravs_last_error(eng._h)
    assert rounds.value == dens["max_rounds"]
    other = np.ones(n, dtype=bool)
    other[gas] = False
    assert np.array_equal(buf[gas, 5], dens["hsml"][gas]) and np.array_equal(buf[other, 5], hsml0[other])
    for c, k in enumerate(abi.SPH_OUT_NAMES):
        assert np.array_equal(buf[gas, 6 + c], dens[k][gas]) and np.all(buf[other, 6 + c] == -3.25), k
    assert np.all(buf[:, [0, 4, 11]] == -3.25) and np.array_equal(buf[:, 1:4], vel)
    # hydro: one row = [vel x 3, hsml, density, pressure, dhsml_factor, div_vel, curl_vel, timestep (int32 in a double's
    # slot), pad, accel x 3, dt_entropy, pad, max_signal_vel] doubles
    W = 17
    buf = np.full((n, W), -3.25)
    buf[:, 0:3] = vel
    for c, k in enumerate(H.COLS):
        buf[:, 3 + c] = np.where(other, 1.0, col[k])
    buf.view(np.int32).reshape(n, 2 * W)[:, 18] = f["timestep"]
    at = lambda c: buf.ctypes.data + 8 * c   # noqa: E731
    hi, ho = abi.HydroIn(), abi.HydroOut()
    hi.vel_pred, hi.vel_pred_stride = at(0), 8 * W
    for c, k in enumerate(H.COLS):
        setattr(hi, k, at(3 + c))
        setattr(hi, k + "_stride", 8 * W)
    hi.timestep, hi.timestep_stride = at(9), 8 * W
    hi.art_bulk_visc_const, hi.timebase_interval, hi.gamma, hi.viscosity_limiter = VISC, tbi, GAMMA, 1
    ho.hydro_accel, ho.hydro_accel_stride = at(11), 8 * W
    ho.dt_entropy, ho.dt_entropy_stride = at(14), 8 * W
    ho.max_signal_vel, ho.max_signal_vel_stride = at(16), 8 * W
    assert L.ngravs_sph_hydro(eng._h, C.byref(hi), C.byref(ho), C.byref(ms)) == 0, L.ngravs_last_error(eng._h)
    eng.close()
    assert np.array_equal(buf[gas, 11:14], hyd["hydro_accel"][gas]) and np.array_equal(buf[gas, 14], hyd["dt_entropy"][gas])
    assert np.array_equal(buf[gas, 16], hyd["max_signal_vel"][gas]) and np.any(hyd["hydro_accel"][gas] != 0)
    assert np.all(buf[other, 11:17] == -3.25) and np.all(buf[:, [10, 15]] == -3.25)
