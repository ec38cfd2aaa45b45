"""SPH density and smoothing lengths (ngravs_sph_density, csrc/kernels_sph.hip) against a numpy restatement of the reference.

The truth is restated here by hand from density.c / ngb.c (line citations below): brute-force O(N^2) pair sums in chunks
(distances of a chunk of targets to ALL gas particles, then the pairs with r2 < h2 exactly as density.c:531), and the iteration
rules of density.c:314-389 applied per particle.  The restatement itself, and the device directly, are held to the reference's
own output in tests/test_sph_reference.py (the reference's SPH path builds for one task: oracle/_ref/).

Tolerance: the device sums differ from numpy's by summation order (and fused multiply-adds) only: TOL = 1e-11 relative, the
project's figure for kernels against the oracle; DivVel / CurlVel are measured against sum|terms| / rho, not against the result
(the terms cancel).  A particle whose NumNgb in some round lies within 1e-9 relative of a decision bound (DesNumNgb +-
MaxNumNgbDeviation, DesNumNgb +- DesNumNgb / 2) can legitimately take the other branch: the restatement flags those from its own
numbers; they are left out of the comparison and must stay below 0.1 % of the targets.  Flagged on the CPU for the seeded inputs
below: uniform periodic 0 of 12 000, Plummer 0 of 12 000, the 512-target sample of the 2^20 run 0.

Starting hsml of the parity cases: h_est / 3 for the targets of even rank and 3 h_est for the odd ones, h_est the length that
holds DesNumNgb particles at the local mean gas density (the box's for the uniform box, the Plummer profile's for the sphere: one
constant cannot be off by a factor of three everywhere in a sphere whose density spans decades).
"""
import numpy as np
import pytest

KC1, KC2, KC3, KC4, KC5, KC6 = 2.546479089470, 15.278874536822, 45.836623610466, 30.557749073644, 5.092958178941, -15.278874536822
NORM_COEFF = 4.188790204786   # allvars.h:109-115, NUMDIMS = 3
MAXITER = 150                 # allvars.h:97
TOL = 1e-11
DES, DEV = 50.0, 1.0


def spline(u, hinv3, hinv4):
    """density.c:541-550"""
    lo = u < 0.5
    wk = np.where(lo, hinv3 * (KC1 + KC2 * (u - 1) * u * u), hinv3 * KC5 * (1.0 - u) * (1.0 - u) * (1.0 - u))
    dwk = np.where(lo, hinv4 * u * (KC3 * u - KC4), hinv4 * KC6 * (1.0 - u) * (1.0 - u))
    return wk, dwk


def _nearest(d, box):
    """density.c:517-530"""
    if box:
        d = np.where(d > 0.5 * box, d - box, d)
        d = np.where(d < -0.5 * box, d + box, d)
    return d


def _r2_matrix(X, G, box):
    r2 = np.zeros((len(X), len(G)))
    for k in range(3):
        d = _nearest(X[:, k, None] - G[None, :, k], box)
        r2 += d * d
    return r2


def _evaluate(X, V, h, r2, G, GM, GV, box):
    """density_evaluate (density.c:467-599) for targets X (velocities V, trial lengths h) over the gas particles G; r2 = their
    distance matrix.  Returns rho, weighted_numngb, dhsmlrho, divv, rot[3] and sum|terms| of divv and of rot."""
    n = len(X)
    ii, jj = np.nonzero(r2 < (h * h)[:, None])          # r2 < h2, :531
    hinv = 1.0 / h
    hinv3 = hinv * hinv * hinv
    hinv4 = hinv3 * hinv
    r = np.sqrt(r2[ii, jj])
    u = r * hinv[ii]
    wk, dwk = spline(u, hinv3[ii], hinv4[ii])
    m = GM[jj]
    s = lambda w: np.bincount(ii, weights=w, minlength=n)   # noqa: E731
    rho = s(m * wk)
    wnn = s(NORM_COEFF * wk / hinv3[ii])                 # :556
    dhr = s(-m * (3 * hinv[ii] * wk + u * dwk))          # :558
    pos = r > 0                                          # :560
    ii, jj, fac = ii[pos], jj[pos], (m * dwk)[pos] / r[pos]
    d = _nearest(X[ii] - G[jj], box)
    dv = V[ii] - GV[jj]
    tdiv = fac * (d[:, 0] * dv[:, 0] + d[:, 1] * dv[:, 1] + d[:, 2] * dv[:, 2])
    t0 = fac * (d[:, 2] * dv[:, 1] - d[:, 1] * dv[:, 2])
    t1 = fac * (d[:, 0] * dv[:, 2] - d[:, 2] * dv[:, 0])
    t2 = fac * (d[:, 1] * dv[:, 0] - d[:, 0] * dv[:, 1])
    divv = -s(tdiv)
    rot = np.stack([s(t0), s(t1), s(t2)], axis=1)
    return rho, wnn, dhr, divv, rot, s(np.abs(tdiv)), s(np.abs(t0)) + s(np.abs(t1)) + s(np.abs(t2))


def restate(pos, mass, vel, ptype, targets, h0, des, dev, minh=0.0, box=0.0, one_round=False, chunk_pairs=6e6):
    """density() (density.c:56-441) for the rows `targets`, iterated per particle.  Returns a dict of arrays over `targets`
    (hsml, density, num_ngb, div_vel, curl_vel, dhsml_factor, div_scale, curl_scale, rounds, flagged) and the set of rules
    that fired.  one_round: a single evaluation at h0 (no iteration)."""
    gas = np.nonzero(ptype == 0)[0]                      # ngb.c:221
    G, GM, GV = pos[gas], mass[gas], vel[gas]
    nt = len(targets)
    out = {k: np.zeros(nt) for k in ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor", "div_scale", "curl_scale")}
    out["rounds"] = np.zeros(nt, dtype=np.int64)
    out["flagged"] = np.zeros(nt, dtype=bool)
    log = set()
    step = max(1, int(chunk_pairs // len(gas)))
    for c0 in range(0, nt, step):
        sl = slice(c0, min(nt, c0 + step))
        rows = targets[sl]
        X, V = pos[rows], vel[rows]
        R2 = _r2_matrix(X, G, box)
        n = len(rows)
        h = np.array(h0[sl], dtype=np.float64)
        left, right = np.zeros(n), np.zeros(n)           # :95-99
        live = np.ones(n, dtype=bool)
        it = 0
        while live.any():
            a = np.nonzero(live)[0]
            rho, nn, dhr, divv, rot, sdiv, srot = _evaluate(X[a], V[a], h[a], R2[a], G, GM, GV, box)
            ha, la, ra = h[a], left[a], right[a]
            with np.errstate(divide="ignore"):             # a target alone inside h: 1 / 0 = inf, as in the reference (unused then)
                dhf = 1 / (1 + ha * dhr / (3 * rho))      # :296-297
            for bound in (des - dev, des + dev, 0.5 * des, 1.5 * des):
                out["flagged"][c0 + a] |= np.abs(nn - bound) <= 1e-9 * bound
            redo = (nn < (des - dev)) | ((nn > (des + dev)) & (ha > 1.01 * minh))          # :314-316
            ok_bracket = redo & (la > 0) & (ra > 0) & ((ra - la) < 1.0e-3 * la)          # :321-328
            if ok_bracket.any():
                log.add("accept_bracket")
            if (~redo & (nn > des + dev)).any():
                log.add("accept_at_min")
            redo &= ~ok_bracket
            if one_round:
                redo[:] = False
            done = a[~redo]
            g = c0 + done
            out["hsml"][g], out["density"][g], out["num_ngb"][g] = ha[~redo], rho[~redo], nn[~redo]
            out["div_vel"][g] = (divv / rho)[~redo]                                          # :303
            out["curl_vel"][g] = (np.sqrt(rot[:, 0] ** 2 + rot[:, 1] ** 2 + rot[:, 2] ** 2) / rho)[~redo]   # :299-301
            out["dhsml_factor"][g] = dhf[~redo]
            out["div_scale"][g], out["curl_scale"][g] = (sdiv / rho)[~redo], (srot / rho)[~redo]
            out["rounds"][g] = it + 1
            live[done] = False
            # the rest: bracket and next trial (:330-386)
            few = nn < (des - dev)
            la = np.where(redo & few, np.maximum(ha, la), la)                                # :330-331
            many = redo & ~few
            ra = np.where(many & ((ra == 0) | (ha < ra)), ha, ra)                            # :332-341
            both = redo & (ra > 0) & (la > 0)
            newton = np.abs(nn - des) < 0.5 * des                                            # :362, :374
            fac = 1 - (nn - des) / (3 * np.maximum(nn, 1e-300)) * dhf
            up, down = redo & (ra == 0) & (la > 0), redo & (ra > 0) & (la == 0)
            hn = np.where(both, np.power(0.5 * (np.power(la, 3) + np.power(ra, 3)), 1.0 / 3), ha)   # :353-354
            hn = np.where(up, np.where(newton, ha * fac, ha * 1.26), hn)                    # :360-370
            hn = np.where(down, np.where(newton, ha * fac, ha / 1.26), hn)                  # :372-382
            for name, m in (("left", redo & few), ("right", many), ("bisect", both), ("newton", (up | down) & newton),
                            ("grow_1.26", up & ~newton), ("shrink_1.26", down & ~newton), ("clamp", redo & (hn < minh))):
                if m.any():
                    log.add(name)
            hn = np.where(redo & (hn < minh), minh, hn)                                      # :385-386
            h[a], left[a], right[a] = hn, la, ra
            it += 1
            assert it <= MAXITER, "the restatement itself did not converge (endrun(1155), density.c:416)"
    return out, log


def compare(res, ref, rows, tol=TOL, what=""):
    """device result (arrays over all rows) against the restatement (arrays over `rows`); flagged targets are left out"""
    keep = ~ref["flagged"]
    assert ref["flagged"].sum() <= 1e-3 * len(rows), "too many borderline targets: %d" % ref["flagged"].sum()
    worst = {}
    for k in ("hsml", "density", "num_ngb", "dhsml_factor"):
        worst[k] = np.max(np.abs(res[k][rows] - ref[k])[keep] / np.abs(ref[k])[keep])
    worst["div_vel"] = np.max((np.abs(res["div_vel"][rows] - ref["div_vel"]) / ref["div_scale"])[keep])
    worst["curl_vel"] = np.max((np.abs(res["curl_vel"][rows] - ref["curl_vel"]) / ref["curl_scale"])[keep])
    print("sph parity %s: %s (flagged %d of %d)" % (what, ", ".join("%s %.2e" % kv for kv in worst.items()), ref["flagged"].sum(), len(rows)))
    for k, v in worst.items():
        assert v <= tol, (what, k, v)
    return worst


# ---- inputs -------------------------------------------------------------------------------------------------------------
def gas_mix(pkg, kind, n=20000, ngas=12000, seed=5, box=1000.0):
    """N particles, `ngas` of type 0 mixed with types 1 and 2 (N_GRAVS = 2), random velocities; starting hsml off by x3"""
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        pos, mass, _ = pkg.ic.uniform_box(n, box=box, n_gravs=2, seed=seed)
    else:
        pos, mass, _ = pkg.ic.plummer_sphere(n, seed=seed)
    ptype = np.where(rng.permutation(n) < ngas, 0, 1 + (np.arange(n) % 2)).astype(np.int32)
    mass = mass * rng.uniform(0.5, 1.5, n)
    vel = rng.normal(0.0, 1.0, (n, 3))
    if kind == "uniform":
        ngas_density = np.full(n, ngas / box ** 3)
    else:
        ngas_density = ngas * 3 / (4 * np.pi) * (1 + np.sum(pos * pos, axis=1)) ** -2.5
    h_est = (DES / (NORM_COEFF * ngas_density)) ** (1.0 / 3)
    gas = np.nonzero(ptype == 0)[0]
    hsml = np.zeros(n)
    hsml[gas] = np.where(np.arange(len(gas)) % 2 == 0, h_est[gas] / 3, h_est[gas] * 3)
    return pos, mass, ptype, vel, hsml, gas


def make_engine(pkg, periodic, pos, mass, ptype, box=1000.0, active=None, **kw):
    cfg = pkg.make_config(n_gravs=2, periodic=int(periodic), box_size=box if periodic else 0.0, softening=[0.01] * 6,
                          type_to_grav=[0, 0, 1, 0, 0, 0], walk_mode=pkg.WALK_GROUP, **kw)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype, active=active)
    eng.domain_Decomposition()
    eng.force_treebuild()
    return eng


CASES = [("uniform", True), ("plummer", False)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_sph_kernel_is_exported_and_is_the_reference_spline(pkg, have_lib):
    assert "ngravs_sph_density" in pkg.EXPORTS and "ngravs_sph_kernel" in pkg.EXPORTS
    assert hasattr(have_lib, "ngravs_sph_density") and hasattr(have_lib, "ngravs_sph_kernel")
    hdr = open(pkg.__file__.replace("gadget-2.0.7-ngravs_amd/__init__.py", "include/ngravs_hip.h")).read()
    assert "int ngravs_sph_density(" in hdr and "int ngravs_sph_kernel(" in hdr
    for h in (0.37, 1.0, 812.5):
        hinv3, hinv4 = (1 / h) ** 3, (1 / h) ** 4
        r = np.linspace(0.0, 1.2 * h, 10000)
        wk, dwk = pkg.sph_kernel(h, r)
        inside = r * r < h * h
        wk0, dwk0 = spline(r / h, hinv3, hinv4)
        assert np.max(np.abs(wk - wk0)[inside]) <= 1e-14 * hinv3 and np.max(np.abs(dwk - dwk0)[inside]) <= 1e-14 * hinv4
        assert np.all(wk[~inside] == 0) and np.all(dwk[~inside] == 0) and (~inside).sum() > 1000
        rr = np.linspace(0.0, h, 100001)
        w = pkg.sph_kernel(h, rr)[0] * rr * rr
        integral = 4 * np.pi * np.sum(0.5 * (w[1:] + w[:-1]) * np.diff(rr))
        assert abs(integral - 1) < 1e-8, integral


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", CASES)
def test_parity_with_the_restatement(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, kind)
    box = 1000.0 if periodic else 0.0
    ref, log = restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    for rule in ("left", "right", "bisect", "newton", "grow_1.26", "shrink_1.26"):
        assert rule in log, (rule, log)
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    res = eng.sph_density(vel, hsml, DES, DEV)
    assert res["max_rounds"] == ref["rounds"].max() or ref["flagged"].any()
    compare(res, ref, gas, what=kind)
    # independent of the restatement's iteration: one brute-force evaluation at the returned lengths
    chk, _ = restate(pos, mass, vel, ptype, gas, res["hsml"][gas], DES, DEV, box=box, one_round=True)
    nn = chk["num_ngb"]
    band = (nn >= (DES - DEV) * (1 - 1e-9)) & (nn <= (DES + DEV) * (1 + 1e-9))
    assert band.all(), (nn.min(), nn.max())
    assert np.max(np.abs(res["density"][gas] - chk["density"]) / chk["density"]) <= TOL
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", CASES)
def test_min_gas_hsml_clamps(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, kind, n=6000, ngas=4000, seed=11)
    box = 1000.0 if periodic else 0.0
    free, _ = restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    minh = float(np.quantile(free["hsml"], 1.0 / 3))          # a third of the targets want less than this
    ref, log = restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, minh=minh, box=box)
    assert "clamp" in log and "accept_at_min" in log
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    res = eng.sph_density(vel, hsml, DES, DEV, min_gas_hsml=minh)
    compare(res, ref, gas, what=kind + " clamped")
    clamped = res["hsml"][gas] == minh
    assert 0.25 * len(gas) < clamped.sum() < 0.42 * len(gas)
    assert np.all(res["num_ngb"][gas][clamped] > DES - DEV) and np.any(res["num_ngb"][gas][clamped] > DES + DEV)
    assert np.all(res["hsml"][gas] >= minh)
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", CASES)
def test_only_active_gas_rows_are_written_and_a_refit_tree_serves(pkg, kind, periodic):
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, kind, n=6000, ngas=4000, seed=12)
    box = 1000.0 if periodic else 0.0
    rng = np.random.default_rng(3)
    active = (rng.uniform(size=len(pos)) < 0.4).astype(np.uint8)
    targets = gas[active[gas] != 0]
    hsml = np.where(np.isin(np.arange(len(pos)), targets), hsml, -7.0)   # rows that are no targets are not read
    eng = make_engine(pkg, periodic, pos, mass, ptype, active=active)
    sentinel = {k: np.full(len(pos), -3.25) for k in pkg.abi.SPH_OUT_NAMES}
    res = eng.sph_density(vel, hsml, DES, DEV, out=sentinel)
    other = np.ones(len(pos), dtype=bool)
    other[targets] = False
    for k in pkg.abi.SPH_OUT_NAMES:
        assert np.all(res[k][other] == -3.25) and np.all(res[k][targets] != -3.25), k
    assert np.all(res["hsml"][other] == -7.0) and np.all(res["hsml"][targets] > 0)
    ref, _ = restate(pos, mass, vel, ptype, targets, hsml[targets], DES, DEV, box=box)
    compare(res, ref, targets, what=kind + " active")
    # kept tree, drifted positions: refit, then the same result as a fresh build
    pos2 = pos + 0.02 * (box if periodic else 1.0) / 20 * rng.normal(size=pos.shape)
    if periodic:
        pos2 = np.mod(pos2, box)
    eng.update_particles(pos2, mass, ptype, active=active)
    kept = eng.sph_density(vel, hsml, DES, DEV)
    fresh_eng = make_engine(pkg, periodic, pos2, mass, ptype, active=active)
    fresh = fresh_eng.sph_density(vel, hsml, DES, DEV)
    ref2, _ = restate(pos2, mass, vel, ptype, targets, hsml[targets], DES, DEV, box=box)
    compare(kept, ref2, targets, what=kind + " refit")
    compare(fresh, ref2, targets, what=kind + " fresh")
    eng.close()
    fresh_eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("periodic", [True, False])
def test_coincident_pair_and_a_sphere_across_three_faces(pkg, periodic):
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, "uniform", n=6000, ngas=4000, seed=13)
    box = 1000.0 if periodic else 0.0
    pos[gas[1]] = pos[gas[0]]                         # r = 0: counted in rho, skipped in div / curl (density.c:560)
    pos[gas[2]] = [0.4, 999.7, 0.2]                   # the sphere of DesNumNgb crosses three faces of the periodic box
    ref, _ = restate(pos, mass, vel, ptype, gas, hsml[gas], DES, DEV, box=box)
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    res = eng.sph_density(vel, hsml, DES, DEV)
    compare(res, ref, gas, what="coincident, periodic %d" % periodic)
    assert np.isfinite(res["div_vel"][gas[:3]]).all() and np.isfinite(res["curl_vel"][gas[:3]]).all()
    if periodic:
        h = res["hsml"][gas[2]]
        assert h > 0.4 and h > 1000 - 999.7 and h > 0.2
    eng.close()


@pytest.mark.gpu
def test_refusals_and_gravity_is_not_disturbed(pkg):
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, "uniform", n=6000, ngas=4000, seed=14)
    cfg_kw = dict(n_gravs=2, periodic=1, box_size=1000.0, softening=[0.01] * 6, type_to_grav=[0, 0, 1, 0, 0, 0], walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(pkg.make_config(**cfg_kw))
    eng.set_particles(pos, mass, ptype)
    with pytest.raises(pkg.NgravsError, match="status -4.*built tree"):      # no tree
        eng.sph_density(vel, hsml, DES, DEV)
    eng.domain_Decomposition()
    eng.force_treebuild()
    bad = hsml.copy()
    bad[gas[7]] = 0.0
    with pytest.raises(pkg.NgravsError, match="status -1.*hsml"):
        eng.sph_density(vel, bad, DES, DEV)
    with pytest.raises(pkg.NgravsError, match="status -1.*des_num_ngb"):
        eng.sph_density(vel, hsml, 0.0, DEV)
    two = pkg.Engine(pkg.make_config(world_size=2, rank=0, **cfg_kw))
    two.set_particles(pos, mass, ptype)
    with pytest.raises(pkg.NgravsError, match="status -4.*single task only"):
        two.sph_density(vel, hsml, DES, DEV)
    two.close()
    # no type-0 target: success, nothing written
    none = make_engine(pkg, True, pos, mass, np.where(ptype == 0, 1, ptype).astype(np.int32))
    r0 = none.sph_density(vel, hsml, DES, DEV)
    assert r0["max_rounds"] == 0 and np.all(r0["density"] == 0) and np.array_equal(r0["hsml"], hsml)
    none.close()
    # the tree is not disturbed: gravity after a density call is bit-identical to gravity without one
    eng.sph_density(vel, hsml, DES, DEV)
    eng.gravity_tree()
    acc1, _, cost1 = eng.get_accel()
    plain = make_engine(pkg, True, pos, mass, ptype)
    plain.gravity_tree()
    acc0, _, cost0 = plain.get_accel()
    assert np.array_equal(acc0, acc1) and np.array_equal(cost0, cost1)
    eng.close()
    plain.close()


@pytest.mark.gpu
def test_a_million_gas_particles_against_a_brute_force_sample(pkg):
    n, box = 1 << 20, 1000.0
    rng = np.random.default_rng(21)
    pos = rng.uniform(0.0, box, (n, 3))
    mass = rng.uniform(0.5, 1.5, n) / n
    vel = rng.normal(0.0, 1.0, (n, 3))
    ptype = np.zeros(n, dtype=np.int32)
    h_est = (DES / (NORM_COEFF * n / box ** 3)) ** (1.0 / 3)
    hsml = np.where(np.arange(n) % 2 == 0, h_est / 3, h_est * 3)
    cfg = pkg.make_config(n_gravs=1, periodic=1, box_size=box, softening=[0.01] * 6, walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.domain_Decomposition()
    eng.force_treebuild()
    res = eng.sph_density(vel, hsml, DES, DEV)
    sample = np.sort(rng.choice(n, 512, replace=False))
    ref, _ = restate(pos, mass, vel, ptype, sample, hsml[sample], DES, DEV, box=box)
    compare(res, ref, sample, what="2^20 sample")
    print("sph 2^20: max rounds %d, %.2f ms" % (res["max_rounds"], res["kernel_ms"]))
    eng.close()


@pytest.mark.gpu
def test_device_tensors_give_the_host_result(pkg):
    """zero-copy hand-over: torch device tensors in, device tensors out, bit for bit what the host arrays give"""
    import torch
    pos, mass, ptype, vel, hsml, gas = gas_mix(pkg, "uniform", n=6000, ngas=4000, seed=15)
    eng = make_engine(pkg, True, pos, mass, ptype)
    host = eng.sph_density(vel, hsml, DES, DEV)
    dev = eng.sph_density(torch.from_numpy(vel).cuda(), torch.from_numpy(hsml).cuda(), DES, DEV)
    assert dev["max_rounds"] == host["max_rounds"]
    for k in ("hsml",) + tuple(pkg.abi.SPH_OUT_NAMES):
        assert dev[k].is_cuda and np.array_equal(dev[k].cpu().numpy(), host[k]), k
    eng.close()
