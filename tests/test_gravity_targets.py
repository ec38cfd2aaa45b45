"""Gravity at targets that are not an engine's own particles: ngravs_gravity_tree_targets (the strict walk for records handed in:
the reference's force_treeevaluate(j, 1) / _shortrange(j, 1) / _lattice_correction(j, 1), gravtree.c:133-285) and
ngravs_pm_targets (GravPM of the last PM step's mesh at their places).

Tolerances:
  * own particles handed over as foreign targets: np.array_equal with the own strict walk (the walk of a lane does not depend on
    its wave-mates, the body is the same code);
  * against the oracle's walk and the oracle's direct sums: 1e-10 of the largest acceleration, TOL of test_gpu_parity.py
    (summation order / exp rounding only), identical interaction counts;
  * the lattice-correction walk uses every node of at most 0.2 BoxSize that does not straddle the half-box seam as a monopole
    WHATEVER the opening criterion says (forcetree.c:2203-2243), so "everything opened" is not the direct sum there: the kernel
    is held to the oracle's two walks (1e-9, as in test_lattice.py) on a uniform box, and to direct_lattice (1e-4 max, 2e-5
    median, its tolerance in test_lattice.py) on a clump, where the monopoles stand for their particles;
  * mesh force: 1e-10 of max |GravPM| against tests/pm_reference.py, TOL of test_gpu_pm_mesh.py.
"""
import ctypes as C

import numpy as np
import pytest

import pm_reference
from conftest import rel_err

TOL = 1e-10
COUNTS = (1, 63, 65, 1037)      # probes: one lane, a partial wave, a wave and a lane, several blocks and a partial wave


def _rms(e):
    return float(np.sqrt(np.mean(e ** 2)))


def _maxerr(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_null_context_is_refused_without_a_gpu(pkg, have_lib):
    assert C.sizeof(pkg.abi.GravTargets) == 72
    tg = pkg.abi.GravTargets()
    out = np.full(3, -3.25)
    nint = np.full(1, -3, dtype=np.int32)
    assert have_lib.ngravs_gravity_tree_targets(None, C.byref(tg), 1, out.ctypes.data, nint.ctypes.data, None) == -1
    assert have_lib.ngravs_pm_targets(None, C.byref(tg), 1, out.ctypes.data) == -1
    assert np.all(out == -3.25) and nint[0] == -3


def test_engine_argument_checks_need_no_device(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)        # no context: the checks come before anything that needs one
    eng._h = C.c_void_p()
    ok_pos, ok_typ = np.zeros((5, 3)), np.zeros(5, dtype=np.int32)
    bad = [(np.zeros((5, 2)), ok_typ), (np.zeros(5), ok_typ), (np.zeros((5, 3), dtype=np.int64), ok_typ), (np.zeros((5, 3, 1)), ok_typ),
           (ok_pos, np.zeros(5)), (ok_pos, np.zeros(4, dtype=np.int32)), (ok_pos, np.zeros((5, 1), dtype=np.int32))]
    for pos, typ in bad:
        with pytest.raises(ValueError):
            eng.gravity_tree_targets(pos, typ)
        with pytest.raises(ValueError):
            eng.pm_targets(pos, typ)


# ---- GPU -----------------------------------------------------------------------------------------------------------------------
def _newton(t, s, r2, r, N):
    return s / r2


def _plummer(t, s, h, r, N):
    hi = 1.0 / h
    u = r * hi
    if u < 0.5:
        return s * hi ** 3 * (10.666666666667 + u * u * (32.0 * u - 38.4))
    return s * hi ** 3 * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u ** 3 - 0.066666666667 / u ** 3)


def _case(pkg, name):
    """(cfg, pos, mass, typ, user_fns) of the configurations of the own-positions test"""
    fns = None
    if name in ("plummer", "user"):
        n = 12000 if name == "plummer" else 8000
        pos, mass, typ = pkg.ic.plummer_sphere(n, seed=3)
        kw = dict(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6, walk_mode=pkg.WALK_STRICT)
        if name == "user":       # the set-up of tests/test_user_laws.py: the model's own copies of Newton's law and the Plummer spline
            fns = [(pkg.abi.USER_ACCEL, _newton), (pkg.abi.USER_SPLINE, _plummer)]
            kw["wiring"] = {"accel": [[pkg.abi.LAW_USER0]], "spline": [[pkg.abi.SPLINE_USER0 + 1]]}
        return pkg.make_config(**kw), pos, mass, typ, fns
    ng, pmgrid, n, wiring, L = {"treepm_c4": (2, 32, 20000, "c4", 1e4), "lattice": (1, 0, 6000, "newton", 100.0),
                                "treepm_ng3": (3, 16, 9000, "c4", 1e4)}[name]
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=11)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_STRICT)
    return cfg, pos, mass, typ, fns


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["plummer", "treepm_c4", "lattice", "treepm_ng3", "user"])
def test_own_positions_reproduce_the_own_strict_walk(pkg, O, name):
    """the engine's own particles, shuffled, as foreign targets with their type, OldAcc and mass: GravAccel and GravCost of the
    WALK_STRICT run, bit for bit, under the Barnes-Hut and under the relative criterion; all n and a subset of 65"""
    cfg, pos, mass, typ, fns = _case(pkg, name)
    n = len(pos)
    eng = pkg.Engine(cfg, user_fns=fns)
    eng.set_particles(pos, mass, typ)
    perm = np.random.default_rng(5).permutation(n)
    col = np.zeros(n)
    for crit in ("barnes-hut", "relative"):
        if crit == "relative":
            eng.set_opening(0.0, 0.005)
            eng.set_old_acc(col)
        eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
        acc, old, cost = eng.get_accel()
        for sel in (perm, perm[:65]):
            a, ni = eng.gravity_tree_targets(pos[sel], typ[sel], old_acc=col[sel], mass=mass[sel], want_nint=True)
            assert np.array_equal(a, acc[sel]), (name, crit, len(sel), np.abs(a - acc[sel]).max())
            assert np.array_equal(ni, cost[sel]), (name, crit, len(sel))
        col = old                                  # OldAcc of the Barnes-Hut pass: the relative pass walks with it
    if name == "plummer":
        # another OldAcc column than the engine's own: the oracle's walk with that column
        rng = np.random.default_rng(6)
        col2 = col * rng.uniform(0.3, 3.0, n)
        idx = np.sort(rng.choice(n, 1037, replace=False)).astype(np.int32)
        a, ni = eng.gravity_tree_targets(pos[idx], typ[idx], old_acc=col2[idx], mass=mass[idx], want_nint=True)
        T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
        a_o, n_o = T.walk(old_acc=col2, idx=idx)
        a_o, _ = O.finish(cfg, a_o)
        print("foreign OldAcc column vs oracle walk: max err %.2e, %d of %d counts differ" % (_maxerr(a, a_o), int(np.sum(ni != n_o)), len(idx)))
        assert _maxerr(a, a_o) < TOL
        assert np.array_equal(ni, n_o)
    eng.close()


def _probe_types(k):
    return (np.arange(k) % 6).astype(np.int32)


def _prefixes_agree(call, probes, ptype, full):
    """1, 63 and 65 probes give the first rows of the result for all 1037: partial waves, and the scatter back"""
    for k in COUNTS[:-1]:
        got = call(probes[:k], ptype[:k])
        for g, f in zip(got, full):
            assert np.array_equal(g, f[:k]), k


@pytest.mark.gpu
def test_opening_everything_is_the_direct_sum_tree_only(pkg, O):
    """err_tol_theta = 0 and old_acc = 0: the relative criterion opens every node with mass.  Probes of every type inside the set, on
    particles, and up to three domain lengths outside the cube, against the oracle's direct sum with the probes appended as
    zero-mass rows (1e-10 per target, the tolerance O.direct gets in test_gpu_parity.py); every source is an interaction"""
    n, k = 3000, COUNTS[-1]
    pos, mass, _ = pkg.ic.plummer_sphere(n, seed=21)
    typ = (1 + np.arange(n) % 5).astype(np.int32)
    cfg = pkg.make_config(n_gravs=2, G=43007.1, theta=0.0, softening=[0.01, 0.02, 0.015, 0.03, 0.01, 0.025],
                          type_to_grav=pkg.ic.default_type_to_grav(2), wiring="newton", walk_mode=pkg.WALK_STRICT)
    rng = np.random.default_rng(22)
    dom = O.domain_extent(pos)
    probes = pos[rng.choice(n, k)] + rng.normal(0, 0.05, (k, 3))                    # inside the set
    probes[400:600] = pos[rng.choice(n, 200, replace=False)]                        # on particles
    out = rng.normal(0, 1, (k - 600, 3))
    probes[600:] = dom[3:6] + out / np.linalg.norm(out, axis=1)[:, None] * dom[6] * rng.uniform(0.5, 3.0, (k - 600, 1))   # outside the cube
    ptype = _probe_types(k)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.force_treebuild()
    call = lambda p, t: eng.gravity_tree_targets(p, t, want_nint=True)   # noqa: E731
    a, ni = call(probes, ptype)
    want = O.direct(cfg, np.concatenate([pos, probes]), np.concatenate([mass, np.zeros(k)]), np.concatenate([typ, ptype]),
                    n + np.arange(k, dtype=np.int32))            # (x G, as the library delivers it)
    e = rel_err(a, want)
    print("everything opened, tree-only: max rel err %.2e (inside %.2e, on particles %.2e, outside %.2e)" %
          (e.max(), e[:400].max(), e[400:600].max(), e[600:].max()))
    assert e.max() < TOL
    assert np.all(ni == n)
    _prefixes_agree(call, probes, ptype, (a, ni))
    eng.close()


@pytest.mark.gpu
def test_opening_everything_is_the_direct_sum_treepm(pkg, O):
    """The short-range walk prunes NODES by a box test (forcetree.c:1828-1862) and particles by the end of the table, so with
    everything opened its sources are a set between the spheres of RCUT Asmth and 6 Asmth, not a sphere.  Here the sources are a
    clump of diameter 0.1 BoxSize < RCUT Asmth that wraps around the faces x = 0 and z = BoxSize, and every probe is either within
    0.12 BoxSize of all of them (inside the clump, on particles, on the two faces: coordinates exactly 0 and exactly BoxSize) or
    farther than 6 Asmth from all of them (on the faces y = 0 and y = BoxSize): then the walk IS oracle_py.direct_shortrange over
    the table's reach, with n interactions, or exactly nothing."""
    n, k, L, N = 4000, COUNTS[-1], 1.0, 32
    rng = np.random.default_rng(31)
    centre = np.array([0.02, 0.5, 0.98])

    def ball(m, radius):
        v = rng.normal(0, 1, (m, 3))
        return centre + v / np.linalg.norm(v, axis=1)[:, None] * radius * rng.uniform(0, 1, (m, 1)) ** (1 / 3)
    pos = np.mod(ball(n, 0.05), L)
    mass = rng.uniform(0.5, 1.5, n) / n
    typ = (1 + np.arange(n) % 2).astype(np.int32)
    eps = 0.002
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=N, box_size=L, G=43007.1, theta=0.0, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4", walk_mode=pkg.WALK_STRICT)
    asmth = 1.25 * L / N
    assert 0.12 * L < 4.5 * asmth and 6 * asmth < 0.3 * L
    probes = np.mod(ball(k, 0.07), L)
    probes[600:800] = pos[rng.choice(n, 200, replace=False)]
    probes[800:870, 0] = 0.0                       # on the face x = 0, inside the clump
    probes[870:937, 2] = L                         # on the face z = BoxSize
    probes[937:] = rng.uniform(0, L, (k - 937, 3))
    probes[937:, 1] = np.where(np.arange(k - 937) % 2 == 0, 0.0, L)      # far from every source
    ptype = _probe_types(k)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.force_treebuild()
    call = lambda p, t: eng.gravity_tree_targets(p, t, want_nint=True)   # noqa: E731
    a, ni = call(probes, ptype)
    tab, _ = O.shortrange_table(cfg)
    a_o, _ = O.direct_shortrange(cfg, np.concatenate([pos, probes]), np.concatenate([mass, np.zeros(k)]), np.concatenate([typ, ptype]),
                                 n + np.arange(k, dtype=np.int32), tab, 6.0 * asmth)
    err = _maxerr(a[:937], cfg.G * a_o[:937])
    print("everything opened, TreePM: max err %.2e of the largest acceleration" % err)
    assert err < TOL
    assert np.all(ni[:937] == n)
    assert np.all(a[937:] == 0) and np.all(ni[937:] == 0) and np.all(a_o[937:] == 0)
    _prefixes_agree(call, probes, ptype, (a, ni))
    eng.close()


_LATTICE = {}


def _lattice_case(pkg, O):
    """periodic tree-only, err_tol_theta = 0 and old_acc = 0: sources, probes of every type (anywhere, on particles with their
    types, on the faces: coordinates exactly 0 and exactly BoxSize), the engine's answer and the oracle's lattice tables -- once"""
    if not _LATTICE:
        n, k, L = 3000, COUNTS[-1], 100.0
        pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=1, seed=41)
        pos[0], pos[1] = 0.0, L                          # the domain cube is that of [0, BoxSize]^3 with or without the probes
        eps = L / (40 * n ** (1 / 3))
        cfg = pkg.make_config(n_gravs=1, periodic=1, pmgrid=0, box_size=L, G=1.0, theta=0.0, softening=[eps, 2 * eps, eps, 1.5 * eps, eps, eps],
                              wiring="newton", walk_mode=pkg.WALK_STRICT)   # (one Ewald table: the oracle builds it on the CPU)
        rng = np.random.default_rng(42)
        probes, ptype = rng.uniform(0, L, (k, 3)), _probe_types(k)
        on = rng.choice(np.arange(2, n), 200, replace=False).astype(np.int32)
        probes[400:600], ptype[400:600] = pos[on], typ[on]
        for j in range(3):
            probes[600 + 60 * j: 630 + 60 * j, j] = 0.0
            probes[630 + 60 * j: 660 + 60 * j, j] = L
        probes[780, :2] = 0.0
        probes[781, 1:] = L
        eng = pkg.Engine(cfg)
        eng.set_particles(pos, mass, typ)
        eng.domain_Decomposition()
        eng.force_treebuild()
        call = lambda p, t: eng.gravity_tree_targets(p, t, want_nint=True)   # noqa: E731
        a, ni = call(probes, ptype)
        _prefixes_agree(call, probes, ptype, (a, ni))
        eng.close()
        _LATTICE.update(cfg=cfg, pos=pos, mass=mass, typ=typ, probes=probes, ptype=ptype, on=on, a=a, ni=ni, lat=O.lattice_tables(cfg))
    return _LATTICE


@pytest.mark.gpu
def test_opening_everything_periodic_tree_only_is_the_references_two_walks(pkg, O):
    """The force walk opens everything and is the nearest-image direct sum.  The lattice-correction walk does NOT become a direct sum:
    a node the criterion wants opened is still used as a monopole when it is at most 0.2 BoxSize wide and does not straddle the
    half-box seam (forcetree.c:2203-2243).  Truth is therefore the oracle's two walks themselves: for probes on particles, those
    particles' own walks (identical counts); for the others, the walks of a tree over particles and probes, the probes at zero
    mass (same domain cube; a probe only adds nodes whose monopole is the one particle beside it, or nothing).  1e-9 of the largest
    acceleration, as the strict walk against these oracle walks in test_lattice.py."""
    c = _lattice_case(pkg, O)
    cfg, pos, mass, typ, probes, ptype, a, ni, lat = (c[x] for x in ("cfg", "pos", "mass", "typ", "probes", "ptype", "a", "ni", "lat"))
    n, k = len(pos), len(probes)
    dom = O.domain_extent(pos)
    T = O.Tree(cfg, pos, mass, typ, dom)
    a_on, n_on = T.walk(idx=c["on"])
    assert np.all(n_on == n)                         # the force walk: every source
    a_on, n_on = O.lattice_walk(T, a_on, n_on, lat, idx=c["on"])
    a_on, _ = O.finish(cfg, a_on)
    free = np.r_[0:400, 600:k]
    upos = np.concatenate([pos, probes[free]])
    assert np.array_equal(O.domain_extent(upos), dom)
    U = O.Tree(cfg, upos, np.concatenate([mass, np.zeros(len(free))]), np.concatenate([typ, ptype[free]]), dom)
    idx = (n + np.arange(len(free))).astype(np.int32)
    a_free, n_free = U.walk(idx=idx)
    nearest = O.direct(cfg, upos, np.concatenate([mass, np.zeros(len(free))]), np.concatenate([typ, ptype[free]]), idx)
    assert _maxerr(a_free * cfg.G, nearest) < TOL    # ... and is the nearest-image direct sum
    a_free, _ = O.lattice_walk(U, a_free, n_free, lat, idx=idx)
    a_free, _ = O.finish(cfg, a_free)
    scale = np.abs(a_free).max()
    e_on, e_free = np.abs(a[400:600] - a_on).max() / scale, np.abs(a[free] - a_free).max() / scale
    print("periodic tree-only vs the oracle's two walks: on particles %.2e, elsewhere %.2e of the largest acceleration" % (e_on, e_free))
    assert e_on < 1e-9 and e_free < 1e-9
    assert np.array_equal(ni[400:600], n_on)
    assert np.all(ni > n) and np.all(ni <= 2 * n)    # every source in the force walk, then the correction walk's nodes and particles


@pytest.mark.gpu
def test_opening_everything_periodic_tree_only_against_direct_lattice(pkg, O):
    """oracle_py.direct_lattice with the probes as zero-mass rows, at the tolerance direct_lattice is held to in test_lattice.py
    (1e-4 max, 2e-5 median relative error per target).  With err_tol_theta = 0 and old_acc = 0 the force walk is a direct sum, the
    lattice-correction walk still sums monopoles of nodes up to 0.2 BoxSize (test above), so the walks are the direct sum only as
    far as those monopoles stand for their particles: a node of rms radius s is off by (s / BoxSize)^2 of its correction, and the
    correction is 4 (r / BoxSize)^3 of the nearest-image force at distance r.  In a uniform box neither factor is small and the
    reference's own walks are 1.7e-2 (max) / 1.2e-3 (median) from direct_lattice (the oracle alone, on the CPU); for a clump of
    radius 0.05 BoxSize and probes within 0.07 BoxSize of its centre both are, and the reference's own walks are 2.6e-6 / 6.6e-7 from
    it (the oracle alone, these inputs) -- a factor 40 and 30 inside the tolerance.  So here: such a clump, wrapped around the faces x = 0 and z = BoxSize, probes of
    every type inside it, on particles, and on those two faces with coordinates exactly 0 and exactly BoxSize."""
    c = _lattice_case(pkg, O)
    cfg, lat = c["cfg"], c["lat"]
    n, k, L = 4000, COUNTS[-1], cfg.box_size
    rng = np.random.default_rng(43)
    centre = np.array([0.02, 0.5, 0.98]) * L

    def ball(m, radius):
        v = rng.normal(0, 1, (m, 3))
        return centre + v / np.linalg.norm(v, axis=1)[:, None] * radius * rng.uniform(0, 1, (m, 1)) ** (1 / 3)
    pos = np.mod(ball(n, 0.05 * L), L)
    mass = rng.uniform(0.5, 1.5, n) / n
    typ = (1 + np.arange(n) % 5).astype(np.int32)
    probes, ptype = np.mod(ball(k, 0.07 * L), L), _probe_types(k)
    probes[600:800] = pos[rng.choice(n, 200, replace=False)]
    probes[800:900, 0] = 0.0
    probes[900:1000, 2] = L
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.force_treebuild()
    call = lambda p, t: eng.gravity_tree_targets(p, t, want_nint=True)   # noqa: E731
    a, ni = call(probes, ptype)
    _prefixes_agree(call, probes, ptype, (a, ni))
    eng.close()
    # (direct_lattice skips the lattice term of a pair at zero distance, forcetree.c:3519-3528: probes on particles may stay)
    want = O.direct_lattice(cfg, np.concatenate([pos, probes]), np.concatenate([mass, np.zeros(k)]), np.concatenate([typ, ptype]),
                            n + np.arange(k, dtype=np.int32), lat)   # (x G)
    e = rel_err(a, want)
    print("everything opened, periodic tree-only clump vs direct_lattice: rel err max %.2e median %.2e (inside %.2e, on particles %.2e, "
          "faces %.2e)" % (e.max(), np.median(e), max(e[:600].max(), e[1000:].max()), e[600:800].max(), e[800:1000].max()))
    assert e.max() < 1e-4 and np.median(e) < 2e-5
    assert np.all(ni > n) and np.all(ni <= 2 * n)


def _relative_pass(pkg, cfg, pos, mass, typ):
    """an engine after the Barnes-Hut pass and the relative-criterion pass that walks with its OldAcc: (eng, OldAcc column, acc, pm)"""
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
    _, old, _ = eng.get_accel()
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
    if cfg.pmgrid:
        acc, _, _, pm = eng.get_accel(want_pm=True)
    else:
        acc, pm = eng.get_accel()[0], 0.0
    return eng, old, acc, pm


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["tree_only", "treepm"])
def test_real_criterion_at_arbitrary_points(pkg, regime):
    """2 000 probes = particle positions displaced by one softening length in a random direction (distributed as the particles
    are), with the particles' type, mass and OldAcc, under the relative criterion: the rms relative error against the direct sum
    (Engine.direct_sum / direct_sum_targets, Ewald-corrected in the periodic run; pinned to the oracle by test_gpu_parity.py and
    test_lattice.py) is at most 1.25 x that of the own strict walk on the same particles -- equal in law, 25 % for the sampling
    noise of an rms over 2 000 heavy-tailed samples.  TreePM: walk + pm_targets."""
    n, k = 20000, 2000
    if regime == "tree_only":
        pos, mass, typ = pkg.ic.plummer_sphere(n, seed=51)
        eps, L = 0.01, 0.0
        cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[eps] * 6, walk_mode=pkg.WALK_STRICT)
    else:
        L = 1e4
        pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=52)
        eps = L / (40 * n ** (1 / 3))
        cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=32, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
                              type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4", walk_mode=pkg.WALK_STRICT)
    eng, old, acc, pm = _relative_pass(pkg, cfg, pos, mass, typ)
    rng = np.random.default_rng(53)
    idx = np.sort(rng.choice(n, k, replace=False)).astype(np.int32)
    d = rng.normal(0, 1, (k, 3))
    probes = pos[idx] + eps * d / np.linalg.norm(d, axis=1)[:, None]
    if L:
        probes = np.mod(probes, L)
    a = eng.gravity_tree_targets(probes, typ[idx], old_acc=old[idx], mass=mass[idx])
    if L:
        a = a + eng.pm_targets(probes, typ[idx])
    e_own = _rms(rel_err((acc + pm)[idx], eng.direct_sum(idx)))
    e_probe = _rms(rel_err(a, eng.direct_sum_targets(probes, typ[idx], mass=mass[idx])))
    print("real criterion [%s]: rms rel err own strict walk %.3e, probes %.3e, ratio %.3f" % (regime, e_own, e_probe, e_probe / e_own))
    assert e_probe <= 1.25 * e_own
    eng.close()


@pytest.mark.gpu
def test_two_engines_tree_only(pkg, O):
    """a set split at the median x into engines A and B: for A's particles, A's own strict walk plus B's walk for them as foreign
    targets is the force of the union -- the oracle's direct sum to 1e-10 with everything opened, and within the band of
    test_real_criterion_at_arbitrary_points of ONE engine's strict walk over the union with the real criterion.  The two errors
    come from different trees, so unlike there they are not correlated sample by sample, and the ratio of two heavy-tailed rms
    values is noisier: the largest set the file uses, 10 000 targets (measured 1.13; with 6 000 particles, 3 000 targets, 1.255)"""
    n = 20000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=61)
    kw = dict(n_gravs=1, softening=[0.01] * 6, walk_mode=pkg.WALK_STRICT)
    inA = pos[:, 0] < np.median(pos[:, 0])
    rows = np.flatnonzero(inA).astype(np.int32)

    def split_force(theta, old_acc):
        tot = None
        for own in (inA, ~inA):
            e = pkg.Engine(pkg.make_config(G=1.0, theta=theta, **kw))
            e.set_particles(pos[own], mass[own], typ[own], old_acc=None if old_acc is None else old_acc[own])
            e.compute_accelerations(pm_step=False)
            part = e.get_accel()[0] if own is inA else e.gravity_tree_targets(pos[inA], typ[inA], old_acc=None if old_acc is None else old_acc[inA],
                                                                               mass=mass[inA])
            tot = part if tot is None else tot + part
            e.close()
        return tot
    cfg = pkg.make_config(G=1.0, theta=0.5, **kw)
    want = O.direct(cfg, pos, mass, typ, rows)
    err = _maxerr(split_force(0.0, None), want)
    print("two engines, everything opened: max err %.2e of the largest acceleration" % err)
    assert err < TOL
    one, old, acc, _ = _relative_pass(pkg, cfg, pos, mass, typ)
    one.close()
    e_one, e_split = _rms(rel_err(acc[rows], want)), _rms(rel_err(split_force(0.0, old), want))
    print("two engines, real criterion: rms rel err one engine %.3e, A + B at A's particles %.3e, ratio %.3f" % (e_one, e_split, e_split / e_one))
    assert e_split <= 1.25 * e_one


@pytest.mark.gpu
def test_two_engines_mesh_force(pkg):
    """periodic TreePM, same box and mesh: GravPM of A's PM step plus B.pm_targets(A's particles) is GravPM of one engine holding
    the union (the mesh force is linear in the density)"""
    n, L, N = 6000, 1.0, 24
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=62)
    cfg_kw = dict(n_gravs=2, periodic=1, pmgrid=N, box_size=L, G=1.7, theta=0.5, softening=[L / 1000] * 6,
                  type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4")
    inA = pos[:, 0] < np.median(pos[:, 0])
    pm = {}
    for name, own in (("A", inA), ("B", ~inA), ("U", np.ones(n, dtype=bool))):
        e = pkg.Engine(pkg.make_config(**cfg_kw))
        e.set_particles(pos[own], mass[own], typ[own])
        e.domain_Decomposition()
        e.pmforce_periodic()
        pm[name] = e.pm_targets(pos[inA], typ[inA]) if name == "B" else e.get_pm()
        e.close()
    err = _maxerr(pm["A"] + pm["B"], pm["U"][inA])
    print("two engines, mesh force: max err %.2e of max |GravPM|" % err)
    assert err < TOL


@pytest.mark.gpu
@pytest.mark.parametrize("N", [16, 24, 32])
def test_mesh_force_at_foreign_targets(pkg, N):
    n, k, L = 5000, COUNTS[-1], 1.0 if N != 24 else 1e4
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=70 + N)
    mass = np.random.default_rng(71).uniform(0.5, 1.5, n) / n
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=N, box_size=L, G=43007.1 if L > 1 else 1.7, theta=0.5, softening=[L / 700] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4")
    rng = np.random.default_rng(72)
    probes = rng.uniform(0, L, (k, 3))
    probes[0] = L                                   # every coordinate exactly BoxSize
    probes[1] = 0.0
    probes[2, 0] = L
    probes[3] = (3 * L / N, 0.0, (N - 1) * L / N)   # a cell corner at the seam
    ptype = _probe_types(k)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.force_treebuild()
    with pytest.raises(pkg.NgravsError, match="status -4"):      # (d) before any PM step: no valid mesh
        eng.pm_targets(probes, ptype)
    eng.pmforce_periodic()
    own = eng.get_pm()
    # (a) own positions with own types: the engine's own GravPM.  NOT bit-equal in general: the own rows go through the force-mesh
    # march and its gather, the targets through the fused gather -- the same expressions, which the compiler contracts into other
    # multiply-adds (measured: bit-equal at N = 16 and 32 in a unit box, 6.3e-16 of max |GravPM| at N = 24 in a box of 1e4)
    at_own = eng.pm_targets(pos, typ)
    print("pm_targets at own positions [N=%d]: max diff %.2e of max |GravPM|, bit-equal: %s" %
          (N, np.abs(at_own - own).max() / np.abs(own).max(), np.array_equal(at_own, own)))
    assert np.abs(at_own - own).max() <= 1e-13 * np.abs(own).max()
    # (b) arbitrary probes of every type: the reference over particles and probes, the probes at zero mass (+0.0 changes no mesh value)
    got = eng.pm_targets(probes, ptype)
    ref = pm_reference.pm_periodic(cfg, np.concatenate([pos, probes]), np.concatenate([mass, np.zeros(k)]), np.concatenate([typ, ptype]))[n:]
    err = _maxerr(got, ref)
    print("pm_targets at probes [N=%d]: %.2e of max |GravPM|" % (N, err))
    assert np.isfinite(got).all() and err < TOL
    _prefixes_agree(lambda p, t: (eng.pm_targets(p, t),), probes, ptype, (got,))
    # (c) a step without PM, with moved particles: the mesh of the last PM step is still the one that answers
    moved = np.mod(pos + rng.normal(0, 0.01 * L, (n, 3)), L)
    eng.set_particles(moved, mass, typ, grav_pm=own)
    eng.compute_accelerations(pm_step=False)
    assert np.array_equal(eng.pm_targets(probes, ptype), got)
    eng.close()


def _targets(pkg, pos, typ, old_acc=None, mass=None):
    tg = pkg.abi.GravTargets()
    tg.pos, tg.pos_stride = pos.ctypes.data, 24
    tg.type, tg.type_stride = typ.ctypes.data, 4
    if old_acc is not None:
        tg.old_acc, tg.old_acc_stride = old_acc.ctypes.data, 8
    if mass is not None:
        tg.mass, tg.mass_stride = mass.ctypes.data, 8
    return tg


@pytest.mark.gpu
def test_refusals_write_nothing_and_disturb_nothing(pkg, have_lib):
    """every row of the header's refusal table: the status, the message, result buffers (pre-filled with -3.25 / -3) untouched; and
    after all of it, and successful calls between, the engine's own results and a repeated gravity_tree are bit for bit what they
    were"""
    lib = have_lib
    n, k, L, N = 3000, 65, 1.0, 16
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=81)
    typ[::7] = 0                                     # some gas, for the adaptive-softening row
    cfg_kw = dict(n_gravs=2, periodic=1, pmgrid=N, box_size=L, G=1.7, theta=0.5, softening=[L / 600] * 6,
                  type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4", walk_mode=pkg.WALK_STRICT)
    rng = np.random.default_rng(82)
    probes, ptype = rng.uniform(0, L, (k, 3)), _probe_types(k)
    acc, nint = np.full((k, 3), -3.25), np.full(k, -3, dtype=np.int32)

    def refused(eng, which, status, word, tg, nt=k, result=True):
        h = eng._h
        tgp = C.byref(tg) if tg is not None else None
        out = acc.ctypes.data if result else None
        if which == "walk":
            rc = lib.ngravs_gravity_tree_targets(h, tgp, nt, out, nint.ctypes.data, None)
        else:
            rc = lib.ngravs_pm_targets(h, tgp, nt, out)
        msg = lib.ngravs_last_error(h).decode()
        assert rc == status, (which, word, rc, msg)
        assert word in msg, (which, word, msg)
        assert np.all(acc == -3.25) and np.all(nint == -3), (which, word)

    eng = pkg.Engine(pkg.make_config(**cfg_kw))
    eng.set_particles(pos, mass, typ)
    good = _targets(pkg, probes, ptype)
    refused(eng, "walk", -4, "built tree", good)                 # no built tree
    eng.domain_Decomposition()
    eng.force_treebuild()
    refused(eng, "pm", -4, "mesh", good)                         # no valid mesh
    eng.compute_accelerations(pm_step=True)
    before = eng.get_accel(want_pm=True)
    ok_walk, ok_pm = eng.gravity_tree_targets(probes, ptype), eng.pm_targets(probes, ptype)
    for which in ("walk", "pm"):
        refused(eng, which, -1, "NULL", None)
        refused(eng, which, -1, "pos is NULL", pkg.abi.GravTargets(type=ptype.ctypes.data, type_stride=4))
        refused(eng, which, -1, "type is NULL", pkg.abi.GravTargets(pos=probes.ctypes.data, pos_stride=24))
        refused(eng, which, -1, "NULL", good, result=False)
        refused(eng, which, -1, "nt", good, nt=-1)
        bad_t = ptype.copy()
        bad_t[3] = 6
        refused(eng, which, -1, "type", _targets(pkg, probes, bad_t))
        bad_t[3] = -1
        refused(eng, which, -1, "type", _targets(pkg, probes, bad_t))
        for v in (np.nan, np.inf):
            bad_p = probes.copy()
            bad_p[64, 1] = v
            refused(eng, which, -1, "finite", _targets(pkg, bad_p, ptype))
        for v in (-1e-9, L + 1e-9):
            bad_p = probes.copy()
            bad_p[0, 2] = v
            refused(eng, which, -1, "BoxSize", _targets(pkg, bad_p, ptype))
        assert np.array_equal(eng.gravity_tree_targets(probes, ptype), ok_walk) and np.array_equal(eng.pm_targets(probes, ptype), ok_pm)
    # nt = 0: NGRAVS_OK, nothing written
    assert lib.ngravs_gravity_tree_targets(eng._h, C.byref(good), 0, acc.ctypes.data, nint.ctypes.data, None) == 0
    assert lib.ngravs_pm_targets(eng._h, C.byref(good), 0, acc.ctypes.data) == 0
    assert np.all(acc == -3.25) and np.all(nint == -3)
    after = eng.get_accel(want_pm=True)
    eng.gravity_tree()
    again = eng.get_accel(want_pm=True)
    for b, a, g in zip(before, after, again):
        assert np.array_equal(b, a) and np.array_equal(b, g)
    # adaptive gas softening on: explicit targets carry no softening length
    eng.set_gas_softening(np.full(n, L / 300))
    for which in ("walk", "pm"):
        refused(eng, which, -4, "adaptive gas softening is on and explicit targets carry no softening length", good)
    eng.close()
    # no mesh in the configuration
    tree_only = pkg.Engine(pkg.make_config(**dict(cfg_kw, pmgrid=0)))
    tree_only.set_particles(pos, mass, typ)
    tree_only.compute_accelerations(pm_step=False)
    refused(tree_only, "pm", -4, "PMGRID", good)
    tree_only.close()
    # several tasks
    two = pkg.Engine(pkg.make_config(world_size=2, rank=0, **cfg_kw))
    two.set_particles(pos, mass, typ)
    for which in ("walk", "pm"):
        refused(two, which, -4, "single task only", good)
    two.close()
    # outside a periodic configuration any finite position is served
    free = pkg.Engine(pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6, walk_mode=pkg.WALK_STRICT))
    free.set_particles(pos, mass, np.ones(n, dtype=np.int32))
    free.compute_accelerations(pm_step=False)
    far = free.gravity_tree_targets(np.array([[-7.0, 1e6, 3.0]]), np.array([1], dtype=np.int32))
    assert np.isfinite(far).all() and np.abs(far).max() > 0
    free.close()


@pytest.mark.gpu
def test_device_pointers_give_the_host_results(pkg):
    import torch
    n, k, L = 5000, COUNTS[-1], 1e4
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=91)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=16, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4", walk_mode=pkg.WALK_STRICT)
    eng, old, _, _ = _relative_pass(pkg, cfg, pos, mass, typ)
    rng = np.random.default_rng(92)
    probes, ptype = rng.uniform(0, L, (k, 3)), _probe_types(k)
    poa, pmass = old[rng.choice(n, k)], rng.uniform(0.5, 1.5, k)
    a, ni = eng.gravity_tree_targets(probes, ptype, old_acc=poa, mass=pmass, want_nint=True)
    g = eng.pm_targets(probes, ptype)
    dev = lambda x: torch.from_numpy(x).cuda()   # noqa: E731
    a_d, ni_d = eng.gravity_tree_targets(dev(probes), dev(ptype), old_acc=dev(poa), mass=dev(pmass), want_nint=True)
    g_d = eng.pm_targets(dev(probes), dev(ptype))
    assert a_d.is_cuda and ni_d.is_cuda and g_d.is_cuda
    assert np.array_equal(a_d.cpu().numpy(), a) and np.array_equal(ni_d.cpu().numpy(), ni) and np.array_equal(g_d.cpu().numpy(), g)
    eng.close()
