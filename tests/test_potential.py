"""Gravitational potentials on the device: ngravs_compute_potential, ngravs_potential_targets, ngravs_lattice_potential_table and
Timeline(potential="device"), held to tests/potential_ref.py (direct pair sums, the reference's ewald_psi restated, the mesh of
tests/pm_reference.py) -- the reference's own potential routines are broken and cannot be the truth.

Bounds:
  * everything opened (err_tol_theta = 1e-6): |pot - pairsum| <= 1e-12 sum_j |term_ij| per row; the rounding of a sum of N terms is
    N eps = 1.1e-13 of that at N = 1037, so the margin is 10x.  One particle: |pot| <= 4 ulp of G m / eps (the walk's own term
    and the self term are the same operations with opposite signs).
  * own rows handed in as targets: bit for bit (the walk of a lane does not depend on its wave-mates); the test's G is a power of
    two so that "x G" commutes with the sums.
  * lattice table: 1e-10 of max|table| (libm erfc / exp / cos on device and host); mesh: 1e-10 of max|pot|, TOL of
    test_gpu_pm_mesh.py; short-range part: 1e-9 of sum|term| against the pair sum cut at tab < NTAB.  (The walk
    prunes by the eff_dist box with the table's reach, 6 Asmth.  With the reference's rcut = 4.5 Asmth in it the box drops pairs
    worth erfc(2.25) = 1.5e-3 of m / r each -- u = r / 2 Asmth -- and the walk misses this bound by 4e4 to 1.4e5 times, measured.)
  * against exact Ewald sums: at most 1.5 x the deviation the CPU restatement shows on the same input.
"""
import ctypes as C
import functools
import os

import numpy as np
import pytest
from scipy.special import erf

import potential_ref as R

SIZES = (1, 2, 63, 65, 1037)     # one lane, one pair, a partial wave, a wave and a lane, five blocks with a partial wave
COUNTS = (1, 63, 65, 1037)       # COUNTS of test_gravity_targets.py
T2G = [0, 1, 0, 1, 0, 1]
BOX = 10.0


def _wiring(pkg, name):
    if name == "newton":
        return "newton"
    A = pkg.abi
    law = [[A.LAW_NEWTON, A.LAW_NEG_NEWTON], [A.LAW_NEG_NEWTON, A.LAW_NEWTON]]
    return {"accel": law, "spline": [[A.SPLINE_PLUMMER, A.SPLINE_NEG_PLUMMER], [A.SPLINE_NEG_PLUMMER, A.SPLINE_PLUMMER]], "greens": law,
            "normed": law}


def _engine(pkg, eps, wiring="newton", G=2.0, theta=1e-6, periodic=0, pmgrid=0, **kw):
    cfg = pkg.make_config(n_gravs=2, periodic=periodic, pmgrid=pmgrid, box_size=BOX if periodic else 0.0, G=G, theta=theta, softening=eps,
                          type_to_grav=T2G, wiring=_wiring(pkg, wiring), walk_mode=pkg.WALK_STRICT, **kw)
    return cfg, pkg.Engine(cfg)


def _load(eng, pos, mass, typ, old_acc=None):
    eng.set_particles(pos, mass, typ, old_acc=old_acc)
    eng.domain_Decomposition()
    eng.force_treebuild()


@functools.lru_cache(maxsize=None)
def _ref_lattice_table():
    return R.lattice_table(1.0, BOX)       # 274 625 Ewald sums in numpy: once for the module


def _rms(e):
    return float(np.sqrt(np.mean(e ** 2)))


# ---- CPU -----------------------------------------------------------------------------------------------------------------------
def test_null_context_is_refused_with_the_outputs_untouched(pkg, have_lib):
    tg = pkg.abi.GravTargets()
    out = np.full(4, -3.25)
    nint = np.full(4, -3, dtype=np.int32)
    tab = np.full(65 ** 3, -3.25)
    assert have_lib.ngravs_compute_potential(None, None, out.ctypes.data, 8, 0, nint.ctypes.data) == -1
    assert have_lib.ngravs_potential_targets(None, C.byref(tg), 4, out.ctypes.data, nint.ctypes.data) == -1
    assert have_lib.ngravs_lattice_potential_table(None, 0, 0, tab.ctypes.data) == -1
    assert np.all(out == -3.25) and np.all(nint == -3) and np.all(tab == -3.25)


def test_engine_argument_checks_need_no_device(pkg):
    eng = pkg.Engine.__new__(pkg.Engine)        # no context: the checks come before anything that needs one
    eng._h, eng.n = C.c_void_p(), 5
    ok_pos, ok_typ = np.zeros((5, 3)), np.zeros(5, dtype=np.int32)
    for pos, typ in [(np.zeros((5, 2)), ok_typ), (np.zeros(5), ok_typ), (np.zeros((5, 3), dtype=np.int64), ok_typ), (ok_pos, np.zeros(5)),
                     (ok_pos, np.zeros(4, dtype=np.int32))]:
        with pytest.raises(ValueError):
            eng.potential_targets(pos, typ)
    for into in (np.zeros(5, dtype=np.float32), np.zeros((5, 1)), np.zeros(10)[::2], np.zeros(4)):
        with pytest.raises(ValueError):
            eng.compute_potential(into=into)
    for t, s in ((-1, 0), (0, 3), (0.5, 0)):
        with pytest.raises(ValueError):
            eng.lattice_potential_table(t, s)


def test_long_range_table_is_pi_erf_u_over_u(pkg, have_lib):
    """E = (force_tab + pot_tab) u of the library's own tables is tempI / u: pi erf(u) / u for Newton, its negative for neg-Newton"""
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=16, box_size=BOX, softening=[0.01] * 6, type_to_grav=T2G, wiring=_wiring(pkg, "cross"))
    E = R.e_table(pkg, cfg)
    u = 3.0 / R.NTAB * (np.arange(R.NTAB) + 0.5)
    want = np.pi * erf(u) / u
    for a in range(2):
        for b in range(2):
            sign = 1.0 if a == b else -1.0
            err = np.abs(E[a, b] - sign * want).max() / np.abs(want).max()
            print("E[%d][%d]: %.2e" % (a, b, err))
            assert np.all(np.abs(E[a, b] - sign * want) <= 1e-12 * np.abs(want))


def test_restated_ewald_psi_against_a_brute_force_image_sum():
    """three points of the octant; the bound is the l = 4 multipole of what the sphere of images cuts off (potential_ref.psi_brute)"""
    for x in ([0.3, 0.1, 0.2], [0.5, 0.5, 0.5], [0.05, 0.4, 0.0]):
        a, b = float(R.ewald_psi(np.array(x))), R.psi_brute(np.array(x))
        print(x, a, b, a - b)
        assert abs(a - b) <= R.psi_brute_bound()
    assert abs(float(R.ewald_psi(np.array([1e-4, 0.0, 0.0]))) - R.LATTICE_ZERO) < 1e-6    # psi -> LatticeZero at the origin


# ---- GPU: 1. tree-only, not periodic, everything opened --------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["newton", "cross"])
@pytest.mark.parametrize("n", SIZES)
def test_everything_opened_is_the_pair_sum(pkg, n, wiring):
    pos, mass, typ, eps = R.particle_set(n, 100 + n)
    cfg, eng = _engine(pkg, eps, wiring)
    _load(eng, pos, mass, typ)
    pot, nint = eng.compute_potential(want_nint=True)
    terms = R.pair_terms(cfg, pos, mass, typ)
    want = R.tail(cfg, None, pos, mass, typ, terms.sum(1))
    bound = 1e-12 * cfg.G * np.abs(terms).sum(1)        # (the row's own term, 2.8 m / h, is one of them)
    print("n = %d %s: max |pot - pairsum| / bound = %.3f" % (n, wiring, (np.abs(pot - want) / bound).max()))
    assert nint.max() <= n                 # (a cell of coincident particles may stand for them even at theta = 1e-6)
    if n == 1:
        print("one particle: pot = %.3e, 4 ulp = %.3e" % (pot[0], 4 * np.spacing(cfg.G * mass[0] / eps[typ[0]])))
        assert abs(pot[0]) <= 4 * np.spacing(cfg.G * mass[0] / eps[typ[0]])
    assert np.all(np.abs(pot - want) <= bound)
    # the same in the caller's order after a shuffled hand-over
    perm = np.random.default_rng(n).permutation(n)
    _load(eng, pos[perm], mass[perm], typ[perm])
    assert np.all(np.abs(eng.compute_potential() - want[perm]) <= bound[perm])
    eng.close()


# ---- 2. opening rules ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_opening_rules_are_the_force_walks(pkg):
    n = 1037
    pos, mass, typ, eps = R.particle_set(n, 7)
    rng = np.random.default_rng(8)
    old = rng.uniform(0.5, 2.0, n) * 5.0
    cfg, eng = _engine(pkg, eps, theta=0.5)
    _load(eng, pos, mass, typ, old_acc=old)
    probes = rng.uniform(-0.3, 1.3, (COUNTS[-1], 3))          # some outside the domain cube
    ptyp = (np.arange(COUNTS[-1]) % 6).astype(np.int32)
    pold = rng.uniform(0.5, 2.0, COUNTS[-1]) * 5.0
    fs = np.array(cfg.force_softening[:])[typ]
    for crit in ("barnes-hut", "relative"):
        if crit == "relative":
            eng.set_opening(0.0, 0.005)
        for k in COUNTS:
            _, ni_f = eng.gravity_tree_targets(probes[:k], ptyp[:k], old_acc=pold[:k], want_nint=True)
            p, ni_p = eng.potential_targets(probes[:k], ptyp[:k], old_acc=pold[:k], want_nint=True)
            assert np.array_equal(ni_p, ni_f), (crit, k)
            assert ni_p.max() < n                              # (nodes were used: the criterion was at work)
        # own rows as targets, self term and tail in numpy, in the device's order of operations: compute_potential bit for bit
        own, ni_own = eng.potential_targets(pos, typ, old_acc=old, mass=mass, want_nint=True)
        pot, ni = eng.compute_potential(want_nint=True)
        assert np.array_equal(ni, ni_own), crit
        assert np.array_equal((own / cfg.G + mass * (1.0 / fs) * 2.8) * cfg.G, pot), crit
    eng.close()


# ---- 3. accuracy at theta = 0.5 ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_accuracy_at_theta_half_is_no_worse_than_the_force_walks(pkg):
    """all-Newton Plummer sphere.  The quadrupole coefficient of the monopole potential's relative error is 1/3 of the force's, so
    the potential's rms relative error must not exceed the strict force walk's on the same set."""
    n = 1037
    pos, mass, _ = pkg.ic.plummer_sphere(n, seed=3)
    typ = (np.arange(n) % 6).astype(np.int32)
    eps = [0.01] * 6
    cfg, eng = _engine(pkg, eps, theta=0.5, G=1.0)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    acc, _, _ = eng.get_accel()
    ref = eng.direct_sum(np.arange(n))
    e_force = _rms(np.linalg.norm(acc - ref, axis=1) / np.linalg.norm(ref, axis=1))
    pot = eng.compute_potential()
    want = R.tail(cfg, None, pos, mass, typ, R.pair_terms(cfg, pos, mass, typ).sum(1))
    e_pot = _rms((pot - want) / want)
    print("theta = 0.5, Plummer n = %d: rms relative error potential %.3e, strict force walk %.3e" % (n, e_pot, e_force))
    assert e_pot <= e_force
    eng.close()


# ---- 4. periodic tree-only --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["newton", "cross"])
def test_periodic_tree_only_lattice_term(pkg, wiring):
    n = 255
    pos, mass, typ, eps = R.particle_set(n, 21, box=BOX)
    cfg, eng = _engine(pkg, eps, wiring, periodic=1)
    _load(eng, pos, mass, typ)
    # the table
    ref = _ref_lattice_table()
    tabs = {}
    for a in range(2):
        for b in range(2):
            sign = R.law_sign(cfg.law_accel[a][b])
            tabs[a, b] = t = eng.lattice_potential_table(a, b)
            err = np.abs(t - sign * ref).max() / np.abs(ref).max()
            print("lattice table [%d][%d]: max err %.2e of max|table|" % (a, b, err))
            assert err <= 1e-10
            assert t[0, 0, 0] == sign * 2.8372975 / BOX
    # everything opened: the pair sum plus the lookup in that same table
    g = R.species(cfg, typ)
    d, r = R.separations(cfg, pos, pos)
    look = np.zeros((n, n))
    for a in range(2):
        for b in range(2):
            m = (g[:, None] == a) & (g[None, :] == b)
            look[m] = (mass[None, :] * R.lat_lookup(tabs[a, b], 2.0 * 64 / BOX, d))[m]
    terms = R.pair_terms(cfg, pos, mass, typ)
    bound = 1e-12 * cfg.G * (np.abs(terms).sum(1) + np.abs(look).sum(1))
    want = R.tail(cfg, None, pos, mass, typ, (terms + look).sum(1))
    pot = eng.compute_potential()
    print("%s: max |pot - (pairsum + lookup)| / bound = %.3f" % (wiring, (np.abs(pot - want) / bound).max()))
    assert np.all(np.abs(pot - want) <= bound)
    # against exact Ewald sums
    exact = R.tail(cfg, None, pos, mass, typ, R.ewald_exact(cfg, pos, mass, typ))
    dev_gpu, dev_ref = np.abs(pot - exact).max(), np.abs(want - exact).max()
    print("%s: deviation from exact Ewald: device %.3e, restatement %.3e (max |pot| %.3e)" % (wiring, dev_gpu, dev_ref, np.abs(exact).max()))
    assert dev_gpu <= 1.5 * dev_ref
    eng.close()


# ---- 5. TreePM --------------------------------------------------------------------------------------------------------------------
def _k0_offset(cfg, mass, typ):
    """k = 0 of the mesh is 0, as for the force: the mean of the short-range potential, -4 pi Asmth^2 / L^3 per unit mass, is
    therefore missing from Ewald's mean-zero potential.  Per target: G sum_j sign_ij m_j 4 pi Asmth^2 / L^3."""
    asmth = 1.25 * BOX / cfg.pmgrid
    g = R.species(cfg, typ)
    cn, _ = R._coeffs(cfg, g, g)
    return cfg.G * (cn * mass[None, :]).sum(1) * 4 * np.pi * asmth ** 2 / BOX ** 3


@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["newton", "cross"])
@pytest.mark.parametrize("pmgrid", [16, 32])
def test_treepm_short_range_mesh_and_total(pkg, pmgrid, wiring):
    n = 255
    pos, mass, typ, eps = R.particle_set(n, 31, box=BOX)
    cfg, eng = _engine(pkg, eps, wiring, periodic=1, pmgrid=pmgrid)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    before = eng.get_accel(want_pm=True)
    probes = np.random.default_rng(32).uniform(0, BOX, (65, 3))
    ptyp = (np.arange(65) % 6).astype(np.int32)
    eng.pm_targets(probes, ptyp)                               # served: the mesh of the PM step
    with pytest.raises(pkg.NgravsError, match="status -4"):    # no compute_potential yet: no potential mesh
        eng.potential_targets(probes, ptyp)
    pot = eng.compute_potential()
    after = eng.get_accel(want_pm=True)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)                            # GravAccel, OldAcc, GravCost, GravPM: bit-equal
    with pytest.raises(pkg.NgravsError, match="status -4"):    # the mesh is no longer the PM step's
        eng.pm_targets(probes, ptyp)
    # short-range part: the pair sum cut at tab < NTAB
    E = R.e_table(pkg, cfg)
    terms = R.pair_terms(cfg, pos, mass, typ, table=E)
    mesh = R.mesh_potential(cfg, pos, mass, typ)
    self_term = 2.8 * mass / np.array(cfg.force_softening[:])[typ]
    short = (pot - mesh) / cfg.G - self_term
    bound = 1e-9 * np.abs(terms).sum(1)
    print("PMGRID %d %s: max |short - pairsum| / bound = %.3e" % (pmgrid, wiring, (np.abs(short - terms.sum(1)) / bound).max()))
    assert np.all(np.abs(short - terms.sum(1)) <= bound)
    # the total against exact Ewald sums (the row's own images included), in the mesh's k = 0 convention
    want = R.tail(cfg, None, pos, mass, typ, terms.sum(1), mesh)
    cfg0 = pkg.make_config(n_gravs=2, periodic=1, box_size=BOX, G=cfg.G, softening=eps, type_to_grav=T2G, wiring=_wiring(pkg, wiring))
    exact = R.tail(cfg0, None, pos, mass, typ, R.ewald_exact(cfg0, pos, mass, typ)) - _k0_offset(cfg, mass, typ)
    dev_gpu, dev_ref = np.abs(pot - exact).max(), np.abs(want - exact).max()
    print("PMGRID %d %s: deviation from exact Ewald: device %.3e, restatement %.3e (max |pot| %.3e)" %
          (pmgrid, wiring, dev_gpu, dev_ref, np.abs(exact).max()))
    assert dev_gpu <= 1.5 * dev_ref
    # served now, walk x G + mesh at the probes
    p = eng.potential_targets(probes, ptyp)
    want_p = cfg.G * R.pair_terms(cfg, pos, mass, typ, probes, ptyp, table=E).sum(1) + R.mesh_potential(cfg, pos, mass, typ, probes, ptyp)
    assert np.abs(p - want_p).max() <= 1e-9 * np.abs(want_p).max()
    eng.close()


@pytest.mark.gpu
@pytest.mark.parametrize("pmgrid", [16, 32])
def test_treepm_mesh_part_alone(pkg, pmgrid):
    """Where the walk contributes nothing or a known constant, the rest is the mesh part: (a) targets farther than 6 Asmth from
    every particle (tab >= NTAB for every pair: the walk's sum is exactly 0); (b) own rows all farther than 6 Asmth from one
    another: the walk is the row's own term, -2.8 m / h + m E[0] / (2 pi Asmth), which the self term and E[0] take out."""
    cfg, eng = _engine(pkg, [0.004] * 6, "cross", periodic=1, pmgrid=pmgrid)
    rng = np.random.default_rng(41)
    # (a) a clump in [0, 0.3 L]^3, probes around 0.65 L: every nearest-image separation is at least 0.33 L per dimension
    n = 300
    pos = rng.uniform(0, 0.3 * BOX, (n, 3))
    mass, typ = rng.uniform(0.5, 2.0, n) / n, rng.integers(0, 6, n).astype(np.int32)
    _load(eng, pos, mass, typ)
    eng.compute_potential()
    for k in COUNTS:
        probes = 0.65 * BOX + rng.uniform(-0.02, 0.02, (k, 3)) * BOX
        ptyp = (np.arange(k) % 6).astype(np.int32)
        p, ni = eng.potential_targets(probes, ptyp, want_nint=True)
        want = R.mesh_potential(cfg, pos, mass, typ, probes, ptyp)
        assert np.all(ni == 0)
        err = np.abs(p - want).max() / np.abs(want).max()
        print("PMGRID %d, %d probes: mesh part max err %.2e of max|pot|" % (pmgrid, k, err))
        assert err <= 1e-10
    # (b) 8 rows on a lattice of spacing L / 2 (jittered): 6 Asmth is 0.47 L at PMGRID 16
    g = np.array([(i, j, k) for i in range(2) for j in range(2) for k in range(2)], dtype=np.float64)
    pos = (0.2 + 0.5 * g) * BOX + rng.uniform(-0.01, 0.01, (8, 3)) * BOX
    mass, typ = rng.uniform(0.5, 2.0, 8), np.arange(8, dtype=np.int32) % 6
    _load(eng, pos, mass, typ)
    pot, ni = eng.compute_potential(want_nint=True)
    assert np.all(ni == 1)
    E0 = R.e_table(pkg, cfg)[0, 0, 0]
    asmth = 1.25 * BOX / pmgrid
    own = cfg.G * mass * E0 / (2 * np.pi * asmth)             # (the self term cancels -2.8 m / h exactly)
    want = R.mesh_potential(cfg, pos, mass, typ)
    err = np.abs(pot - own - want).max() / np.abs(want).max()
    print("PMGRID %d, own rows: mesh part max err %.2e of max|pot|" % (pmgrid, err))
    assert err <= 1e-10
    eng.close()


# ---- 6. split additivity ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_set_split_over_two_engines_adds_up(pkg):
    n = 1037
    pos, mass, typ, eps = R.particle_set(n, 51)
    cfg, eng = _engine(pkg, eps, "cross")
    _load(eng, pos, mass, typ)
    half = np.arange(n) % 2 == 0
    total = np.zeros(n)
    for sel in (half, ~half):
        _, e = _engine(pkg, eps, "cross")
        _load(e, pos[sel], mass[sel], typ[sel])
        total += e.potential_targets(pos, typ, mass=mass)
        e.close()
    terms = R.pair_terms(cfg, pos, mass, typ)
    own = np.diag(terms)                                       # the row's own pair term: -2.8 m / h
    bound = 1e-12 * cfg.G * np.abs(terms).sum(1)
    single = eng.potential_targets(pos, typ, mass=mass)        # the single engine's walk part, x G
    assert np.all(np.abs((total - cfg.G * own) - (single - cfg.G * own)) <= bound)
    assert np.all(np.abs((total - cfg.G * own) - cfg.G * (terms.sum(1) - own)) <= bound)
    eng.close()


# ---- 7. tail ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("case", ["comoving_periodic", "comoving_open", "lambda_only"])
def test_tail_against_the_restatement(pkg, case):
    periodic = case == "comoving_periodic"
    n = 65
    pos, mass, typ, eps = R.particle_set(n, 61, box=BOX if periodic else None)
    cfg, eng = _engine(pkg, eps, "cross", G=1.0, periodic=int(periodic))
    _load(eng, pos, mass, typ)
    par = pkg.abi.make_time_params(comoving=int(case != "lambda_only"), omega0=0.3, omega_lambda=0.7, hubble=0.1)
    walk = eng.potential_targets(pos, typ, mass=mass) / cfg.G
    pot, plain = eng.compute_potential(par), eng.compute_potential()
    want = R.tail(cfg, par, pos, mass, typ, walk)
    err = np.abs(pot - want).max() / np.abs(want).max()
    print("%s: max err %.2e; the tail moves the column by %.2e of it" % (case, err, np.abs(pot - plain).max() / np.abs(want).max()))
    assert err <= 1e-12
    assert np.abs(pot - plain).max() > 1e-6 * np.abs(want).max()     # the case's term is there at all
    eng.close()


# ---- 8. refusals -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_unsupported_configurations_are_refused(pkg):
    A = pkg.abi
    n = 65
    pos, mass, typ, eps = R.particle_set(n, 71)

    def refused(eng, word, status="status -1"):
        out = np.full(n, -3.25)
        with pytest.raises(pkg.NgravsError, match=status) as e:
            eng.compute_potential(into=out)
        assert word in str(e.value), (word, str(e.value))
        with pytest.raises(pkg.NgravsError, match=status) as e:
            eng.potential_targets(pos[:5], typ[:5])
        assert word in str(e.value), (word, str(e.value))
        assert np.all(out == -3.25)

    def newton(t, s, r2, r, N):
        return s / r2

    def plummer(t, s, h, r, N):
        hi = 1.0 / h
        u = r * hi
        if u < 0.5:
            return s * hi ** 3 * (10.666666666667 + u * u * (32.0 * u - 38.4))
        return s * hi ** 3 * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u ** 3 - 0.066666666667 / u ** 3)

    cases = [(dict(wiring="coloyuk", periodic=1, box_size=BOX), None, "no wired potential companion"),
             (dict(wiring="yukawa_offdiag", periodic=1, box_size=BOX), None, "no wired potential companion"),
             (dict(wiring="bam"), None, "no wired potential companion"),
             (dict(wiring={"accel": [[A.LAW_USER0] * 2] * 2, "spline": [[A.SPLINE_USER0 + 1] * 2] * 2}),
              [(A.USER_ACCEL, newton), (A.USER_SPLINE, plummer)], "no wired potential companion"),
             (dict(wiring="newton", world_size=2), None, "single task only")]
    for kw, fns, word in cases:
        cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.5, softening=eps, type_to_grav=T2G, walk_mode=pkg.WALK_STRICT, **kw)
        eng = pkg.Engine(cfg, user_fns=fns)
        eng.set_particles(pos, mass, typ)
        refused(eng, word)
        eng.close()
    # adaptive gas softening; and no tree: NGRAVS_ERR_STATE
    cfg, eng = _engine(pkg, eps, theta=0.5)
    eng.set_particles(pos, mass, typ)
    refused(eng, "built tree", "status -4")
    eng.domain_Decomposition()
    eng.force_treebuild()
    eng.set_gas_softening(np.where(typ == 0, 0.05, 0.0))
    refused(eng, "adaptive gas softening")
    eng.set_gas_softening(None)
    assert np.all(np.isfinite(eng.compute_potential()))
    eng.close()
    # a mesh without periodic boundaries does not get as far as a context
    with pytest.raises(pkg.NgravsError, match="non-periodic PM"):
        pkg.Engine(pkg.make_config(n_gravs=2, pmgrid=16, box_size=BOX, softening=eps, type_to_grav=T2G))


# ---- 9. consumers ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timeline_stations_take_the_device_potential(pkg, tmp_path):
    import torch
    import test_time_integration as T
    n = 65
    pos, mass, typ, eps = R.particle_set(n, 81)
    typ = np.where(typ == 0, 1, typ).astype(np.int32)          # no gas
    vel = np.random.default_rng(82).normal(size=(n, 3)) * 0.05
    # gravity so weak that every row takes max_size_timestep: the sync points are the multiples of 0.25
    cfg = pkg.make_config(n_gravs=2, G=1e-8, softening=eps, theta=1e-6, type_to_grav=T2G, wiring=_wiring(pkg, "cross"))
    eng = pkg.Engine(cfg)
    P = T.params(False, time_max=8.0, timebase_interval=8.0 / T.TB, max_size_timestep=0.25, min_size_timestep=0.0)
    host = dict(type=typ, pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    cols = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    seen = {"statistics": [], "snapshot": []}

    def on_station(name, tl):
        if name in seen:
            seen[name].append(tl.cols["pos"].cpu().numpy().copy())
    rule = pkg.abi.make_output_rule(time_of_first_snapshot=0.3, time_bet_snapshot=0.6)       # between sync points
    out = dict(dir=str(tmp_path) + os.sep, base="snap", snap_format=2, rule=rule, blocks_mask=pkg.abi.snap_mask("POT"), ids=lambda tl: ids)
    par = T.c_params(pkg, P)               # not comoving, OmegaLambda = 0.7: the tail's -0.5 OmegaLambda H^2 r^2 is part of the column
    tl = pkg.timeline.Timeline(eng, cols, par, on_station=on_station, time_bet_statistics=0, potential="device", output=out)
    states = []
    for _ in range(4):
        tl.step()
        states.append(tl.sys_state.EnergyPot)
    assert len(seen["statistics"]) == 4 and len(seen["snapshot"]) >= 1
    for p_at, e_pot in zip(seen["statistics"], states):
        want = R.tail(cfg, par, p_at, mass, typ, R.pair_terms(cfg, p_at, mass, typ).sum(1))
        e_want = (0.5 * mass * want).sum()                     # a = 1
        assert abs(e_pot - e_want) <= 1e-12 * np.abs(0.5 * mass * want).sum()
    for k, p_at in enumerate(seen["snapshot"]):
        _, blocks = pkg.snapshot.read_blocks(str(tmp_path / ("snap_%03d" % k)))
        want = R.tail(cfg, par, p_at, mass, typ, R.pair_terms(cfg, p_at, mass, typ).sum(1))
        order = np.argsort(typ, kind="stable")                 # the file order: type by type
        got = np.asarray(blocks["POT"]).ravel()
        assert got.dtype == np.float32
        assert np.all(np.abs(got - want[order].astype(np.float32)) <= np.spacing(np.abs(want[order]).astype(np.float32)))
    # the last snapshot of a run (run.c:136): float32 of the very column the station computed
    path = tl.write_snapshot()
    _, blocks = pkg.snapshot.read_blocks(path)
    assert np.array_equal(np.asarray(blocks["POT"]).ravel(), tl.potential_column.cpu().numpy()[order].astype(np.float32))
    eng.close()
