"""Adaptive gravitational softening for gas (the reference's ADAPTIVE_GRAVSOFT_FORGAS): ngravs_set_gas_softening through the strict
walk, the direct sum, the group walk, the kept tree and the glue.

The oracle has no adaptive softening.  tests/adaptive_ref.py restates the reference's walk in Python; the CPU tests here pin it to
the oracle with adaptive=False (forces to 1e-12 of the largest force, interaction counts equal) and, with adaptive=True and an
opening angle of 1e-6, to the plain double loop with h = max(soft_i, soft_j); the GPU tests then hold the engine to it.

Input sets (counters of the restatement over the sampled targets, A = node visits opened by the softening rule alone, B = pair
interactions with r < h where h is a gas length; the builders assert A >= 100 and B >= 100 on (a) and (b), and A >= 1 for every
star inside H on (c)):
  (a) Plummer sphere, 2000 gas + 500 type 1 + 500 type 2, N_GRAVS 2, theta 0.5:   A = 19562, B = 51301 over 300 targets
  (b) the same mix uniform in a periodic box, tree-only, theta 0.5:              A = 9757,  B = 36036 over 300 targets
      ... TreePM, PMGRID 16:                                                     A = 9757,  B = 36036
  (c) the fat clump, 8 gas particles of length H = 0.2 in a cell of side 0.004 and 200 stars around them: A >= 1 for each of
      the 130 stars inside H (A = 775 over all 208 targets), B = 1967
On (b) the gas lengths (0.08 .. 0.3 of the box) are comparable with the TreePM cut of a 16^3 mesh (0.35): both walks are far from
the periodic direct sum there (rms 0.7 / 0.5 of the nearly cancelling total force), which the bound of test 5 allows for.
"""
import functools
import os
import subprocess

import numpy as np
import pytest

import adaptive_ref as R

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
SOFT = [0.02, 0.01, 0.03, 0.01, 0.01, 0.01]      # Plummer-equivalent lengths per type (types 1 / 2: 0.01 / 0.03)
T2G = [0, 0, 1, 0, 0, 0]                         # gas and type 1 are species 0, type 2 is species 1
NSAMPLE = 300


class Case:
    """one input set: particles, gas lengths, the sampled targets, the configuration keywords"""

    def __init__(self, name, pos, mass, typ, hsml, kw, idx):
        self.name, self.pos, self.mass, self.typ, self.hsml, self.kw, self.idx = name, pos, mass, typ, hsml, kw, idx
        self.n = len(pos)


def _full_hsml(typ, pos, rng, box=0.0):
    h = np.zeros(len(pos))
    gas = typ == 0
    h[gas] = R.gas_lengths(pos[gas], rng, box)
    return h


@functools.lru_cache(maxsize=None)
def case(pkg_ic, name):
    rng = np.random.default_rng({"a": 301, "b": 302, "c": 303}[name])
    if name == "a":
        pos, mass, _ = pkg_ic.plummer_sphere(3000, seed=21)
        typ = R.mixed_types(2000, 500, 500, rng)
        kw = dict(n_gravs=2, softening=SOFT, type_to_grav=T2G, wiring="newton")
        hsml = _full_hsml(typ, pos, rng)
    elif name == "b":
        pos = rng.random((3000, 3))
        mass = np.full(3000, 1.0 / 3000)
        typ = R.mixed_types(2000, 500, 500, rng)
        kw = dict(n_gravs=2, softening=SOFT, type_to_grav=T2G, periodic=1, box_size=1.0)
        hsml = _full_hsml(typ, pos, rng, box=1.0)
    else:
        # eight gas particles inside one cell of side l = 0.004 with a length H = 0.2 >> l; 200 stars around them at distances
        # 0.03 .. 0.6 (log-uniform): for theta = 0.5 the clump's cell is far enough (l / d < theta) from every one of them, so
        # for a star inside H only the maxsoft rule opens it
        ell, H = 0.004, 0.2
        c0 = np.array([0.137, 0.211, 0.093])
        gas = c0 + ell * (0.1 + 0.8 * rng.random((8, 3)))
        d = 0.03 * (0.6 / 0.03) ** rng.random(200)
        u = rng.normal(size=(200, 3))
        stars = c0 + 0.5 * ell + d[:, None] * u / np.linalg.norm(u, axis=1)[:, None]
        pos = np.concatenate([gas, stars])
        mass = np.concatenate([np.full(8, 1.0), np.full(200, 0.01)])
        typ = np.concatenate([np.zeros(8), np.ones(200)]).astype(np.int32)
        kw = dict(n_gravs=1, softening=[0.001] * 6, wiring="newton")
        hsml = np.where(typ == 0, H, 0.0)
    n = len(pos)
    idx = np.arange(n, dtype=np.int32) if n <= NSAMPLE else np.sort(rng.choice(n, NSAMPLE, replace=False)).astype(np.int32)
    return Case(name, pos, mass, typ, hsml, kw, idx)


def config(pkg, cs, regime, **more):
    """regime: 'open' (tree-only as the set is), 'periodic' (tree-only with the lattice), 'treepm' (PMGRID 16)"""
    kw = dict(G=1.0, theta=0.5, err_tol_force_acc=0.005, walk_mode=pkg.WALK_STRICT)
    kw.update(cs.kw)
    if regime == "treepm":
        kw.update(pmgrid=16, wiring="c4")
    elif regime == "periodic":
        kw.update(wiring="newton")
    else:
        assert not kw.get("periodic")
    kw.update(more)
    return pkg.make_config(**kw)


@functools.lru_cache(maxsize=None)
def restated(pkg, O, name, regime, theta, adaptive=True, old_key=None):
    """the restatement's forces (with the oracle's lattice walk in the periodic tree-only regime), counts and counters for the
    sampled targets; computed once per case and shared"""
    cs = case(pkg.ic, name)
    cfg = config(pkg, cs, regime)
    cfg.err_tol_theta = theta
    old = _OLD.get(old_key)
    dom = O.domain_extent(cs.pos)
    T = R.Tree(cfg, cs.pos, cs.mass, cs.typ, dom, hsml=cs.hsml)
    tab = O.shortrange_table(cfg)[0] if cfg.pmgrid else None
    acc, nint, A, B = T.walk(idx=cs.idx, old_acc=old, table=tab, adaptive=adaptive)
    if regime == "periodic":
        OT = O.Tree(cfg, cs.pos, cs.mass, cs.typ, dom)
        n32 = nint.astype(np.int32)
        O.lattice_walk(OT, acc, n32, O.lattice_tables(cfg), old_acc=old, idx=cs.idx)
        nint = n32.astype(np.int64)
        OT.close()
    return acc, nint, A, B


_OLD = {}   # OldAcc columns of the relative-criterion cases, by key (lru_cache wants hashable arguments)


# ==== CPU: the restatement is the oracle's walk, then the double loop ==================================================================
@pytest.mark.parametrize("name,regime", [("a", "open"), ("c", "open"), ("b", "periodic"), ("b", "treepm")])
@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_restatement_is_the_oracle_walk(pkg, O, name, regime, theta):
    """adaptive=False: forces to 1e-12 of the largest force and equal interaction counts, theta = 0.5 and the relative criterion,
    tree-only and TreePM with the oracle's table: pins the restatement's tree (top-tree nodes included) before its adaptive branch
    is trusted"""
    cs = case(pkg.ic, name)
    cfg = config(pkg, cs, regime)
    cfg.err_tol_theta = theta
    old = None if theta else np.abs(np.sin(1.0 + np.arange(cs.n))) * (50.0 if name == "c" else 1.0) + 0.1
    dom = O.domain_extent(cs.pos)
    tab = O.shortrange_table(cfg)[0] if cfg.pmgrid else None
    OT = O.Tree(cfg, cs.pos, cs.mass, cs.typ, dom)
    a_o, n_o = OT.walk(old_acc=old, idx=cs.idx, table=tab)
    T = R.Tree(cfg, cs.pos, cs.mass, cs.typ, dom)
    assert len(T.nodes) == OT.numnodes
    a_r, n_r, _, _ = T.walk(idx=cs.idx, old_acc=old, table=tab, adaptive=False)
    assert np.array_equal(n_r, n_o.astype(np.int64))
    assert np.abs(a_r - a_o).max() <= 1e-12 * np.abs(a_o).max()
    OT.close()


@pytest.mark.parametrize("name,regime", [("a", "open"), ("b", "periodic"), ("c", "open")])
def test_restatement_opened_everywhere_is_the_double_loop(pkg, O, name, regime):
    """adaptive=True with theta = 1e-6: every node is opened, what is left is the pair rule h = max(soft_i, soft_j)"""
    cs = case(pkg.ic, name)
    cfg = config(pkg, cs, regime)
    cfg.err_tol_theta = 1e-6
    idx = cs.idx[:40]
    T = R.Tree(cfg, cs.pos, cs.mass, cs.typ, O.domain_extent(cs.pos), hsml=cs.hsml)
    acc, nint, _, _ = T.walk(idx=idx, adaptive=True)
    assert np.all(nint == cs.n)
    ref = R.direct(cfg, cs.pos, cs.mass, cs.typ, T.soft, idx)
    assert np.abs(acc - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("name,regime", [("a", "open"), ("b", "periodic"), ("b", "treepm"), ("c", "open")])
def test_inputs_exercise_the_adaptive_rules(pkg, O, name, regime):
    """the conditions on the input sets: both adaptive rules fire often on (a) and (b); on (c) every star inside H has a node
    opened by the maxsoft rule"""
    cs = case(pkg.ic, name)
    _, _, A, B = restated(pkg, O, name, regime, 0.5)
    print("set (%s) %s: A = %d, B = %d over %d targets" % (name, regime, A.sum(), B.sum(), len(cs.idx)))
    if name == "c":
        d = np.linalg.norm(cs.pos - cs.pos[:8].mean(axis=0), axis=1)
        inside = (cs.typ == 1) & (d < 0.2 - 0.004)
        assert inside.sum() >= 50 and np.all(A[inside] >= 1)
        # ... and the plain rule does not open them: the forces differ
        a_p = restated(pkg, O, name, regime, 0.5, adaptive=False)[0]
        a_a = restated(pkg, O, name, regime, 0.5)[0]
        assert np.abs(a_a - a_p)[inside].max() > 1e-3 * np.abs(a_p).max()
    else:
        assert A.sum() >= 100 and B.sum() >= 100


def test_header_exports_and_bindings_agree(pkg):
    hdr = open(os.path.join(ROOT, "include", "ngravs_hip.h")).read()
    assert "int ngravs_set_gas_softening(ngravs_ctx *ctx, const double *hsml, int64_t stride, int on_device);" in hdr
    assert "ngravs_set_gas_softening" in pkg.EXPORTS and hasattr(pkg.Engine, "set_gas_softening")
    assert "NGRAVS_KERNEL_STRICT_ADAPTIVE = %d" % pkg.abi.KERNEL_STRICT_ADAPTIVE in hdr
    assert "NGRAVS_KERNEL_GROUP_ADAPTIVE = %d" % pkg.abi.KERNEL_GROUP_ADAPTIVE in hdr
    assert "#define NGRAVS_ABI_VERSION 3" in hdr and pkg.abi.ABI_VERSION == 3


def test_library_exports_the_call(pkg, have_lib):
    assert hasattr(have_lib, "ngravs_set_gas_softening")


GLUE_DEFS = ["-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION", "-DUNEQUALSOFTENINGS"]
SPH_OPTION_SETS = [[], ["-DPERIODIC"], ["-DPERIODIC", "-DPMGRID=64"], ["-DPERIODIC", "-DISOTHERM_EQS"], ["-DPERIODIC", "-DNOVISCOSITYLIMITER"]]


def _glue(pkg):
    return os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")


def _includes():
    return ["-I" + os.path.join(ROOT, "tests", "glue_stub_sph"), "-I" + os.path.join(ROOT, "tests", "glue_stub"), "-I" + os.path.join(ROOT, "include")]


@pytest.mark.parametrize("flags", SPH_OPTION_SETS)
@pytest.mark.parametrize("sph", [[], ["-DNGRAVS_GLUE_SPH"]])
def test_glue_compiles_with_the_switch(pkg, flags, sph, tmp_path):
    """-Wall -Wextra -Werror with -DADAPTIVE_GRAVSOFT_FORGAS over the option sets of the SPH glue tests, with and without
    -DNGRAVS_GLUE_SPH: the object refers to ngravs_set_gas_softening; without the define it does not"""
    obj = str(tmp_path / "gadget_glue.o")
    base = ["gcc", "-c", "-O0", "-Wall", "-Wextra", "-Werror"] + GLUE_DEFS + _includes() + flags + sph
    for define, want in ((["-DADAPTIVE_GRAVSOFT_FORGAS"], True), ([], False)):
        out = subprocess.run(base + define + [_glue(pkg), "-o", obj], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        und = {ln.split()[-1] for ln in subprocess.run(["nm", "-u", obj], capture_output=True, text=True, check=True).stdout.splitlines()}
        assert ("ngravs_set_gas_softening" in und) == want


# ==== GPU ==============================================================================================================================
def _engine(pkg, cfg, cs, hsml="case", tuning=None, **kw):
    eng = pkg.Engine(cfg)
    if tuning:
        eng.set_tuning(**tuning)
    eng.set_particles(cs.pos, cs.mass, cs.typ, **kw)
    if hsml is not None:
        eng.set_gas_softening(cs.hsml if isinstance(hsml, str) else hsml)
    return eng


def _old_acc(pkg, cs, regime):
    """OldAcc for the relative criterion: what a theta pass of the adaptive strict walk leaves (once per case and regime)"""
    key = (cs.name, regime)
    if key not in _OLD:
        eng = _engine(pkg, config(pkg, cs, regime), cs)
        eng.compute_accelerations(pm_step=regime == "treepm")
        _OLD[key] = eng.get_accel()[1]
        eng.close()
    return key


STRICT_CASES = [("a", "open", 0.5), ("a", "open", 0.0), ("c", "open", 0.5), ("c", "open", 0.0), ("b", "periodic", 0.5),
                ("b", "treepm", 0.5), ("b", "treepm", 0.0)]


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime,theta", STRICT_CASES)
def test_strict_walk_is_the_reference_rule(pkg, O, name, regime, theta):
    """1. the adaptive strict walk against the restatement on the three sets, tree-only open (theta 0.5 and the relative criterion),
    tree-only periodic with the lattice, TreePM: forces to 1e-10 of the largest force, equal interaction counts (the strict walk's
    terms), and the kernel that ran"""
    cs = case(pkg.ic, name)
    old_key = None if theta else _old_acc(pkg, cs, regime)
    cfg = config(pkg, cs, regime)
    cfg.err_tol_theta = theta
    eng = _engine(pkg, cfg, cs, old_acc=_OLD.get(old_key))
    eng.compute_accelerations(pm_step=regime == "treepm")
    acc, _, cost = eng.get_accel()
    kern = eng.last_walk_kernel()
    eng.close()
    a_r, n_r, A, B = restated(pkg, O, name, regime, theta, True, old_key)
    err = np.abs(acc[cs.idx] / cfg.G - a_r).max() / np.abs(a_r).max()
    print("adaptive strict walk, set (%s) %s theta %g: max force diff %.1e, %.1f interactions per target, A = %d, B = %d"
          % (name, regime, theta, err, n_r.mean(), A.sum(), B.sum()))
    assert kern == pkg.abi.KERNEL_STRICT_ADAPTIVE
    assert np.array_equal(cost[cs.idx].astype(np.int64), n_r)
    assert err < 1e-10


@pytest.mark.gpu
@pytest.mark.parametrize("regime", ["open", "treepm"])
def test_degenerate_lengths_give_the_plain_strict_walk(pkg, regime):
    """2. an all-gas set with hsml = force_softening[0] everywhere: the adaptive strict walk is the plain one, 1e-13, equal counts"""
    n = 3000
    rng = np.random.default_rng(44)
    if regime == "open":
        pos, mass, _ = pkg.ic.plummer_sphere(n, seed=45)
        kw = {}
    else:
        pos, mass = rng.random((n, 3)), np.full(n, 1.0 / n)
        kw = dict(periodic=1, box_size=1.0, pmgrid=16)
    typ = np.zeros(n, dtype=np.int32)
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.02] * 6, walk_mode=pkg.WALK_STRICT, **kw)
    out = {}
    for ada in (0, 1):
        eng = pkg.Engine(cfg)
        eng.set_particles(pos, mass, typ)
        if ada:
            eng.set_gas_softening(np.full(n, cfg.force_softening[0]))
        eng.compute_accelerations(pm_step=bool(kw))
        out[ada] = eng.get_accel() + (eng.last_walk_kernel(),)
        eng.close()
    assert out[0][3] == pkg.abi.KERNEL_STRICT and out[1][3] == pkg.abi.KERNEL_STRICT_ADAPTIVE
    assert np.array_equal(out[0][2], out[1][2])
    assert np.abs(out[1][0] - out[0][0]).max() <= 1e-13 * np.abs(out[0][0]).max()


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime", [("a", "open"), ("c", "open"), ("b", "periodic")])
def test_direct_sum_uses_the_pair_rule(pkg, O, name, regime):
    """3. direct_sum(idx) in adaptive mode, open and periodic (with the oracle's lattice tables), against the numpy double loop"""
    cs = case(pkg.ic, name)
    cfg = config(pkg, cs, regime)
    eng = _engine(pkg, cfg, cs)
    eng.domain_Decomposition()
    d = eng.direct_sum(cs.idx)
    eng.set_gas_softening(None)
    d_plain = eng.direct_sum(cs.idx)
    eng.close()
    soft = R.particle_soft(cfg, cs.typ, cs.hsml)
    ref = R.direct(cfg, cs.pos, cs.mass, cs.typ, soft, cs.idx, lat=O.lattice_tables(cfg) if cfg.periodic else None)
    err = np.abs(d - ref).max() / np.abs(ref).max()
    print("adaptive direct sum, set (%s) %s: max diff %.1e" % (name, regime, err))
    assert err < 1e-11
    assert np.abs(d - d_plain).max() > 1e-3 * np.abs(ref).max()      # the lengths matter on these sets


GROUP_TUNING = {"walk_spread": 64, "walk_nleaf": 0, "walk_root": 1, "walk_sg": 1}


@pytest.mark.gpu
@pytest.mark.parametrize("fused", [0, 1])
@pytest.mark.parametrize("name,regime", [("a", "open"), ("c", "open"), ("b", "treepm")])
def test_group_walk_kernels_take_the_reference_interactions(pkg, O, name, regime, fused):
    """4. the group-walk kernels with one target per wave (the tuning of test_group_walk_kernels_reproduce_the_reference_set_tree_only),
    30 % of the rows active, split and fused: forces to 1e-11 of the restatement's, cost >= its count, and the kernel that ran"""
    cs = case(pkg.ic, name)
    cfg = config(pkg, cs, regime, walk_mode=pkg.WALK_GROUP, group_reach=6.0)
    sub = cs.idx[np.random.default_rng(6).uniform(size=len(cs.idx)) < 0.3]
    active = (np.random.default_rng(7).uniform(size=cs.n) < 0.3).astype(np.uint8)
    active[cs.idx] = 0
    active[sub] = 1                                  # of the sampled targets exactly `sub` are active
    assert 0.2 < active.mean() < 0.4 and len(sub) >= 50
    eng = _engine(pkg, cfg, cs, active=active, tuning=dict(GROUP_TUNING, walk_fused=fused))
    eng.compute_accelerations(pm_step=regime == "treepm")
    acc, _, cost = eng.get_accel()
    kern = eng.last_walk_kernel()
    eng.close()
    a_r, n_r, _, _ = restated(pkg, O, name, regime, 0.5)
    pick = np.isin(cs.idx, sub)
    err = np.abs(acc[sub] / cfg.G - a_r[pick]).max() / np.abs(a_r).max()
    print("adaptive group-walk kernels (%s), set (%s) %s: max force diff %.1e; %.1f (restatement %.1f) interactions"
          % ("fused" if fused else "split", name, regime, err, cost[sub].mean(), n_r[pick].mean()))
    assert kern == pkg.abi.KERNEL_GROUP_ADAPTIVE
    assert np.all(cost[sub] >= n_r[pick]) and np.all(acc[active == 0] == 0)
    assert err < 1e-11


@pytest.mark.gpu
@pytest.mark.parametrize("name,regime", [("a", "open"), ("b", "treepm")])
def test_production_group_walk_is_as_accurate_as_the_strict_walk(pkg, name, regime):
    """5. nothing tuned: the group walk against the adaptive direct sum, rms no worse than 1.05 x the strict walk's + 1e-3 (the bound
    of test_group_walk_unequal_softenings)"""
    cs = case(pkg.ic, name)
    pm = regime == "treepm"
    res = {}
    for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
        eng = _engine(pkg, config(pkg, cs, regime, walk_mode=mode), cs)
        eng.compute_accelerations(pm_step=pm)
        out = eng.get_accel(want_pm=pm)
        truth = eng.direct_sum(cs.idx)
        res[mode] = (out[0] + (out[3] if pm else 0.0), truth, eng.last_walk_kernel(), out[2])
        eng.close()
    assert res[pkg.WALK_GROUP][2] == pkg.abi.KERNEL_GROUP_ADAPTIVE
    rel = lambda a, b: np.linalg.norm(a - b, axis=1) / np.linalg.norm(b, axis=1)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    e_s = rms(rel(res[pkg.WALK_STRICT][0][cs.idx], res[pkg.WALK_STRICT][1]))
    e_g = rms(rel(res[pkg.WALK_GROUP][0][cs.idx], res[pkg.WALK_GROUP][1]))
    print("adaptive production walk, set (%s) %s: strict rms %.2e, group rms %.2e against the adaptive direct sum; ia %.0f / %.0f"
          % (name, regime, e_s, e_g, res[pkg.WALK_STRICT][3].mean(), res[pkg.WALK_GROUP][3].mean()))
    assert e_g <= 1.05 * e_s + 1e-3


@pytest.mark.gpu
def test_kept_tree_sees_new_lengths_and_their_removal(pkg):
    """6. update_particles with unchanged positions, then every length doubled: the kept tree's node lengths are refreshed (a fresh
    engine with the doubled lengths, 1e-13, equal counts); then set_gas_softening(None): bitwise the forces of an engine that
    never had lengths"""
    cs = case(pkg.ic, "a")
    cfg = config(pkg, cs, "open")

    def sequence(first, second):
        eng = _engine(pkg, cfg, cs, hsml=first)
        eng.compute_accelerations(pm_step=False)
        eng.update_particles(cs.pos, cs.mass, cs.typ)
        if second is not None:
            eng.set_gas_softening(second)
        eng.gravity_tree()
        return eng, eng.get_accel()

    eng, (acc2, _, cost2) = sequence(cs.hsml, 2 * cs.hsml)
    fresh = _engine(pkg, cfg, cs, hsml=2 * cs.hsml)
    fresh.compute_accelerations(pm_step=False)
    acc_f, _, cost_f = fresh.get_accel()
    fresh.close()
    assert np.array_equal(cost2, cost_f)
    assert np.abs(acc2 - acc_f).max() <= 1e-13 * np.abs(acc_f).max()
    eng.set_gas_softening(None)
    eng.gravity_tree()
    acc0, _, cost0 = eng.get_accel()
    assert eng.last_walk_kernel() == pkg.abi.KERNEL_STRICT
    eng.close()
    never, (acc_n, _, cost_n) = sequence(None, None)
    never.close()
    assert np.array_equal(acc0, acc_n) and np.array_equal(cost0, cost_n)
    assert np.abs(acc2 - acc0).max() > 1e-3 * np.abs(acc0).max()


@pytest.mark.gpu
def test_device_tensor_is_the_host_column(pkg):
    """Engine.set_gas_softening with a device tensor (read in place, type-0 rows only) gives bitwise the host column's forces"""
    import torch
    cs = case(pkg.ic, "a")
    cfg = config(pkg, cs, "open")
    out = []
    for dev in (False, True):
        col = cs.hsml.copy()
        col[cs.typ != 0] = np.nan                    # never read
        eng = _engine(pkg, cfg, cs, hsml=torch.from_numpy(col).cuda() if dev else col)
        eng.compute_accelerations(pm_step=False)
        out.append(eng.get_accel())
        eng.close()
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][2], out[1][2])


@pytest.mark.gpu
def test_refusals_change_nothing(pkg, have_lib):
    """7. every refusal of ngravs_set_gas_softening: status, message, and the state after it; sph_density is not touched by the mode"""
    import ctypes as C
    L = have_lib
    ARG, STATE = -1, -4
    cs = case(pkg.ic, "a")
    cfg = config(pkg, cs, "open")
    h = np.ascontiguousarray(cs.hsml)

    def call(eng, col):
        rc = L.ngravs_set_gas_softening(eng._h, col.ctypes.data if col is not None else None, 8, 0)
        return rc, L.ngravs_last_error(eng._h).decode()

    # no particles yet
    eng = pkg.Engine(cfg)
    rc, msg = call(eng, h)
    assert rc == ARG and "no particles" in msg
    eng.set_particles(cs.pos, cs.mass, cs.typ)
    eng.compute_accelerations(pm_step=False)
    plain = eng.get_accel()[0]
    # a negative and a non-finite value on type-0 rows are refused, and the context stays without lengths; on other rows they are not read
    gas = np.nonzero(cs.typ == 0)[0]
    for bad in (-1.0, np.nan, np.inf):
        col = h.copy()
        col[gas[5]] = bad
        rc, msg = call(eng, col)
        assert rc == ARG and "type-0 rows" in msg
        eng.gravity_tree()
        assert eng.last_walk_kernel() == pkg.abi.KERNEL_STRICT and np.array_equal(eng.get_accel()[0], plain)
    col = h.copy()
    col[cs.typ != 0] = np.nan
    assert call(eng, col)[0] == 0
    eng.gravity_tree()
    ada = eng.get_accel()[0]
    assert eng.last_walk_kernel() == pkg.abi.KERNEL_STRICT_ADAPTIVE and not np.array_equal(ada, plain)
    # ... and a refused call leaves the lengths that were there
    col = h.copy()
    col[gas[0]] = -2.0
    assert call(eng, col)[0] == ARG
    eng.gravity_tree()
    assert np.array_equal(eng.get_accel()[0], ada)
    # explicit targets have no length
    acc = np.zeros((2, 3))
    rc = L.ngravs_direct_sum_targets(eng._h, cs.pos[:2].ctypes.data, None, cs.typ[:2].ctypes.data, 2, acc.ctypes.data)
    assert rc == STATE and "carry no softening length" in L.ngravs_last_error(eng._h).decode()
    # ngravs_set_softening changes the other types' lengths: the node lengths follow
    fs = np.array([cfg.force_softening[t] for t in range(6)])
    eng.set_softening(fs * 40.0)
    eng.gravity_tree()
    big = eng.get_accel()
    eng.close()
    cfg_big = config(pkg, cs, "open", softening=[40.0 * s for s in SOFT])
    fresh = _engine(pkg, cfg_big, cs)
    fresh.compute_accelerations(pm_step=False)
    want = fresh.get_accel()
    # sph_density is the same call with and without the mode
    vel = np.zeros((cs.n, 3))
    d_on = fresh.sph_density(vel, cs.hsml, 32.0, 2.0)
    fresh.set_gas_softening(None)
    d_off = fresh.sph_density(vel, cs.hsml, 32.0, 2.0)
    fresh.close()
    assert np.array_equal(big[2], want[2]) and np.abs(big[0] - want[0]).max() <= 1e-13 * np.abs(want[0]).max()
    for k in ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor"):
        assert np.array_equal(d_on[k], d_off[k]), k
    # several tasks
    cfg2 = config(pkg, cs, "open", world_size=2)
    eng = pkg.Engine(cfg2)
    eng.set_particles(cs.pos, cs.mass, cs.typ)
    rc, msg = call(eng, h)
    eng.close()
    assert rc == STATE and "single task only" in msg
    # user-defined laws
    law = pkg.abi.GravityFn(lambda t, s, r2, r, n: s / r2)
    spl = pkg.abi.GravityFn(lambda t, s, hh, r, n: s / (hh * hh * hh))
    cfgu = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6,
                           wiring={"accel": [[pkg.abi.LAW_USER0]], "spline": [[pkg.abi.SPLINE_USER0 + 1]]}, walk_mode=pkg.WALK_STRICT)
    eng = pkg.Engine(cfgu, user_fns=[(pkg.abi.USER_ACCEL, law), (pkg.abi.USER_SPLINE, spl)])
    eng.set_particles(cs.pos, cs.mass, np.zeros(cs.n, dtype=np.int32))
    rc, msg = call(eng, h)
    eng.close()
    assert rc == ARG and "user-defined laws" in msg
    # a group-walk configuration without an adaptive kernel is refused by the walk, which names it and the mode that serves it
    csb = case(pkg.ic, "b")
    eng = _engine(pkg, config(pkg, csb, "periodic", walk_mode=pkg.WALK_GROUP), csb)
    eng.domain_Decomposition()
    rc = L.ngravs_gravity_tree(eng._h)
    msg = L.ngravs_last_error(eng._h).decode()
    assert rc == ARG and "periodic tree-only" in msg and "NGRAVS_WALK_STRICT" in msg
    eng.set_walk_mode(pkg.WALK_STRICT)
    eng.gravity_tree()
    assert eng.last_walk_kernel() == pkg.abi.KERNEL_STRICT_ADAPTIVE
    eng.close()
    assert C.sizeof(C.c_double) == 8


# ---- 8. the glue, executed ---------------------------------------------------------------------------------------------------------
T_DRIVER = 60.0      # a driver run takes about 2 s; the limit only ends a hung child


def _driver_run(pkg, TG, kind, periodic, extra):
    """tests/glue_stub_sph/glue_sph_driver.c with the flags of test_sph_glue_runs_on_the_gpu plus `extra`, one run with the gas
    calls; -> the three stages"""
    import tempfile
    pos, mass, ptype, vel, u, soft = TG.glue_inputs(pkg, kind)
    n = len(pos)
    opts = ["-DPERIODIC", "-DPMGRID=32"] if periodic else []
    libdir = os.path.dirname(pkg.LIB_PATH)
    with tempfile.TemporaryDirectory(prefix="glue_ada_") as tmp:
        exe = os.path.join(tmp, "glue_sph_run")
        cmd = ["gcc", "-O1", "-Wall", "-Wextra", "-Werror"] + TG.GLUE_DEFS + ["-DNGRAVS_GLUE_SPH", "-DN_GRAVS=1", "-DYUKAWA_IMASS=60"] + opts + \
            extra + TG._includes() + [TG._glue(pkg), os.path.join(ROOT, "tests", "glue_stub_sph", "glue_sph_driver.c"), "-o", exe,
                                      "-L" + libdir, "-lngravs_hip", "-lm", "-lpthread", "-Wl,-rpath," + libdir]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        rows = np.column_stack([pos, mass, ptype.astype(np.float64), vel, u])
        hd = np.array([n, TG.NGAS_GLUE, 1, 1.0, TG.BOX if periodic else 0.0, 0.5, 0.005, TG.SR.DES, TG.SR.DEV, TG.SR.VISC, TG.H.KIND_TBI[kind]] + soft)
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(hd.tobytes())
            f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
        r = subprocess.run([exe, fin, fout, tmp + "/"], capture_output=True, text=True, timeout=T_DRIVER)
        assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
        return TG.read_stages(fout, n, TG.NGAS_GLUE)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", [("plummer", False), ("uniform", True)])
def test_glue_hands_the_smoothing_lengths_over(pkg, have_lib, kind, periodic):
    """8. the SPH glue driver built once more with -DADAPTIVE_GRAVSOFT_FORGAS: stage 1's gravity_tree() runs after stage 0's density()
    has set Hsml, and its GravAccel is what an Engine gives for the same particles with set_gas_softening(Hsml of stage 0), to
    1e-12 of the largest force; the build without the define differs by more than 1e-6 (relative) on a gas row"""
    import test_glue_sph as TG
    s0, s1, _ = _driver_run(pkg, TG, kind, periodic, ["-DADAPTIVE_GRAVSOFT_FORGAS"])
    p0, p1, _ = _driver_run(pkg, TG, kind, periodic, [])
    pos, mass, ptype, vel, u, soft = TG.glue_inputs(pkg, kind)
    n, ngas = len(pos), TG.NGAS_GLUE
    assert np.array_equal(s0["Hsml"], p0["Hsml"]) and np.all(s0["Hsml"] > 0)          # density() does not depend on the switch
    cfg = pkg.make_config(n_gravs=1, periodic=int(periodic), pmgrid=32 if periodic else 0, box_size=TG.BOX if periodic else 0.0, G=1.0,
                          theta=0.5, err_tol_force_acc=0.005, softening=soft, walk_mode=pkg.WALK_GROUP, tree_alloc_factor=0.8)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype, active=np.ones(n, dtype=np.uint8))
    hs = np.zeros(n)
    hs[:ngas] = s0["Hsml"]
    eng.set_gas_softening(hs)
    eng.compute_accelerations(pm_step=bool(periodic))
    acc = eng.get_accel()[0]
    kern = eng.last_walk_kernel()
    eng.close()
    ga, gp = s1["P"][:, 0:3], p1["P"][:, 0:3]
    assert kern == pkg.abi.KERNEL_GROUP_ADAPTIVE
    assert np.abs(ga - acc).max() <= 1e-12 * np.abs(acc).max()
    d = np.linalg.norm(ga - gp, axis=1)[:ngas] / np.linalg.norm(gp, axis=1)[:ngas]
    print("glue with ADAPTIVE_GRAVSOFT_FORGAS (%s): largest relative change of a gas row's GravAccel %.2e, median %.2e" % (kind, d.max(), np.median(d)))
    assert d.max() > 1e-6
