"""-m gpu: the HIP path (through the C ABI) against the oracle on the same seeded inputs.

Tolerances (fp64 path, BASELINE.json north_star):
  * Peano-Hilbert keys, domain extent, interaction counts: bit-exact / equal.
  * strict walk, PM: <= 1e-10 of the largest acceleration (summation order / exp / FFT rounding only).
  * group walk: it never uses a node the reference would have opened, so its error against direct
    summation must not exceed the reference tree's own (ErrTolForceAcc 0.005).
"""
import os

import numpy as np
import pytest

from conftest import galaxy_config, galaxy_ic, rel_err

pytestmark = pytest.mark.gpu

TOL = 1e-10


def _engine(pkg, cfg, pos, mass, typ, tuning=None, **kw):
    eng = pkg.Engine(cfg)
    if tuning:
        eng.set_tuning(**tuning)
    eng.set_particles(pos, mass, typ, **kw)
    return eng


def test_keys_and_domain_bit_exact(pkg, O):
    for seed, (gen, n) in enumerate([("uniform", 100000), ("plummer", 50000)]):
        if gen == "uniform":
            pos, mass, typ = pkg.ic.uniform_box(n, box=1e4, n_gravs=2, seed=100 + seed)
        else:
            pos, mass, typ = pkg.ic.plummer_sphere(n, seed=100 + seed)
        cfg = pkg.make_config(n_gravs=2, softening=[0.01] * 6, type_to_grav=pkg.ic.default_type_to_grav(2))
        eng = _engine(pkg, cfg, pos, mass, typ)
        eng.domain_Decomposition()
        dom = O.domain_extent(pos)
        assert np.array_equal(eng.domain(), dom)                       # DomainCorner/Center/Len/Fac exact
        k_gpu, k_orc = eng.keys(), O.keys(pos, dom)
        assert np.array_equal(k_gpu, k_orc)                            # bit-exact Peano keys
        order = eng.order()
        assert np.array_equal(np.sort(order), np.arange(n))            # a permutation
        assert np.all(np.diff(k_gpu[order]) >= 0)                      # sorted along the curve
        # stand-alone key kernel at other bit depths
        for bits in (5, 18, 21):
            fac = dom[7] * 2.0 ** (bits - 18)
            kk = eng.peano_keys(pos[:5000], dom[:3], fac, bits)
            ref = np.array([O.peano_key(int((p[0] - dom[0]) * fac), int((p[1] - dom[1]) * fac),
                                        int((p[2] - dom[2]) * fac), bits) for p in pos[:5000]])
            assert np.array_equal(kk, ref)
        eng.close()


def _strict_vs_oracle(pkg, O, cfg, pos, mass, typ, old_acc=None, pm=True):
    eng = _engine(pkg, cfg, pos, mass, typ, old_acc=old_acc)
    eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
    if cfg.pmgrid:
        acc, old, cost, gpm = eng.get_accel(want_pm=True)
    else:
        acc, old, cost = eng.get_accel()
        gpm = None
    dom = O.domain_extent(pos)
    T = O.Tree(cfg, pos, mass, typ, dom)
    tab = O.shortrange_table(cfg)[0] if cfg.pmgrid else None
    a_o, n_o = T.walk(old_acc=old_acc, table=tab)
    pm_o = O.pm_periodic(cfg, pos, mass, typ) if cfg.pmgrid else None
    a_o, old_o = O.finish(cfg, a_o, pm_o)
    return eng, (acc, old, cost, gpm), (a_o, old_o, n_o, pm_o), T


def test_strict_walk_tree_only_plummer(pkg, O):
    n = 30000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=3)
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6, walk_mode=pkg.WALK_STRICT)
    eng, (acc, old, cost, _), (a_o, old_o, n_o, _), T = _strict_vs_oracle(pkg, O, cfg, pos, mass, typ)
    scale = np.abs(a_o).max()
    assert np.abs(acc - a_o).max() / scale < TOL
    assert np.array_equal(cost.astype(np.int64), n_o)
    assert np.allclose(old, old_o, rtol=1e-9)
    # second pass with the relative criterion (accel.c:48-52)
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc2, old2, cost2 = eng.get_accel()
    cfg.err_tol_theta = 0.0
    a2, n2 = T.walk(old_acc=old_o)
    a2, _ = O.finish(cfg, a2)
    assert np.abs(acc2 - a2).max() / scale < TOL
    assert np.mean(cost2.astype(np.int64) == n2) > 0.999
    eng.close()


def test_strict_walk_galaxy_collision_reference_statistics(pkg, O, kats):
    """C1 on the GPU: the reference's own interaction counts (1178.53 / 598.546 per particle)."""
    d = galaxy_ic(pkg)
    cfg = galaxy_config(pkg, walk_mode=pkg.WALK_STRICT)
    pos, mass, typ = d["pos"], d["mass"], d["type"]
    eng, (acc, old, cost, _), (a_o, old_o, n_o, _), T = _strict_vs_oracle(pkg, O, cfg, pos, mass, typ)
    want = kats["galaxy_collision"]
    assert abs(cost.mean() - want["ia_per_part_theta05"]) < 5e-3
    assert np.array_equal(cost.astype(np.int64), n_o)
    assert np.abs(acc - a_o).max() / np.abs(a_o).max() < TOL
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc2, _, cost2 = eng.get_accel()
    assert abs(cost2.mean() - want["ia_per_part_rel0005"]) < 5e-3
    eng.close()


@pytest.mark.parametrize("wiring,ng,pmgrid,n", [("newton", 1, 32, 20000), ("c4", 2, 32, 30000), ("coloyuk", 2, 64, 40000),
                                               ("yukawa_offdiag", 2, 32, 20000), ("c4", 3, 32, 20000)])
def test_strict_treepm_and_pm(pkg, O, wiring, ng, pmgrid, n):
    L = 1e4
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=11)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_STRICT)
    eng, (acc, old, cost, gpm), (a_o, old_o, n_o, pm_o), T = _strict_vs_oracle(pkg, O, cfg, pos, mass, typ)
    assert np.abs(gpm - pm_o).max() / np.abs(pm_o).max() < TOL          # GravPM
    assert np.abs(acc - a_o).max() / np.abs(a_o).max() < TOL            # GravAccel (short-range tree)
    assert np.array_equal(cost.astype(np.int64), n_o)                   # GravCost = ninteractions
    assert np.allclose(old, old_o, rtol=1e-8)                           # OldAcc = |tree + PM/G|
    # relative-criterion pass
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc2, _, cost2 = eng.get_accel()
    cfg.err_tol_theta = 0.0
    a2, n2 = T.walk(old_acc=old_o, table=O.shortrange_table(cfg)[0])
    a2, _ = O.finish(cfg, a2, pm_o)
    assert np.abs(acc2 - a2).max() / np.abs(a2).max() < 1e-8
    assert np.mean(cost2.astype(np.int64) == n2) > 0.999
    eng.close()


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_configurations_against_the_oracle(pkg, O, seed):
    """Differential test of the reference path (decomposition, keys, tree, reference walk, PM, OldAcc) against the oracle over random
    small configurations: particle number, 1-3 species, wiring, TreePM (16-64 mesh) or tree-only, clustering, unequal softening
    lengths, opening angle; both criteria.  Identical interaction counts, forces to rounding."""
    rng = np.random.default_rng(9000 + seed)
    n = int(rng.integers(500, 20000))
    ng = int(rng.integers(1, 4))
    pm = seed % 2 == 0
    L = float(rng.choice([1.0, 1e4]))
    pos = rng.random((n, 3))
    if rng.random() < 0.6:
        k = int(n * rng.uniform(0.1, 0.8))
        pos[:k] = np.mod(rng.random(3) + rng.uniform(0.005, 0.2) * rng.standard_normal((k, 3)), 1.0)
    pos = np.clip(pos, 0.0, 1.0 - 1e-12) * L
    mass = rng.uniform(0.5, 1.5, n) / n
    typ = (1 + rng.integers(0, ng, n)).astype(np.int32) if ng > 1 else rng.integers(0, 6, n).astype(np.int32)
    eps = L / (40 * n ** (1 / 3))
    soft = [eps * float(rng.choice([1.0, 1.0, 2.5])) for _ in range(6)]
    wiring = "newton" if ng == 1 else str(rng.choice(["c4", "newton", "coloyuk", "yukawa_offdiag"] if (ng == 2 and pm) else ["c4", "newton"] if pm else ["newton"]))
    kw = dict(n_gravs=ng, G=float(rng.choice([1.0, 43007.1])), theta=float(rng.uniform(0.3, 0.8)), softening=soft,
              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_STRICT)
    if pm:
        kw.update(periodic=1, pmgrid=int(rng.choice([16, 32, 64])), box_size=L)
    cfg = pkg.make_config(**kw)
    eng, (acc, old, cost, gpm), (a_o, old_o, n_o, pm_o), T = _strict_vs_oracle(pkg, O, cfg, pos, mass, typ)
    scale = np.abs(a_o).max()
    e1 = np.abs(acc - a_o).max() / scale
    epm = np.abs(gpm - pm_o).max() / np.abs(pm_o).max() if pm else 0.0
    same1 = np.array_equal(cost.astype(np.int64), n_o)
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc2, _, cost2 = eng.get_accel()
    cfg.err_tol_theta = 0.0
    a2, n2 = T.walk(old_acc=old_o, table=O.shortrange_table(cfg)[0] if pm else None)
    a2, _ = O.finish(cfg, a2, pm_o)
    e2 = np.abs(acc2 - a2).max() / np.abs(a2).max()
    same2 = np.mean(cost2.astype(np.int64) == n2)
    eng.close()
    T.close()
    print("seed %d: n %d, N_GRAVS %d, %s, pmgrid %d, L %g, theta %.2f: theta pass |da| %.1e counts equal %s, GravPM %.1e; relative pass |da| %.1e, counts equal for %.4f"
          % (seed, n, ng, wiring, cfg.pmgrid, L, cfg.err_tol_theta if False else kw["theta"], e1, same1, epm, e2, same2))
    assert e1 < TOL and same1 and epm < TOL
    assert np.allclose(old, old_o, rtol=1e-8)
    assert e2 < 1e-8 and same2 > 0.999


@pytest.mark.parametrize("seed", list(range(8)))
def test_random_configurations_production_walk_accuracy(pkg, seed):
    """The production (group) walk against the reference walk over random small configurations (species, wiring, TreePM / tree-only,
    clustering, unequal softening lengths), both with the relative criterion, both measured against the direct sum of a sample
    (gravtree_forcetest.c's truth: tree + PM against the periodic direct sum in a box): the production walk is not less accurate
    than the reference walk on the same input."""
    rng = np.random.default_rng(4000 + seed)
    n = int(rng.integers(5000, 30000))
    ng = int(rng.integers(1, 4))
    pm = seed % 2 == 1
    L = 1.0
    pos = rng.random((n, 3))
    if rng.random() < 0.7:
        k = int(n * rng.uniform(0.1, 0.8))
        pos[:k] = np.mod(rng.random(3) + rng.uniform(0.01, 0.2) * rng.standard_normal((k, 3)), 1.0)
    pos = np.clip(pos, 0.0, 1.0 - 1e-12) * L
    mass = rng.uniform(0.5, 1.5, n) / n
    typ = (1 + rng.integers(0, ng, n)).astype(np.int32) if ng > 1 else rng.integers(0, 6, n).astype(np.int32)
    eps = L / (40 * n ** (1 / 3))
    soft = [eps * float(rng.choice([1.0, 1.0, 2.0])) for _ in range(6)]
    wiring = "newton" if (ng == 1 or not pm) else str(rng.choice(["c4", "newton"]))
    res = {}
    for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
        kw = dict(n_gravs=ng, G=1.0, theta=0.5, softening=soft, type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=mode)
        if pm:
            kw.update(periodic=1, pmgrid=int(32 if n < 15000 else 64), box_size=L)
        cfg = pkg.make_config(**kw)
        eng = _engine(pkg, cfg, pos, mass, typ)
        eng.compute_accelerations(pm_step=pm)
        _, old, _ = eng.get_accel()
        eng.set_old_acc(old)
        eng.set_opening(0.0, 0.005)
        eng.gravity_tree()
        if pm:
            a, _, c, p = eng.get_accel(want_pm=True)
        else:
            a, _, c = eng.get_accel()
            p = 0.0
        idx = np.arange(seed % 7, n, max(1, n // 600), dtype=np.int32)
        if "truth" not in res:
            res["truth"] = eng.direct_sum(idx)
        e = rel_err((a + p)[idx], res["truth"])
        res[mode] = (np.sqrt(np.mean(e ** 2)), e.max(), c.mean())
        eng.close()
    (rs, ms, cs), (rg, mg, cg) = res[pkg.WALK_STRICT], res[pkg.WALK_GROUP]
    print("seed %d: n %d, N_GRAVS %d, %s, %s: reference walk rms %.2e max %.2e (%.0f ia) | production walk rms %.2e max %.2e (%.0f ia)"
          % (seed, n, ng, wiring, "TreePM %d" % cfg.pmgrid if pm else "tree-only", rs, ms, cs, rg, mg, cg))
    assert rg <= 1.1 * rs + 1e-4 and mg <= max(2.0 * ms, 0.03)


def test_group_walk_tree_only_accuracy(pkg, O):
    """group walk vs direct summation: no worse than the reference tree at the same ErrTolForceAcc"""
    n = 40000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=5)
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6, walk_mode=pkg.WALK_GROUP)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    acc1, old, _ = eng.get_accel()
    idx = np.arange(0, n, 40, dtype=np.int32)
    direct = eng.direct_sum(idx)
    assert rel_err(direct, O.direct(cfg, pos, mass, typ, idx)).max() < 1e-11   # GPU direct sum == oracle direct sum
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc2, _, cost2 = eng.get_accel()
    e_grp = rel_err(acc2[idx], direct)
    # the reference tree on the same input
    cfg_s = pkg.make_config(n_gravs=1, G=1.0, theta=0.0, softening=[0.01] * 6)
    T = O.Tree(cfg_s, pos, mass, typ)
    a_o, _ = T.walk(old_acc=old)
    e_ref = rel_err(O.finish(cfg_s, a_o)[0][idx], direct)
    print("group rms %.2e max %.2e | reference-tree rms %.2e max %.2e" %
          (np.sqrt(np.mean(e_grp ** 2)), e_grp.max(), np.sqrt(np.mean(e_ref ** 2)), e_ref.max()))
    assert np.sqrt(np.mean(e_grp ** 2)) <= np.sqrt(np.mean(e_ref ** 2)) * 1.05
    assert e_grp.max() < 0.02
    eng.close()


def test_group_walk_leftover_groups(pkg, O):
    """split walk with item lists far too short (tuning walk_lcap): most groups are left over by the traversal kernel
    and redone in sub-groups (down to one target per wave = the reference's own per-target tests) by the fused kernel.
    Every target must still get a complete force: accuracy against direct summation between the normal group walk's and
    the reference tree's, same interaction-count scale, and the regions grow for the next step."""
    n = 40000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=7)
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.01] * 6, walk_mode=pkg.WALK_GROUP)
    idx = np.arange(0, n, 40, dtype=np.int32)

    def run(tuning=None):
        eng = _engine(pkg, cfg, pos, mass, typ, tuning=tuning)
        eng.compute_accelerations(pm_step=False)
        _, old, _ = eng.get_accel()
        eng.set_opening(0.0, 0.005)
        eng.set_old_acc(old)
        eng.gravity_tree()
        acc, _, cost = eng.get_accel()
        eng.gravity_tree()                      # second step: grown regions, same input
        acc_b, _, _ = eng.get_accel()
        direct = eng.direct_sum(idx)
        eng.close()
        return acc, acc_b, cost, direct, old

    acc_n, _, cost_n, direct, old = run()
    acc_s, acc_s2, cost_s, _, _ = run(tuning={"walk_lcap": 1024})
    cfg_s = pkg.make_config(n_gravs=1, G=1.0, theta=0.0, softening=[0.01] * 6)
    a_o, _ = O.Tree(cfg_s, pos, mass, typ).walk(old_acc=old)
    e_ref = rel_err(O.finish(cfg_s, a_o)[0][idx], direct)
    e_n, e_s, e_s2 = rel_err(acc_n[idx], direct), rel_err(acc_s[idx], direct), rel_err(acc_s2[idx], direct)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    print("normal rms %.2e | short lists rms %.2e, next step %.2e | reference tree %.2e | ia/particle %.1f vs %.1f" %
          (rms(e_n), rms(e_s), rms(e_s2), rms(e_ref), cost_n.mean(), cost_s.mean()))
    assert np.all(np.isfinite(acc_s)) and np.all(cost_s > 0)
    assert rms(e_s) <= rms(e_ref) * 1.05 and e_s.max() < 0.03
    assert rms(e_s2) <= rms(e_ref) * 1.05 and e_s2.max() < 0.03
    assert 0.25 < cost_s.mean() / cost_n.mean() < 2.0   # per-target tests need fewer interactions than conservative group tests


@pytest.mark.parametrize("wiring,ng", [("newton", 1), ("c4", 2)])
@pytest.mark.parametrize("reach", [0.0, 6.0])
def test_group_walk_treepm_accuracy_vs_ewald(pkg, O, wiring, ng, reach):
    """TreePM total (tree + PM) against an independent Ewald sum (tests/golden/ewald_truth_*.npz, made by
    tests/golden/make_ewald_golden.py): the group walk must be at least as accurate as the reference walk, whose
    own error is rms 6.5e-3 .. 9.1e-3 here (7.8e-3 .. 9.6e-3).  The two walks differ at the
    1e-2 level of the (strongly cancelling) total force because the reference truncates at its rcut box
    (forcetree.c:1828-1862) while the group walk cuts on a sphere of radius group_reach * Asmth."""
    import os
    sys_path = os.path.join(os.path.dirname(__file__), "golden")
    import sys
    sys.path.insert(0, sys_path)
    from make_ewald_golden import N, L, SEED, case_config
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ewald_truth_%s.npz" % wiring))
    pos, mass, typ = pkg.ic.uniform_box(N, box=L, n_gravs=ng, seed=SEED)
    cfg, eps = case_config(pkg, wiring, ng, walk_mode=pkg.WALK_GROUP, group_reach=reach)
    eng = _engine(pkg, cfg, pos, mass, typ, old_acc=gold["old_acc"])
    eng.set_opening(0.0, 0.005)                     # steady-state pass (relative criterion)
    eng.compute_accelerations(pm_step=True)
    acc, _, cost, gpm = eng.get_accel(want_pm=True)
    idx, truth = gold["idx"], gold["truth"]
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    e_grp = rel_err((acc + gpm)[idx], truth)
    e_ref = rel_err(gold["ref_total"], truth)
    print("TreePM vs Ewald [%s reach %.1f]: group rms %.2e max %.2e ia/part %.1f | reference walk rms %.2e max %.2e ia/part %.1f" %
          (wiring, reach, rms(e_grp), e_grp.max(), cost.mean(), rms(e_ref), e_ref.max(), float(gold["ref_ia_per_part"])))
    assert rms(e_grp) <= rms(e_ref)
    assert rms(e_grp) < 1.0e-2
    eng.close()


def test_positions_outside_the_periodic_box_are_refused(pkg):
    """PERIODIC: the reference wraps the particles onto the box before it decomposes (do_box_wrapping, domain.c:81) and the
    glue does the same; the walk's start table and the evaluation kernel's shortcut for groups away from the faces rely on
    positions in [0, BoxSize].  A caller that skips the wrapping gets an error, not wrong forces."""
    pos, mass, typ = pkg.ic.uniform_box(4096, box=1.0, n_gravs=1, seed=3)
    cfg = pkg.make_config(n_gravs=1, periodic=1, pmgrid=32, box_size=1.0, G=1.0, theta=0.5, softening=[0.002] * 6)
    below, above = pos.copy(), pos.copy()
    below[7, 1] = -1e-9
    above[11, 2] = 1.0 + 1e-9
    for bad in (pos + 0.37, below, above):
        eng = pkg.Engine(cfg)
        eng.set_particles(bad, mass, typ)
        with pytest.raises(Exception):
            eng.compute_accelerations(pm_step=True)
        eng.close()
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    eng.close()


def test_group_walk_sparse_active_set_vs_ewald(pkg, O):
    """individual timesteps: only ~3 % of the particles are active (gravtree.c:113).  The group walk compacts the active
    targets of the Peano order into groups of 64 (boxes ~3x wider than a 64-particle stretch); accuracy against the Ewald
    golden stays in the reference band, inactive particles are not written, Nf is the active count, and the result agrees
    with the uncompacted walk (tuning walk_compact=0) at the level of the walk error."""
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(__file__), "golden"))
    from make_ewald_golden import N, L, SEED, case_config
    wiring, ng = "c4", 2
    gold = np.load(os.path.join(os.path.dirname(__file__), "golden", "ewald_truth_%s.npz" % wiring))
    pos, mass, typ = pkg.ic.uniform_box(N, box=L, n_gravs=ng, seed=SEED)
    idx, truth = gold["idx"], gold["truth"]
    active = (np.random.default_rng(1).uniform(size=N) < 0.02).astype(np.uint8)
    active[idx] = 1
    cfg, eps = case_config(pkg, wiring, ng, walk_mode=pkg.WALK_GROUP, group_reach=0.0)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    res = {}
    for compact in ("1", "0", "S8", "S64"):      # S8 / S64: compacted, 8 / 64 lanes per target (sub-groups of 8 / 1 targets)
        tuning = {"walk_compact": 0 if compact == "0" else 1}
        if compact.startswith("S"):
            tuning["walk_spread"] = int(compact[1:])
        eng = _engine(pkg, cfg, pos, mass, typ, tuning=tuning, old_acc=gold["old_acc"], active=active)
        eng.set_opening(0.0, 0.005)
        eng.compute_accelerations(pm_step=True)
        acc, old_out, cost, gpm = eng.get_accel(want_pm=True)
        # the reference's semantics: only active rows of P[] are touched (gravtree.c:318-341)
        sent = (np.full((N, 3), 7.0), np.full(N, 8.0), np.full(N, 9.0, dtype=np.float32))
        eng.get_accel(into=sent)
        st = eng.stats()
        eng.close()
        assert st.n_active == int(active.sum())
        assert np.all(acc[active == 0] == 0) and np.all(cost[active == 0] == 0)
        assert np.array_equal(old_out[active == 0], gold["old_acc"][active == 0])       # not walked: OldAcc is the input's
        assert np.all(sent[0][active == 0] == 7.0) and np.all(sent[1][active == 0] == 8.0) and np.all(sent[2][active == 0] == 9.0)
        assert np.array_equal(sent[0][active == 1], acc[active == 1]) and np.array_equal(sent[1][active == 1], old_out[active == 1])
        res[compact] = (acc, cost, rms(rel_err((acc + gpm)[idx], truth)))
    e_ref = rms(rel_err(gold["ref_total"], truth))
    d = rel_err(res["1"][0][active == 1], res["0"][0][active == 1])
    print("sparse active set (%d of %d): compacted rms %.2e (ia %.0f), uncompacted rms %.2e (ia %.0f), reference walk %.2e; "
          "compacted vs uncompacted median %.1e" % (active.sum(), N, res["1"][2], res["1"][1][active == 1].mean(), res["0"][2],
                                                   res["0"][1][active == 1].mean(), e_ref, np.median(d)))
    print("  lanes per target 8: rms %.2e (ia %.0f); 64: rms %.2e (ia %.0f)" %
          (res["S8"][2], res["S8"][1][active == 1].mean(), res["S64"][2], res["S64"][1][active == 1].mean()))
    for k in res:
        assert res[k][2] <= e_ref * 1.05, k
    assert np.median(d) < 5e-3


@pytest.mark.parametrize("wiring,ng,theta", [("c4", 2, 0.0), ("newton", 1, 0.5), ("c4", 3, 0.0)])
def test_group_walk_kernels_reproduce_the_reference_interaction_set(pkg, O, wiring, ng, theta):
    """The PRODUCTION kernels (traversal k_walk_group2<..,1> + evaluation k_walk_group2<..,2>: item lists, LDS pool, fp32 reach
    masks, table-bin Yukawa factor, rsq + Newton step) against the oracle, tightly: with one target per wave (64 lanes per
    target: the group's box is the target itself, so every conservative group test IS the reference's per-target test), the
    cut at the end of the short-range table (group_reach 6.0 = tabindex < NTAB, forcetree.c:1962-1967), no leaf shortcut
    (walk_nleaf 0) and the walk started at the root, the group walk must take exactly the reference's interactions:
    forces equal to rounding of the different arithmetic (1e-11 -- one wrong or missing interaction shows at 1e-3), and for one
    species identical interaction counts for every target."""
    n, L, pmgrid = 24000, 1.0, 32
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=91)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_STRICT, group_reach=6.0)
    active = (np.random.default_rng(5).uniform(size=n) < 0.4).astype(np.uint8)       # < 3/4 active: targets are compacted
    idx = np.nonzero(active)[0].astype(np.int32)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    _, old, _ = eng.get_accel()
    eng.close()
    cfg.err_tol_theta = theta                                                         # 0: relative criterion with that OldAcc
    tab, _ = O.shortrange_table(cfg)
    T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
    a_o, n_o = T.walk(old_acc=old, idx=idx, table=tab)
    cfg.walk_mode = pkg.WALK_GROUP
    eng = _engine(pkg, cfg, pos, mass, typ, tuning={"walk_spread": 64, "walk_nleaf": 0, "walk_root": 1, "walk_sg": 1},
                  old_acc=old, active=active)
    eng.domain_Decomposition()
    eng.gravity_tree()
    acc, _, cost = eng.get_accel()
    st = eng.stats()
    eng.close()
    assert st.reserved[5] >= 1                                                        # the split (traversal + evaluation) kernels ran
    # GravCost: the reference counts a node once, the group walk once per source species that holds mass in it
    if ng == 1:
        assert np.array_equal(cost[idx].astype(np.int64), n_o.astype(np.int64))
    else:
        assert np.all(cost[idx] >= n_o) and cost[idx].mean() < 1.5 * n_o.mean()
    err = np.abs(acc[idx] / cfg.G - a_o).max() / np.abs(a_o).max()
    print("group-walk kernels, one target per wave [%s, N_GRAVS=%d, theta=%g]: %.1f (oracle %.1f) interactions/target, max force diff %.1e"
          % (wiring, ng, theta, cost[idx].mean(), n_o.mean(), err))
    assert err < 1e-11
    assert np.all(acc[active == 0] == 0)


@pytest.mark.parametrize("theta", [0.5, 0.0])
def test_group_walk_kernels_reproduce_the_reference_set_tree_only(pkg, O, theta):
    """The same for a tree-only, non-periodic set (no cut, no tables: other instantiations of the same kernels): Plummer sphere,
    two species with DIFFERENT softening lengths (the per-source softening type travels through the pool), Barnes-Hut and relative
    criterion; one target per wave, no leaf shortcut, start at the root -> the oracle's forces to rounding."""
    n = 20000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=78)
    typ = (1 + (np.arange(n) % 2)).astype(np.int32)
    cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.5, softening=[0.01, 0.01, 0.03, 0.01, 0.01, 0.01],
                          type_to_grav=pkg.ic.default_type_to_grav(2), wiring="newton", walk_mode=pkg.WALK_STRICT)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    _, old, _ = eng.get_accel()
    eng.close()
    cfg.err_tol_theta = theta
    active = (np.random.default_rng(6).uniform(size=n) < 0.3).astype(np.uint8)
    idx = np.nonzero(active)[0].astype(np.int32)
    T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
    a_o, n_o = T.walk(old_acc=old, idx=idx)
    cfg.walk_mode = pkg.WALK_GROUP
    for fused in (0, 1):
        eng = _engine(pkg, cfg, pos, mass, typ, old_acc=old, active=active,
                      tuning={"walk_spread": 64, "walk_nleaf": 0, "walk_root": 1, "walk_sg": 1, "walk_fused": fused})
        eng.compute_accelerations(pm_step=False)
        acc, _, cost = eng.get_accel()
        eng.close()
        err = np.abs(acc[idx] / cfg.G - a_o).max() / np.abs(a_o).max()
        print("tree-only group-walk kernels (%s), one target per wave, theta=%g: max force diff %.1e; %.1f (oracle %.1f) interactions" %
              ("fused" if fused else "split", theta, err, cost[idx].mean(), n_o.mean()))
        assert err < 1e-11 and np.all(cost[idx] >= n_o)


@pytest.mark.parametrize("ng", [2, 3])
def test_production_walk_is_the_cut_direct_sum(pkg, O, ng):
    """The production configuration of the production kernels -- 64 targets per wave, traversal units of four groups, sphere cut at
    RCUT (group_reach 4.5), leaf shortcut, start table, wrap-free groups: nothing tuned -- against an exact quantity: at the bench's
    density and criterion every source inside the cut sphere reaches the force loop as a PARTICLE (the relative criterion opens
    every cell this close for at least one of the 256 targets of a unit), so the group walk's force must be the sum of the
    reference's short-range pair interaction (forcetree.c:1953-2032) over every particle within RCUT * Asmth, pair for pair:
    identical interaction counts and forces to rounding for (almost) every target; a target whose list holds a monopole is
    counted and bounded.  This ties the production path to the oracle's arithmetic, not to an error band."""
    n, L, pmgrid = 1 << 17, 1.0, 64                               # 2 mesh cells per particle, as C4 / C5
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=123)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_GROUP)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=True)                       # theta pass: OldAcc
    _, old, _ = eng.get_accel()
    eng.set_old_acc(old)
    eng.set_opening(0.0, 0.005)                                    # the steady-state relative criterion of the bench
    eng.compute_accelerations(pm_step=True)
    acc, _, cost = eng.get_accel()
    st = eng.stats()
    eng.close()
    assert st.reserved[5] >= 1                                     # the split (traversal + evaluation) kernels ran
    idx = np.sort(np.random.default_rng(11).choice(n, 512, replace=False)).astype(np.int32)
    tab, _ = O.shortrange_table(cfg)
    reach = 4.5 * 1.25 * L / pmgrid
    a_o, n_o = O.direct_shortrange(cfg, pos, mass, typ, idx, tab, reach)
    err = np.linalg.norm(acc[idx] / cfg.G - a_o, axis=1) / np.linalg.norm(a_o, axis=1)
    same = cost[idx].astype(np.int64) == n_o.astype(np.int64)
    exact = err < 1e-10
    print("production group walk vs cut direct sum [N_GRAVS=%d]: %.1f (oracle %.1f) pairs/target; counts equal for %d, force equal to "
          "rounding for %d of %d targets (median %.1e, worst of those %.1e); the others: max %.1e" %
          (ng, cost[idx].mean(), n_o.mean(), same.sum(), exact.sum(), len(idx), np.median(err), err[exact].max(), err.max()))
    assert same.mean() > 0.97 and exact.mean() > 0.97               # (almost) every target: the same pairs, the same force to rounding
    assert err.max() < 2e-3                                         # the rest: a cell at the edge of the cut taken as one monopole
    assert abs(cost[idx].mean() - n_o.mean()) < 0.01 * n_o.mean()


def test_group_walk_three_species(pkg, O):
    """N_GRAVS=3 (the C5 wiring: Newton diagonal, Newton+Yukawa off-diagonal; short-range tables read through L1/L2
    instead of LDS): the group walk stays within the reference walk's own error band of the strict result"""
    n, L, pmgrid, ng = 30000, 1e4, 32, 3
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=44)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_STRICT)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    acc_s, old, cost_s, pm = eng.get_accel(want_pm=True)
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    acc_s2, _, _ = eng.get_accel()
    eng.set_walk_mode(pkg.WALK_GROUP)
    eng.gravity_tree()
    acc_g, _, cost_g = eng.get_accel()
    # against the periodic direct sum (the reference's FORCETEST truth): the group walk must not be less accurate than the
    # reference walk (strict) on the same input, and inside the reference TreePM band
    idx = np.arange(0, n, 75, dtype=np.int32)
    truth = eng.direct_sum(idx)
    e_g, e_s = rel_err((acc_g + pm)[idx], truth), rel_err((acc_s2 + pm)[idx], truth)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    print("N_GRAVS=3 vs periodic direct sum: group rms %.2e max %.2e | reference walk rms %.2e max %.2e" %
          (rms(e_g), e_g.max(), rms(e_s), e_s.max()))
    assert rms(e_g) <= rms(e_s) * 1.02 and rms(e_g) < 9.6e-3
    assert np.all(np.isfinite(acc_g)) and cost_g.min() >= 1
    # momentum: symmetric wiring -> the short-range forces nearly cancel in the sum
    assert np.abs(np.sum(mass[:, None] * acc_g, axis=0)).max() / np.sum(mass[:, None] * np.abs(acc_g)) < 2e-3
    eng.close()


def test_edge_cases_small_and_ragged(pkg, O):
    for n in (1, 2, 63, 64, 65, 130):
        rng = np.random.default_rng(n)
        pos = rng.uniform(-1, 1, (n, 3))
        mass = rng.uniform(0.5, 1.5, n)
        typ = (1 + rng.integers(0, 2, n)).astype(np.int32)
        cfg = pkg.make_config(n_gravs=2, G=2.0, theta=0.5, softening=[0.05, 0.05, 0.02, 0.05, 0.05, 0.05],
                              type_to_grav=pkg.ic.default_type_to_grav(2), wiring="newton", tree_alloc_factor=4.0)
        idx = np.arange(n, dtype=np.int32)
        want = O.direct(cfg, pos, mass, typ, idx)
        for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
            cfg.walk_mode = mode
            eng = _engine(pkg, cfg, pos, mass, typ)
            eng.set_opening(1e-9, 0.005)          # theta -> 0: every node is opened, the walk becomes a direct sum
            eng.compute_accelerations(pm_step=False)
            acc, _, cost = eng.get_accel()
            if n > 1:
                assert rel_err(acc, want).max() < 1e-10, (n, mode)
            else:
                assert np.abs(acc).max() < 1e-9      # self term only: COM rounding x spline core
            assert np.all(cost == n)
            eng.close()


def test_inactive_particles_and_buckets(pkg, O):
    n = 5000
    rng = np.random.default_rng(77)
    pos = rng.uniform(0, 1, (n, 3))
    pos[100:108] = pos[100]                      # 8 coincident particles: below any key resolution -> bucket leaf
    mass = np.full(n, 1.0 / n)
    typ = np.ones(n, dtype=np.int32)
    active = (rng.uniform(size=n) < 0.3).astype(np.uint8)
    active[100:104] = 1
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.4, softening=[0.01] * 6, tree_alloc_factor=2.0)
    idx = np.nonzero(active)[0].astype(np.int32)
    want = O.direct(cfg, pos, mass, typ, idx)
    for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
        cfg.walk_mode = mode
        eng = _engine(pkg, cfg, pos, mass, typ, active=active, old_acc=np.full(n, 0.25))
        eng.compute_accelerations(pm_step=False)
        acc, old, cost = eng.get_accel()
        assert np.all(acc[active == 0] == 0) and np.all(cost[active == 0] == 0)     # only active particles are written
        assert np.all(old[active == 0] == 0.25)                                     # ... and inactive ones keep their OldAcc
        assert np.allclose(old[active == 1], np.linalg.norm(acc[active == 1], axis=1), rtol=1e-12)
        e = rel_err(acc[idx], want)
        assert np.median(e) < 5e-3 and np.quantile(e, 0.99) < 5e-2     # BH theta=0.4 in a uniform cube: a few weak-force outliers
        st = eng.stats()
        assert st.n_active == int(active.sum())
        eng.close()


def test_one_pass_build_is_the_levelwise_tree(pkg, O):
    """The one-pass build (every particle starts the nodes of levels (d_prev, d_cur]) and the level-by-level build (the
    multi-task path) give the SAME tree: same node count, and the reference walk on them returns bitwise equal accelerations
    and equal interaction counts -- clustered, uniform, coincident particles (buckets), two species."""
    rng = np.random.default_rng(2024)
    cases = []
    pos, _, _ = pkg.ic.plummer_sphere(30000, seed=5)
    cases.append((pos, np.ones(30000, dtype=np.int32)))
    pos = rng.uniform(0, 1, (20000, 3))
    pos[500:520] = pos[500]                       # a bucket of 20
    pos[7000:7003] = pos[7000]
    cases.append((pos, (1 + (np.arange(20000) % 2)).astype(np.int32)))
    pos = rng.uniform(0, 1, (2, 3))
    cases.append((pos, np.ones(2, dtype=np.int32)))
    for pos, typ in cases:
        n = len(pos)
        mass = rng.uniform(0.5, 1.5, n) / n
        ng = 2 if typ.max() > 1 else 1
        kw = dict(n_gravs=ng, G=1.0, theta=0.5, softening=[0.005] * 6, tree_alloc_factor=2.5)
        if ng == 2:
            kw.update(type_to_grav=[0, 0, 1, 1, 1, 1], wiring="coloyuk", yukawa_imass=3.0, box_size=1.0)
        cfg = pkg.make_config(**kw)
        cfg.walk_mode = pkg.WALK_STRICT
        res = []
        for levelwise in (0, 1):
            eng = _engine(pkg, cfg, pos, mass, typ, tuning=dict(tree_levelwise=levelwise))
            eng.compute_accelerations(pm_step=False)
            acc, old, cost = eng.get_accel()
            res.append((acc.copy(), cost.copy(), eng.stats().n_nodes))
            eng.close()
        assert res[0][2] == res[1][2] and res[0][2] >= 1
        assert np.array_equal(res[0][1], res[1][1])
        assert np.array_equal(res[0][0], res[1][0])
        print("one-pass == level-wise: n=%d, %d nodes" % (n, res[0][2]))


def test_two_stage_sort_is_the_full_sort(pkg, O):
    """Peano order by a radix sort on the top 42 key bits + a stable fix-up of the runs that tie there == a stable radix sort on
    all 63 bits (tuning sort_full): bitwise equal reference-walk forces, equal interaction counts and node counts -- with
    pairs that share their top bits (particles 1e-6 apart), a clump of 40 coincident particles (fixed up in place) and a clump of
    300 (longer than the fix-up allows: falls back to the full sort)."""
    rng = np.random.default_rng(11)
    n = 60000
    pos = rng.uniform(0, 1, (n, 3))
    pos[1000:1400] = pos[500:900] + rng.uniform(0, 1e-6, (400, 3))   # close pairs: equal top bits, different low bits
    for clump in (40, 300):
        p2 = pos.copy()
        p2[2000:2000 + clump] = p2[2000]
        mass = rng.uniform(0.5, 1.5, n) / n
        typ = np.ones(n, dtype=np.int32)
        cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.5, softening=[0.004] * 6, tree_alloc_factor=2.5)
        cfg.walk_mode = pkg.WALK_STRICT
        res = []
        for full in (0, 1):
            eng = _engine(pkg, cfg, p2, mass, typ, tuning=dict(sort_full=full))
            eng.compute_accelerations(pm_step=False)
            acc, old, cost = eng.get_accel()
            res.append((acc.copy(), cost.copy(), eng.stats().n_nodes))
            eng.close()
        assert res[0][2] == res[1][2]
        assert np.array_equal(res[0][1], res[1][1]) and np.array_equal(res[0][0], res[1][0])


def test_grav_pm_handed_over_with_the_particles(pkg, O):
    """A PM step followed by a non-PM step that goes through set_particles again (TreeDomainUpdateFrequency = 0: the glue
    re-decomposes every step).  P[].GravPM lives in the host's P[] between PM steps; handed over with the particles it must
    enter OldAcc = |GravAccel + GravPM/G| exactly as in the reference (gravtree.c:318-330) -- the oracle's finish()."""
    n, L, ng = 20000, 1.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=21)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=32, box_size=L, G=2.5, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_STRICT)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    acc1, old1, _, pm1 = eng.get_accel(want_pm=True)
    # next step: the same particles come in again (fresh P[] hand-over), no PM this step
    eng.set_particles(pos, mass, typ, old_acc=old1, grav_pm=pm1)
    eng.compute_accelerations(pm_step=False)
    acc2, old2, _, pm2 = eng.get_accel(want_pm=True)
    assert np.array_equal(pm2, pm1)                                   # GravPM survives the hand-over unchanged
    assert np.allclose(old2, np.linalg.norm(acc2 / cfg.G + pm1 / cfg.G, axis=1), rtol=1e-12)
    # without GravPM the library cannot know it: OldAcc = |GravAccel| only, and asking for GravPM is a state error
    eng.set_particles(pos, mass, typ, old_acc=old1)
    eng.compute_accelerations(pm_step=False)
    acc3, old3, _ = eng.get_accel()
    assert np.allclose(old3, np.linalg.norm(acc3 / cfg.G, axis=1), rtol=1e-12)
    with pytest.raises(pkg.NgravsError):
        eng.get_pm()
    # oracle: same walk + finish() with the PM force
    tab, _ = O.shortrange_table(cfg)
    T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
    a_o, _ = T.walk(table=tab)
    a_fin, old_o = O.finish(cfg, a_o, O.pm_periodic(cfg, pos, mass, typ))
    assert np.abs(acc2 - a_fin).max() / np.abs(a_fin).max() < TOL
    assert np.abs(old2 - old_o).max() / old_o.max() < TOL
    eng.close()


def test_slab_pm_one_task_equals_the_3d_transform(pkg, O):
    """pmforce_periodic on the slab-decomposed mesh (brick deposit, plane exchanges, 2-D + 1-D FFTs with the Green's
    function on the transposed layout, brick gather) with ONE task must equal the single-task path (3-D FFT on the full
    mesh) to rounding, and the oracle's pmforce_periodic to 1e-10, for 1, 2 and 3 species."""
    import importlib
    import torch.distributed as dist
    dd = importlib.import_module("ngravs_amd.distributed")
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (29400 + os.getpid() % 500), rank=0, world_size=1)
    for ng, wiring, pmgrid in ((1, "newton", 32), (2, "c4", 64), (3, "c4", 32)):
        n, L = 30000, 2.5
        pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=40 + ng)
        pos[: n // 3] = 0.2 * L + 0.3 * (pos[: n // 3] - 0.2 * L)         # a clump: bricks and slabs see uneven load
        eps = L / (40 * n ** (1 / 3))
        kw = dict(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=1.7, theta=0.5, softening=[eps] * 6,
                  type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_GROUP)
        eng = pkg.Engine(pkg.make_config(**kw))
        eng.set_particles(pos, mass, typ)
        eng.domain_Decomposition()
        eng.pmforce_periodic()
        pm_ref = eng.get_pm()
        eng.close()
        deng = dd.DistributedEngine(pkg.make_config(**kw))
        deng.set_particles(pos, mass, typ)
        deng.domain_Decomposition()
        deng.pmforce_periodic()
        deng.n = deng.num_local()
        pm_slab = deng.get_pm()
        ids = deng.local_ids()
        deng.close()
        full = np.zeros_like(pm_ref)
        full[ids] = pm_slab
        scale = np.abs(pm_ref).max()
        pm_o = O.pm_periodic(pkg.make_config(**kw), pos, mass, typ)
        print("slab PM, N_GRAVS=%d PMGRID=%d: vs 3-D path %.1e, vs oracle %.1e" %
              (ng, pmgrid, np.abs(full - pm_ref).max() / scale, np.abs(full - pm_o).max() / scale))
        assert np.abs(full - pm_ref).max() / scale < 1e-12
        assert np.abs(full - pm_o).max() / scale < TOL


def test_cell_sums_in_the_last_peano_order(pkg, O):
    """The top-cell sums of a multi-task decomposition (histogram + work, per-type counts, per-species mass and first moments:
    the global top of the tree is built from them) are taken in plain row order on the first step and, from the second step on,
    in the Peano order of the last local decomposition with one atomic per wave and value.  Same particles, Barnes-Hut criterion
    (no OldAcc dependence): the second step must return the first step's forces (summation order of the sums only) and equal
    interaction counts, and both the single-task engine's -- two species, a clump so that waves straddle cells."""
    import importlib
    import torch.distributed as dist
    dd = importlib.import_module("ngravs_amd.distributed")
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (29400 + os.getpid() % 500), rank=0, world_size=1)
    n = 50000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=91)
    typ = (1 + (np.arange(n) % 2)).astype(np.int32)
    mass = mass * np.where(typ == 2, 3.0, 1.0)
    kw = dict(n_gravs=2, G=1.0, theta=0.5, softening=[0.01, 0.01, 0.02, 0.01, 0.01, 0.01],
              type_to_grav=pkg.ic.default_type_to_grav(2), wiring="newton", walk_mode=pkg.WALK_STRICT)
    eng = pkg.Engine(pkg.make_config(**kw))
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    a1, _, c1 = eng.get_accel()
    eng.close()
    deng = dd.DistributedEngine(pkg.make_config(**kw))
    deng.set_particles(pos, mass, typ, ids=np.arange(n))
    res = []
    for step in range(3):
        deng.compute_accelerations(pm_step=False)
        acc, _, cost = deng.get_accel()[:3]
        ids = deng.local_ids()
        a = np.zeros((n, 3))
        c = np.zeros(n)
        a[ids] = acc
        c[ids] = cost
        res.append((a, c))
    deng.close()
    for step, (a, c) in enumerate(res):
        err = np.linalg.norm(a - a1, axis=1) / np.linalg.norm(a1, axis=1)
        print("step %d vs the single-task engine: max |da|/|a| = %.2e" % (step, err.max()))
        assert np.array_equal(c, c1)
        assert err.max() < 1e-10
    assert np.abs(res[1][0] - res[0][0]).max() / np.abs(res[0][0]).max() < 1e-12


def test_bam_laws_strict_walk_and_direct_sum(pkg, O):
    """the BAM / NGRAVS_ACCUMULATOR family (ngravs.c:495-668; wiring NGRAVS_ACCUMULATOR_TESTING :163-210): laws of
    the TARGET mass and of the number of particles of the source species a node holds (allvars.h:645-648).  Baryons (species
    0) and BAM halos (species 1) with unequal masses so that both dependences matter; the reference walk on the GPU must equal
    the oracle (1e-10, identical interaction counts), the GPU direct sum the oracle's, and the tree error against the direct
    sum stays at the tree's level.  The GROUP walk evaluates the same laws in its own force loop (target mass per lane, particle
    number per pool entry): conservative group decisions, so at least the reference walk's interactions and accuracy."""
    n = 20000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=77)
    rng = np.random.default_rng(3)
    typ = (1 + (np.arange(n) % 2)).astype(np.int32)
    mass = mass * np.where(typ == 2, rng.uniform(5.0, 20.0, n), rng.uniform(0.5, 1.5, n))     # BAM halos heavier, all unequal
    cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.6, softening=[0.01] * 6, type_to_grav=pkg.ic.default_type_to_grav(2),
                          wiring="bam", walk_mode=pkg.WALK_STRICT)
    cfg.bam_epsilon = 0.05                      # eta r of order one inside the sphere: both branches of the law are exercised
    T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
    a_o, n_o = T.walk()
    a_o, _ = O.finish(cfg, a_o)
    idx = np.arange(0, n, 50, dtype=np.int32)
    d_o = O.direct(cfg, pos, mass, typ, idx)
    cfg.walk_mode = pkg.WALK_STRICT
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    acc, _, cost = eng.get_accel()
    d_g = eng.direct_sum(idx)
    assert np.array_equal(cost.astype(np.int64), n_o.astype(np.int64))
    assert np.abs(acc - a_o).max() / np.abs(a_o).max() < TOL
    assert np.abs(d_g - d_o).max() / np.abs(d_o).max() < 1e-11
    e = rel_err(acc[idx], d_o)
    print("BAM wiring: strict == oracle, tree vs direct rms %.2e max %.2e, %.1f interactions/particle" %
          (np.sqrt(np.mean(e ** 2)), e.max(), n_o.mean()))
    assert np.sqrt(np.mean(e ** 2)) < 2e-2
    # the production walk: its own kernels (split traversal + evaluation), and in one-target-per-wave mode the reference's set
    eng.set_walk_mode(pkg.WALK_GROUP)
    eng.gravity_tree()
    acc_g, _, cost_g = eng.get_accel()
    st = eng.stats()
    eng.close()
    eg = rel_err(acc_g[idx], d_o)
    print("BAM wiring, group walk: tree vs direct rms %.2e max %.2e, %.1f interactions/particle (split kernels: %d launches)" %
          (np.sqrt(np.mean(eg ** 2)), eg.max(), cost_g.mean(), int(st.reserved[5])))
    assert st.reserved[5] >= 1
    assert np.all(cost_g >= n_o) and np.sqrt(np.mean(eg ** 2)) <= 1.05 * np.sqrt(np.mean(e ** 2))
    active = (np.random.default_rng(5).uniform(size=n) < 0.3).astype(np.uint8)
    sel = np.nonzero(active)[0]
    cfg.walk_mode = pkg.WALK_GROUP
    eng = _engine(pkg, cfg, pos, mass, typ, tuning={"walk_spread": 64, "walk_nleaf": 0, "walk_root": 1, "walk_sg": 1}, active=active)
    eng.compute_accelerations(pm_step=False)
    acc1, _, cost1 = eng.get_accel()
    eng.close()
    err1 = np.abs(acc1[sel] - a_o[sel]).max() / np.abs(a_o).max()
    print("BAM wiring, group-walk kernels with one target per wave: max force diff to the oracle %.1e" % err1)
    assert err1 < 1e-10


def test_bad_type_on_device_is_rejected(pkg):
    import torch
    n = 1000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=2)
    typ = typ.astype(np.int32)
    typ[17] = 9
    dev = torch.device("cuda", 0)
    d_pos, d_mass, d_typ = torch.from_numpy(pos).to(dev), torch.from_numpy(mass).to(dev), torch.from_numpy(typ).to(dev)
    eng = pkg.Engine(pkg.make_config(n_gravs=1, softening=[0.01] * 6))
    with pytest.raises(pkg.NgravsError):
        eng.set_particles_device(n, d_pos.data_ptr(), d_mass.data_ptr(), d_typ.data_ptr())
    with pytest.raises(pkg.NgravsError):
        eng.set_tuning(no_such_knob=1)
    eng.close()


def test_error_convention(pkg):
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6)
    eng = pkg.Engine(cfg)
    with pytest.raises(pkg.NgravsError):
        eng.gravity_tree()                        # no particles yet: state error, as an endrun() would
    pos, mass, typ = pkg.ic.plummer_sphere(2000, seed=1)
    eng.set_particles(pos, mass, typ)
    with pytest.raises(pkg.NgravsError):
        eng.pmforce_periodic()                    # PM without PMGRID/PERIODIC
    cfg2 = pkg.make_config(n_gravs=1, softening=[0.01] * 6, tree_alloc_factor=0.01)
    eng2 = pkg.Engine(cfg2)
    eng2.set_particles(np.repeat(pos, 4, axis=0) + np.random.default_rng(0).normal(0, 1e-9, (8000, 3)),
                       np.repeat(mass, 4), np.repeat(typ, 4))
    with pytest.raises(pkg.NgravsError):          # endrun(1): maximum number of tree-nodes reached
        eng2.compute_accelerations(pm_step=False)
    eng.close()
    eng2.close()


def test_pm_persists_between_pm_steps_and_multi_shard(pkg, O):
    """GravPM survives a non-PM step (a new domain decomposition), and target shards of a
    world_size-2 job reproduce the single-task result exactly (domain.c:18-21 invariant)."""
    n, L = 20000, 1e4
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=31)
    eps = L / (40 * n ** (1 / 3))
    kw = dict(n_gravs=2, periodic=1, pmgrid=32, box_size=L, G=43007.1, theta=0.5, softening=[eps] * 6,
              type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4", walk_mode=pkg.WALK_GROUP)
    eng = _engine(pkg, pkg.make_config(**kw), pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    acc, old, cost, gpm = eng.get_accel(want_pm=True)
    eng.compute_accelerations(pm_step=False)
    acc_b, old_b, _, gpm_b = eng.get_accel(want_pm=True)
    assert np.array_equal(gpm, gpm_b) and np.array_equal(old, old_b)
    parts = []
    for r in range(2):
        e = _engine(pkg, pkg.make_config(rank=r, world_size=2, **kw), pos, mass, typ)
        e.compute_accelerations(pm_step=True)
        a, _, c = e.get_accel()
        first, count = e.shard()
        assert (first, count) == pkg.shard_range(n, r, 2)
        o = e.order()[first:first + count]
        parts.append((o, a))
        assert np.all(np.delete(a, o, axis=0) == 0)
        e.close()
    merged = np.zeros_like(acc)
    for o, a in parts:
        merged[o] = a[o]
    assert np.array_equal(merged, acc)
    eng.close()


@pytest.mark.parametrize("ng,wiring", [(1, "newton"), (2, "newton")])
def test_dynamic_tree_update_against_the_reference_semantics(pkg, O, ng, wiring):
    """SURVEY 8f-3 in the reference's own terms.  The reference keeps the tree between rebuilds and (i) drifts every node's
    per-species centre of mass with the node velocity, s += vs dt (predict.c:79-91), (ii) enlarges cells that particles left
    (force_update_len, forcetree.c:1005-1085); the oracle restates both (orc_tree_drift).  The library refits instead: it
    recomputes moments from the drifted particles and grows a cell to enclose its particles and child cells.  For a pure drift
    the two are the same tree -- the mass-weighted node velocity moves the centre of mass exactly, and the growth rules coincide
    except for the reference's 0.999999 slack -- so the reference walk on the GPU's refit tree must reproduce the oracle's walk
    on its drifted tree: same interaction counts and forces to rounding for (nearly) every particle."""
    n = 30000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=5)
    typ = (1 + (np.arange(n) % ng)).astype(np.int32)
    rng = np.random.default_rng(8)
    vel = 0.4 * rng.standard_normal((n, 3))
    dt = 0.05                                                   # moves particles by ~2 softening lengths: many leave their cells
    pos2 = pos + vel * dt
    cfg = pkg.make_config(n_gravs=ng, G=1.0, theta=0.5, softening=[0.01] * 6, type_to_grav=pkg.ic.default_type_to_grav(ng),
                          wiring=wiring, walk_mode=pkg.WALK_STRICT)
    T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
    T.drift(pos2, vel, dt)
    a_o, n_o = T.walk()
    a_o, _ = O.finish(cfg, a_o)
    eng = _engine(pkg, cfg, pos, mass, typ)
    eng.compute_accelerations(pm_step=False)                    # builds the tree on the undrifted positions
    eng.update_particles(pos2, mass, typ)
    eng.gravity_tree()                                          # refit + walk
    acc, _, cost = eng.get_accel()
    eng.close()
    same = cost.astype(np.int64) == n_o.astype(np.int64)
    err = np.linalg.norm(acc - a_o, axis=1) / np.linalg.norm(a_o, axis=1)
    print("drifted tree, N_GRAVS=%d: interaction counts equal for %.3f %% of the particles, |da|/|a| median %.1e, 99.9 %% %.1e, max %.1e"
          % (ng, 100.0 * same.mean(), np.median(err), np.quantile(err, 0.999), err.max()))
    assert same.mean() > 0.999                                  # the 0.999999 slack of force_update_len flips a few openings
    assert np.median(err) < 1e-13 and np.quantile(err, 0.99) < 1e-10 and err.max() < 1e-2


@pytest.mark.parametrize("ng", [1, 2])
def test_node_kicks_against_the_refit(pkg, O, ng):
    """The node kicks of timestep.c:331-344: a particle kicked by dv while the tree is kept adds dv m / M_k to the velocity of every
    ancestor (restated in the oracle, orc_tree_drift_kicked), so that the following node drift (predict.c:79-91) moves the centres
    of mass with the NEW velocities.  The library keeps no node velocities: it refits from the drifted particles.  N_GRAVS = 1: the
    kicked node velocity is the mass-weighted mean of the kicked particle velocities, the drifted centre of mass is the exact one,
    and the reference walk on the refit tree reproduces the oracle's walk on its kicked + drifted tree -- equal counts, forces to
    rounding.  N_GRAVS = 2: the reference adds a particle's kick to the node velocities of BOTH species (the loop over k at
    timestep.c:337-340 does not look at the particle's own species), its drifted centres of mass are then NOT those of the
    drifted particles; the refit keeps the exact ones.  The test measures that reference quirk (documented deviation,
    DESIGN 8) and checks that without kicks of the foreign species the two agree again."""
    n = 30000
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=5)
    typ = (1 + (np.arange(n) % ng)).astype(np.int32)
    rng = np.random.default_rng(8)
    vel = 0.4 * rng.standard_normal((n, 3))
    dv = 0.2 * rng.standard_normal((n, 3))
    dt = 0.05
    cfg = pkg.make_config(n_gravs=ng, G=1.0, theta=0.5, softening=[0.01] * 6, type_to_grav=pkg.ic.default_type_to_grav(ng),
                          wiring="newton", walk_mode=pkg.WALK_STRICT)

    def both(dv_):
        pos2 = pos + (vel + dv_) * dt
        T = O.Tree(cfg, pos, mass, typ, O.domain_extent(pos))
        T.drift_kicked(pos2, vel, dv_, dt)
        a_o, n_o = T.walk()
        a_o, _ = O.finish(cfg, a_o)
        T.close()
        eng = _engine(pkg, cfg, pos, mass, typ)
        eng.compute_accelerations(pm_step=False)
        eng.update_particles(pos2, mass, typ)
        eng.gravity_tree()
        acc, _, cost = eng.get_accel()
        eng.close()
        same = cost.astype(np.int64) == n_o.astype(np.int64)
        err = np.linalg.norm(acc - a_o, axis=1) / np.linalg.norm(a_o, axis=1)
        return same, err

    same, err = both(dv)
    print("kicked + drifted tree, N_GRAVS=%d: counts equal for %.3f %%, |da|/|a| median %.1e, 99 %% %.1e, max %.1e"
          % (ng, 100.0 * same.mean(), np.median(err), np.quantile(err, 0.99), err.max()))
    if ng == 1:
        assert same.mean() > 0.999
        assert np.median(err) < 1e-13 and np.quantile(err, 0.99) < 1e-10 and err.max() < 1e-2
    else:
        # the reference's cross-species kicks displace its node centres of mass: visible, small (a monopole position error of
        # |dv| dt m_other / M_k inside cells the walk accepted)
        assert np.median(err) > 1e-9 and np.quantile(err, 0.99) < 5e-2
        dv1 = dv.copy()
        dv1[typ != 1] = 0.0                                     # kicks of ONE species: the other species' node velocities still move
        _, err1 = both(dv1)
        dv0 = np.zeros_like(dv)
        same0, err0 = both(dv0)                                 # no kicks: the pure drift, identical again
        print("   kicks of species 0 only: median %.1e; no kicks: counts equal %.3f %%, median %.1e" % (np.median(err1), 100.0 * same0.mean(), np.median(err0)))
        assert np.median(err1) > 1e-10
        assert same0.mean() > 0.999 and np.median(err0) < 1e-13


def test_dynamic_tree_update_refit(pkg, O):
    """ngravs_update_particles + ngravs_force_update_tree (the drifted tree of TreeDomainUpdateFrequency > 0):
    (a) unchanged positions: the refit tree gives bit-identical forces to the freshly built one;
    (b) drifted positions (a fraction of the mean spacing): forces on the refit tree agree with a full re-decomposition
        + rebuild at the level of the walk's own error, for the strict and the group walk, and the total stays as
        accurate against the periodic direct sum;
    (c) without a tree the call is refused (NGRAVS_ERR_STATE)."""
    n, L, ng = 40000, 1.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=77)
    eps = L / (40 * n ** (1 / 3))
    kw = dict(n_gravs=ng, periodic=1, pmgrid=32, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4")
    rng = np.random.default_rng(3)
    drift = 0.3 * L / n ** (1 / 3) * rng.standard_normal((n, 3))
    # between decompositions the reference does NOT wrap particles back into the box (do_box_wrapping() runs in
    # domain_Decomposition only): drifted positions may leave [0, L) slightly, NEAREST takes care of the images
    pos2 = (pos + drift).astype(np.float32).astype(np.float64)
    pos2w = np.mod(pos2, L)
    pos2w[pos2w >= L] = 0.0
    idx = np.arange(0, n, 100, dtype=np.int32)
    for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
        eng = pkg.Engine(pkg.make_config(walk_mode=mode, **kw))
        with pytest.raises(pkg.NgravsError):
            eng.set_particles(pos, mass, typ)
            eng.update_particles(pos, mass, typ)            # (c) no tree yet
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=True)
        a0, old, c0, pm0 = eng.get_accel(want_pm=True)
        eng.set_opening(0.0, 0.005)
        eng.set_old_acc(old)
        eng.gravity_tree()
        a1, _, c1 = eng.get_accel()
        # (a) same positions
        eng.update_particles(pos, mass, typ, old_acc=old)
        eng.gravity_tree()
        a1b, _, c1b = eng.get_accel()
        assert np.array_equal(a1, a1b) and np.array_equal(c1, c1b)
        # (b) drifted positions on the old tree
        nodes_before = eng.stats().n_nodes
        eng.update_particles(pos2, mass, typ, old_acc=old)
        eng.gravity_tree()                                          # GravPM is kept between PM steps
        a2, _, c2, pm2 = eng.get_accel(want_pm=True)
        assert eng.stats().n_nodes == nodes_before and np.array_equal(pm2, pm0)
        truth = eng.direct_sum(idx)
        eng.close()
        ref = pkg.Engine(pkg.make_config(walk_mode=mode, **kw))
        ref.set_particles(pos2w, mass, typ, old_acc=old)
        ref.set_opening(0.0, 0.005)
        ref.compute_accelerations(pm_step=True)
        a3, _, c3, pm3 = ref.get_accel(want_pm=True)
        ref.close()
        d = rel_err(a2 + pm3, a3 + pm3)                             # same (fresh) long-range part on both sides
        e_refit, e_fresh = rel_err((a2 + pm3)[idx], truth), rel_err((a3 + pm3)[idx], truth)
        rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
        print("mode %d: refit vs rebuild median %.1e p99 %.1e | vs periodic direct sum: refit rms %.2e, rebuild rms %.2e | ia %.0f vs %.0f"
              % (mode, np.median(d), np.percentile(d, 99), rms(e_refit), rms(e_fresh), c2.mean(), c3.mean()))
        assert np.median(d) < 1e-2 and np.percentile(d, 99) < 0.1    # two valid approximations (walk error ~1e-2 at this size)
        assert rms(e_refit) < 1.3 * rms(e_fresh) + 1e-3


def test_reach_pretest_fp32_and_exact_paths_agree(pkg, O):
    """the evaluation kernel pre-selects pairs within reach in packed fp32 (threshold widened by the rounding bound) and
    re-tests r2 < reach2 exactly in the force loop; with tuning walk_exact_reach=1 the selection itself is done in fp64.  Forces and
    interaction counts must be bit-identical (a pair the fp32 test lost would show up here)."""
    n, L, ng = 60000, 1.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=9)
    eps = L / (40 * n ** (1 / 3))
    res = []
    for exact in (0, 1):
        cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=32, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_GROUP)
        eng = _engine(pkg, cfg, pos, mass, typ, tuning={"walk_exact_reach": exact})
        eng.compute_accelerations(pm_step=True)
        acc, old, cost = eng.get_accel()
        eng.set_opening(0.0, 0.005)
        eng.set_old_acc(old)
        eng.gravity_tree()
        acc2, _, cost2 = eng.get_accel()
        eng.close()
        res.append((acc, cost, acc2, cost2))
    for a, b in zip(res[0], res[1]):
        assert np.array_equal(a, b)
    assert res[0][1].mean() > 100


def test_no_or_one_active_particle(pkg, O):
    """degenerate active sets (a step on which nothing, or a single particle, ends its timestep): no launch with an empty
    grid, nothing written for inactive particles, and the single target's force equals the all-active run's to walk accuracy"""
    n, L, ng = 20000, 1.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=4)
    eps = L / (40 * n ** (1 / 3))
    kw = dict(n_gravs=ng, periodic=1, pmgrid=32, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_GROUP)
    full = _engine(pkg, pkg.make_config(**kw), pos, mass, typ)
    full.compute_accelerations(pm_step=True)
    a_full, _, _ = full.get_accel()
    full.close()
    for k in (0, 1):
        active = np.zeros(n, dtype=np.uint8)
        active[:k] = 1
        eng = _engine(pkg, pkg.make_config(**kw), pos, mass, typ, active=active)
        eng.compute_accelerations(pm_step=True)
        acc, old, cost = eng.get_accel()
        st = eng.stats()
        eng.close()
        assert st.n_active == k
        assert np.all(acc[k:] == 0) and np.all(cost[k:] == 0)
        if k:
            assert rel_err(acc[:1], a_full[:1]).max() < 2e-2 and cost[0] > 0


def test_group_walk_unequal_softenings(pkg, O):
    """UNEQUALSOFTENINGS with really different lengths per type (pair softening = max of the two, forcetree.c:1415-1417;
    nodes with mixed softenings are opened inside the larger one, :1488-1499): the group walk's general paths (per-item
    type / flag lookups, per-pair softening in the force loop) against the strict walk and the periodic direct sum"""
    n, L, ng = 30000, 1.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=12)
    sp = L / n ** (1 / 3)
    soft = [0.0, 0.5 * sp, 0.1 * sp, 0.5 * sp, 0.5 * sp, 0.5 * sp]       # type 1: half a spacing, type 2: a tenth
    kw = dict(n_gravs=ng, periodic=1, pmgrid=32, box_size=L, G=1.0, theta=0.5, softening=soft,
              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4")
    idx = np.arange(0, n, 60, dtype=np.int32)
    out = {}
    for mode in (pkg.WALK_STRICT, pkg.WALK_GROUP):
        eng = _engine(pkg, pkg.make_config(walk_mode=mode, **kw), pos, mass, typ)
        eng.compute_accelerations(pm_step=True)
        _, old, _ = eng.get_accel()
        eng.set_opening(0.0, 0.005)
        eng.set_old_acc(old)
        eng.compute_accelerations(pm_step=True)
        acc, _, cost, pm = eng.get_accel(want_pm=True)
        truth = eng.direct_sum(idx)
        eng.close()
        out[mode] = (acc + pm, cost, truth)
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))
    assert rel_err(out[pkg.WALK_STRICT][2], out[pkg.WALK_GROUP][2]).max() < 1e-12      # same direct sum
    e_s = rel_err(out[pkg.WALK_STRICT][0][idx], out[pkg.WALK_STRICT][2])
    e_g = rel_err(out[pkg.WALK_GROUP][0][idx], out[pkg.WALK_GROUP][2])
    d = rel_err(out[pkg.WALK_GROUP][0], out[pkg.WALK_STRICT][0])
    print("unequal softenings: strict rms %.2e, group rms %.2e vs periodic direct sum; group vs strict median %.1e; ia %.0f / %.0f"
          % (rms(e_s), rms(e_g), np.median(d), out[pkg.WALK_STRICT][1].mean(), out[pkg.WALK_GROUP][1].mean()))
    assert rms(e_g) <= 1.05 * rms(e_s) + 1e-3 and np.median(d) < 1e-2


@pytest.mark.gpu
@pytest.mark.parametrize("wiring,ng,pmgrid,soft,every", [
    pytest.param(*c, id="%s-%d-%d-%s" % c[:4] + ("-every%d" % c[4] if c[4] else "")) for c in
    [("newton", 1, 32, "one", 0), ("newton", 1, 256, "one", 0), ("c4", 2, 64, "one", 0), ("c4", 2, 256, "one", 0), ("c4", 3, 256, "one", 0),
     ("c4", 2, 256, "two", 0), ("newton", 1, 256, "two", 0), ("c4", 2, 16, "one", 33)]])
def test_ring_pool_kernel_is_the_synchronous_kernel(pkg, wiring, ng, pmgrid, soft, every):
    """The ring-pool evaluation kernel (kernels_eval.hip: per-lane cursors, trip loop / cull in assembly) against the synchronous one
    (k_walk_group2<..., 2>, tuning walk_ring = 0) on the same item lists: identical interaction counts for every particle, forces to
    rounding (the two sum a target's pairs in different orders).  The cases walk through the kernel's variants: with / without a
    Yukawa law, the Yukawa factor through the table bins (PMGRID 256: ym * bin width < 1e-3) or through exp(), one softening length
    (assembly cull) or two (type bytes), both opening criteria, 5 / 6 / 4 ring slots.  (PMGRID 256 without a Yukawa law is the C3
    bench's case: its exp table is not staged, the softening lengths sit right behind the tables.)
    every 33: every 33rd particle is active and PMGRID is 16, so that the walk compacts the targets and most groups of 64 of them
    span a box too wide to wrap the sources once per group (bhmax >= boxhalf - reach): the per-pair image branch of the wrap
    decision the kernels share, in the ring kernel, the synchronous one and the fused one (walk_fused 1), one lane per target."""
    n, L = 60000, 1.0
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=91)
    pos[: n // 3] = np.mod(0.4 + 0.04 * np.random.default_rng(5).standard_normal((n // 3, 3)), 1.0)   # a clump: softened pairs
    eps = L / (40 * n ** (1 / 3))
    softening = [eps] * 6 if soft == "one" else [eps, eps, 2.5 * eps, eps, 1.7 * eps, eps]
    out = {}
    variants = [("sync", {"walk_ring": 0}), ("ring", {}), ("ring4", {"walk_ring_k": 4})]
    active = None
    if every:
        active = np.zeros(n, dtype=np.uint8)
        active[::every] = 1
        # (lists as long as a unit's can get: no group is left to the leftover pass, which is the fused kernel's)
        base = {"walk_spread": 1, "walk_lcap": 65536}
        variants = [("sync", dict(base, walk_ring=0)), ("ring", base), ("fused", dict(base, walk_fused=1))]
    if (wiring, ng, pmgrid, soft) == ("c4", 2, 256, "two"):
        # two / four lanes per target (walk_spread: what the library chooses for strongly clustered sets): the S lanes of a target share the
        # entries of every block, each against the synchronous kernel with the same spread
        variants += [("sync_s2", {"walk_ring": 0, "walk_spread": 2}), ("ring_s2", {"walk_spread": 2}),
                     ("sync_s4", {"walk_ring": 0, "walk_spread": 4}), ("ring_s4", {"walk_spread": 4})]
    for name, tune in variants:
        cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=1.0, theta=0.5, softening=softening,
                              type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_GROUP)
        eng = _engine(pkg, cfg, pos, mass, typ, tuning=tune, active=active)
        eng.compute_accelerations(pm_step=True)
        a1, o1, c1 = eng.get_accel()
        if every and name == "sync":
            # the case is about groups with a wide box: the share of them among the groups of 64 compacted targets
            t = eng.order()
            t = t[active[t] != 0]
            reach = 4.5 * pkg.abi.ASMTH * L / pmgrid   # (4.5: NGRAVS_GROUP_REACH of ngravs_hip.h, the default group_reach)
            wide = [0.5 * np.ptp(pos[t[k:k + 64]], axis=0).max() >= 0.5 * L - reach for k in range(0, len(t), 64)]
            print("sparse: %d active targets, %d groups, %.2f of them with bhmax >= boxhalf - reach" % (len(t), len(wide), np.mean(wide)))
            assert np.mean(wide) >= 0.5
        eng.set_old_acc(o1)
        eng.set_opening(0.0, 0.005)
        eng.gravity_tree()
        a2, _, c2 = eng.get_accel()
        out[name] = (a1, c1, a2, c2, eng.stats().reserved[3])
        eng.close()
    pairs = [("ring", "sync"), ("ring4", "sync")] + [(v[0], "sync" + v[0][4:]) for v in variants if v[0].startswith("ring_s")]
    if every:
        pairs = [("ring", "sync"), ("fused", "sync")]
    for name, ref in pairs:
        r, s = out[name], out[ref]
        rows = slice(None) if active is None else active != 0     # (inactive rows: all zero, asserted below)
        for k in (0, 2):
            na = np.linalg.norm(s[k][rows], axis=1)       # (a particle with nothing inside the cut has no short-range force at all)
            e = np.linalg.norm((r[k] - s[k])[rows], axis=1) / np.maximum(na, 1e-6 * np.median(na))
            print("%s %s ng %d pmgrid %d %s: pass %d max |da|/|a| %.1e, trips per group %.1f (synchronous %.1f)" %
                  (name, wiring, ng, pmgrid, soft, k // 2 + 1, e.max(), r[4], s[4]))
            assert np.array_equal(r[k + 1], s[k + 1])
            assert e.max() < 1e-11
            if active is not None:
                assert np.all(r[k][active == 0] == 0) and np.all(s[k][active == 0] == 0) and np.all(s[k + 1][active == 0] == 0)
                assert np.all(s[k + 1][active != 0] > 0)
        if name != "fused":   # (the fused kernel evaluates in synchronous blocks too)
            assert r[4] < s[4]
