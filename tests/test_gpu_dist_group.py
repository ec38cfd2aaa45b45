"""-m gpu: the multi-task GROUP walk (the production walk; the path behind bench.py --gpus N) held to the single task pair for pair.

On N tasks a group is a stretch of one task's own particles, so the production walk's groups differ from the single task's and
test_gpu_dist.py can only bound the group walk statistically.  Two ways of taking the grouping out of the comparison do not
depend on how targets are grouped, so they must hold unchanged on any number of tasks:
  * one target per wave (walk_spread 64, no leaf shortcut, walk started at the root, one group per unit): every conservative
    group test is the target's own test, so N tasks must give the single task's forces and counts to rounding -- and no walk may
    want a top leaf that was never imported (walk_unopened() == 0 on every task);
  * the production walk, nothing tuned, at bench density: the sum of the reference's short-range pair force over every particle
    within RCUT * Asmth, target for target, as on one task (test_gpu_parity.py::test_production_walk_is_the_cut_direct_sum).
Gloo process groups, every task on the one GPU of the box, at most 5 tasks."""
import os
import sys

import numpy as np
import pytest

from test_gpu_dist import LEAF_MAX, NKEPT, _degenerate_case, _kept_positions, _strict_case

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

ONE_TARGET = {"walk_spread": 64, "walk_nleaf": 0, "walk_root": 1, "walk_sg": 1}
DEGENERATE = ("two", "tiny", "clump", "slab", "clump_tree")


def _init(rank, world, port):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    import importlib
    import torch.distributed as dist
    import __graft_entry__ as ge
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    return pkg, importlib.import_module("ngravs_amd.distributed"), dist


def _merge(out_dir, prefix, world, n, keys, suffix=""):
    """rows of all tasks by particle id; every particle must be owned exactly once"""
    res = [np.load(os.path.join(out_dir, "%s%d.npz" % (prefix, r))) for r in range(world)]
    seen = np.zeros(n, dtype=np.int64)
    out = {}
    for d in res:
        ids = d["ids" + suffix]
        seen[ids] += 1
        for k in keys:
            v = d[k + suffix]
            if k not in out:
                out[k] = np.zeros((n,) + v.shape[1:], dtype=v.dtype)
            out[k][ids] = v
    assert np.all(seen == 1)
    return out, res


def _rel(a, b):
    return np.linalg.norm(a - b, axis=1) / np.maximum(np.linalg.norm(b, axis=1), 1e-300)


# ---- 1. one target per wave on N tasks ----------------------------------------------------------------------------------------

def _one_target_case(pkg, case, mode):
    """(pos, mass, typ, old, active, cfg, leaf_max, steps) of a case; mode "group": one-target group walk, "strict": reference walk.
    steps: the pm_step flag of each step (two steps, c4 with a following non-PM step)"""
    active = None
    if case in DEGENERATE:
        pos, mass, typ, cfg = _degenerate_case(pkg, case)
        old, leaf_max = np.zeros(len(pos)), 40.0
    else:
        base = "c4" if case == "sparse" else case
        pos, mass, typ, old, cfg = _strict_case(pkg, base)
        leaf_max = LEAF_MAX.get(base)
        if case == "sparse":
            active = (np.arange(len(pos)) % 7 == 3).astype(np.uint8)
    if mode == "group":
        cfg.walk_mode = pkg.WALK_GROUP
        if cfg.pmgrid:
            cfg.group_reach = 6.0          # the cut at the end of the short-range table: the reference's own cut
    pm = bool(cfg.pmgrid)
    steps = [pm, pm] + ([False] if case == "c4" else [])
    return pos, mass, typ, old, active, cfg, leaf_max, steps


def _one_target_worker(rank, world, port, out_dir, case):
    pkg, dd, dist = _init(rank, world, port)
    pos, mass, typ, old, active, cfg, leaf_max, steps = _one_target_case(pkg, case, "group")
    n = len(pos)
    if case in DEGENERATE:
        mine = np.arange(n) if rank == 0 else np.zeros(0, dtype=np.int64)     # one task holds everything, the others start EMPTY
    else:
        mine = np.arange(rank, n, world)
    eng = dd.DistributedEngine(cfg, leaf_max=leaf_max)
    eng.set_tuning(**ONE_TARGET)
    eng.set_particles(pos[mine], mass[mine], typ[mine], old_acc=old[mine], ids=mine,
                      active=None if active is None else active[mine])
    out = {}
    for s, pm_step in enumerate(steps):       # the second step's cut is weighted by the first step's GravCost
        eng.compute_accelerations(pm_step=pm_step)
        a, o, c = eng.get_accel()
        p = eng.get_accel(want_pm=True)[3] if cfg.pmgrid else np.zeros_like(a)
        out.update({"ids%d" % s: eng.local_ids(), "acc%d" % s: a, "old%d" % s: o, "cost%d" % s: c, "pm%d" % s: p,
                    "unop%d" % s: np.array([eng.walk_unopened(), eng.timings["halo"]])})
    np.savez(os.path.join(out_dir, "t%d.npz" % rank), **out)
    eng.close()
    dist.destroy_process_group()


def _single_task(pkg, case, mode):
    pos, mass, typ, old, active, cfg, _, steps = _one_target_case(pkg, case, mode)
    eng = pkg.Engine(cfg)
    if mode == "group":
        eng.set_tuning(**ONE_TARGET)
    eng.set_particles(pos, mass, typ, old_acc=old, active=active)
    res = []
    for pm_step in steps:
        eng.compute_accelerations(pm_step=pm_step)
        a, o, c = eng.get_accel()
        res.append((a, o, c, eng.get_accel(want_pm=True)[3] if cfg.pmgrid else np.zeros_like(a)))
    eng.close()
    return res


@pytest.mark.parametrize("case,world", [("c4", 2), ("c4", 3), ("c3", 3), ("c5", 3), ("plummer", 5), ("periodic", 3),
                                        ("two", 3), ("tiny", 3), ("clump", 3), ("slab", 3), ("clump_tree", 3), ("sparse", 3)])
def test_one_target_group_walk_is_the_single_task(pkg, tmp_path, case, world):
    """One target per wave: (a) the single task's one-target group walk to rounding -- identical GravCost for every particle,
    max |da|/|a| < 1e-10, GravPM and OldAcc within 1e-10 -- on every step; (b) where one task's one-target walk IS the reference
    walk (TreePM with the cut at the table end, tree-only non-periodic), the single task's reference walk as well: forces within
    1e-10, and for one species identical counts (more species: the group walk counts a node once per source species that holds
    mass in it).  The periodic tree-only case (lattice walk) reports (b) without asserting it.  On every task and after every
    walk, walk_unopened() == 0: with one target per group the import decision covers every node a walk opens."""
    import torch.multiprocessing as mp
    port = 24100 + (os.getpid() % 1000)
    mp.spawn(_one_target_worker, args=(world, port, str(tmp_path), case), nprocs=world, join=True)
    pos, mass, typ, old, active, cfg, _, steps = _one_target_case(pkg, case, "group")
    n = len(pos)
    act = np.ones(n, dtype=bool) if active is None else active.astype(bool)
    one = _single_task(pkg, case, "group")
    ref = _single_task(pkg, case, "strict")
    check_ref = case != "periodic"
    for s, pm_step in enumerate(steps):
        m, res = _merge(str(tmp_path), "t", world, n, ("acc", "old", "cost", "pm"), str(s))
        a1, o1, c1, p1 = one[s]
        ar, _, cr, _ = ref[s]
        unop = [int(d["unop%d" % s][0]) for d in res]
        err = _rel(m["acc"][act], a1[act])
        err_ref = _rel(m["acc"][act], ar[act])
        eo = np.abs(m["old"] - o1).max() / o1.max()
        epm = np.abs(m["pm"] - p1).max() / np.abs(p1).max() if cfg.pmgrid else 0.0
        print("%s on %d tasks, step %d (%s): imported %s, walk_unopened %s; vs one task's one-target walk: max |da|/|a| %.1e, counts "
              "equal %s, OldAcc %.1e, GravPM %.1e; vs one task's reference walk: max |da|/|a| %.1e, counts equal %s" %
              (case, world, s, "PM" if pm_step else "no PM", [int(d["unop%d" % s][1]) for d in res], unop, err.max(),
               np.array_equal(m["cost"], c1), eo, epm, err_ref.max(), np.array_equal(m["cost"][act], cr[act])))
        assert unop == [0] * world
        assert np.array_equal(m["cost"], c1)
        assert err.max() < 1e-10 and eo < 1e-10 and epm < 1e-10
        if active is not None:      # rows not walked: no force, no cost, the OldAcc handed over
            assert np.all(m["acc"][~act] == 0) and np.all(m["cost"][~act] == 0)
            assert np.array_equal(m["old"][~act], old[~act])
        if check_ref:
            assert err_ref.max() < 1e-10
            if cfg.n_gravs == 1:
                assert np.array_equal(m["cost"][act], cr[act])
            else:
                assert np.all(m["cost"][act] >= cr[act])


# ---- 2. kept steps with the one-target group walk ----------------------------------------------------------------------------

def _kept_case(pkg, case):
    pos, mass, typ, old, cfg = _strict_case(pkg, case)
    cfg.walk_mode = pkg.WALK_GROUP
    if cfg.pmgrid:
        cfg.group_reach = 6.0
    return pos, mass, typ, old, cfg


def _kept_group_worker(rank, world, port, out_dir, case):
    pkg, dd, dist = _init(rank, world, port)
    pos0, mass, typ, old0, cfg = _kept_case(pkg, case)
    n, L = len(pos0), cfg.box_size if cfg.periodic else 0.0
    eng = dd.DistributedEngine(cfg, leaf_max=300.0)
    eng.set_tuning(**ONE_TARGET)
    ids = np.arange(rank, n, world)
    eng.set_particles(pos0[ids], mass[ids], typ[ids], old_acc=old0[ids], ids=ids)
    eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
    ids = eng.local_ids()
    a, o, c = eng.get_accel()[:3]
    out = {"ids": ids, "acc0": a, "cost0": c, "old0": o, "unop0": np.array([eng.walk_unopened()])}
    for step in range(1, NKEPT):
        pos = _kept_positions(pos0, L, step)
        eng.kept_step(pos[ids], mass[ids], typ[ids], old_acc=o)
        eng.gravity_tree()
        missed = eng.kept_walk_missed()                                 # (collective)
        a, o, c = eng.get_accel()[:3]
        out.update({"acc%d" % step: a, "cost%d" % step: c, "old%d" % step: o, "unop%d" % step: np.array([eng.walk_unopened()]),
                    "missed%d" % step: np.array([missed]), "same%d" % step: np.array([np.array_equal(eng.local_ids(), ids)])})
    np.savez(os.path.join(out_dir, "kg%d.npz" % rank), **out)
    eng.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("case", ["c4", "plummer"])
def test_kept_decomposition_one_target_group_walk(pkg, tmp_path, case):
    """Steps that keep the decomposition, walked by the group walk with one target per wave on three tasks: no task's walk wants a
    leaf that was never imported, nothing migrates, and forces, OldAcc and counts are those of the single task's refit tree
    (update_particles + gravity_tree, the same tuning) -- so the refit pseudo nodes (global moments and sides of the top nodes
    after ngravs_host_kept_step) must be the single task's nodes.  With the cut at the table end every top leaf a TreePM target
    can reach is imported, so in c4 no pseudo node enters a force; the tree-only Plummer sphere is the case that uses their
    moments."""
    import torch.multiprocessing as mp
    world = 3
    port = 25100 + (os.getpid() % 1000)
    mp.spawn(_kept_group_worker, args=(world, port, str(tmp_path), case), nprocs=world, join=True)
    pos0, mass, typ, old0, cfg = _kept_case(pkg, case)
    n, L = len(pos0), cfg.box_size if cfg.periodic else 0.0
    eng = pkg.Engine(cfg)
    eng.set_tuning(**ONE_TARGET)
    eng.set_particles(pos0, mass, typ, old_acc=old0)
    eng.compute_accelerations(pm_step=bool(cfg.pmgrid))
    a1, o1, c1 = eng.get_accel()[:3]
    for step in range(NKEPT):
        if step > 0:
            eng.update_particles(_kept_positions(pos0, L, step), mass, typ, old_acc=o1)
            eng.gravity_tree()
            a1, o1, c1 = eng.get_accel()[:3]
        m, res = _merge(str(tmp_path), "kg", world, n, ("acc%d" % step, "old%d" % step, "cost%d" % step))
        acc, oa, cost = m["acc%d" % step], m["old%d" % step], m["cost%d" % step]
        err = _rel(acc, a1)
        unop = [int(d["unop%d" % step][0]) for d in res]
        print("%s step %d (%s): walk_unopened %s; counts equal %s; |da|/|a| max %.1e; OldAcc %.1e" %
              (case, step, "decomposition" if step == 0 else "kept", unop, np.array_equal(cost, c1), err.max(),
               np.abs(oa - o1).max() / o1.max()))
        assert unop == [0] * world
        if step > 0:
            assert not any(bool(d["missed%d" % step][0]) for d in res)
            assert all(bool(d["same%d" % step][0]) for d in res)
        assert np.array_equal(cost, c1) and err.max() < 1e-10 and np.abs(oa - o1).max() < 1e-10 * o1.max()
    eng.close()


# ---- 3. the production walk on N tasks against the cut direct sum ------------------------------------------------------------

def _cut_case(pkg, ng):
    n, L, pmgrid = 1 << 17, 1.0, 64                               # 2 mesh cells per particle, as C4 / C5
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=123)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=pmgrid, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4", walk_mode=pkg.WALK_GROUP)
    return pos, mass, typ, cfg


def _two_passes(eng):
    """theta pass for OldAcc, then the bench's steady-state relative criterion with it"""
    eng.compute_accelerations(pm_step=True)
    unop = [eng.walk_unopened()]
    _, old, _ = eng.get_accel()
    eng.set_old_acc(old)
    eng.set_opening(0.0, 0.005)
    eng.compute_accelerations(pm_step=True)
    unop.append(eng.walk_unopened())
    acc, _, cost = eng.get_accel()
    return acc, cost, unop


def _cut_worker(rank, world, port, out_dir, ng):
    pkg, dd, dist = _init(rank, world, port)
    pos, mass, typ, cfg = _cut_case(pkg, ng)
    mine = np.arange(rank, len(pos), world)
    eng = dd.DistributedEngine(cfg)
    eng.set_particles(pos[mine], mass[mine], typ[mine], ids=mine)
    acc, cost, unop = _two_passes(eng)
    np.savez(os.path.join(out_dir, "d%d.npz" % rank), ids=eng.local_ids(), acc=acc, cost=cost, unop=np.array(unop))
    eng.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("ng,world", [(2, 3), (3, 3), (2, 5)])
def test_production_walk_on_several_tasks_is_the_cut_direct_sum(pkg, O, tmp_path, ng, world):
    """The production walk, nothing tuned, on several tasks (5 tasks: uneven mesh slabs) against the exact quantity of the single-task
    test: the reference's short-range pair force summed over every particle of the GLOBAL set within RCUT * Asmth -- identical counts
    and forces to rounding for >= 97 % of 512 sampled targets, the rest (a cell at the edge of the cut taken as one monopole) within
    2e-3, the mean count within 1 %, and no fewer exact targets than the single task gets on the same sample.  walk_unopened() is
    printed: a multi-leaf group's box is conservative, so it may be non-zero here; a real miss shows pair for pair."""
    import torch.multiprocessing as mp
    port = 26100 + (os.getpid() % 1000)
    mp.spawn(_cut_worker, args=(world, port, str(tmp_path), ng), nprocs=world, join=True)
    pos, mass, typ, cfg = _cut_case(pkg, ng)
    n = len(pos)
    m, res = _merge(str(tmp_path), "d", world, n, ("acc", "cost"))
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    a1, c1, _ = _two_passes(eng)
    eng.close()
    idx = np.sort(np.random.default_rng(11).choice(n, 512, replace=False)).astype(np.int32)
    tab, _ = O.shortrange_table(cfg)
    a_o, n_o = O.direct_shortrange(cfg, pos, mass, typ, idx, tab, 4.5 * 1.25 * cfg.box_size / cfg.pmgrid)
    n_o = n_o.astype(np.int64)

    def shares(acc, cost):
        err = np.linalg.norm(acc[idx] / cfg.G - a_o, axis=1) / np.linalg.norm(a_o, axis=1)
        return err, np.mean(cost[idx].astype(np.int64) == n_o), np.mean(err < 1e-10)

    err, same, exact = shares(m["acc"], m["cost"])
    _, same1, exact1 = shares(a1, c1)
    print("production walk on %d tasks vs cut direct sum [N_GRAVS=%d]: %.1f (oracle %.1f) pairs/target; counts equal %.4f (one task "
          "%.4f), exact %.4f (one task %.4f); the others: max %.1e; walk_unopened per task (theta pass, relative pass) %s" %
          (world, ng, m["cost"][idx].mean(), n_o.mean(), same, same1, exact, exact1, err.max(), [d["unop"].tolist() for d in res]))
    assert same > 0.97 and exact > 0.97
    assert err.max() < 2e-3
    assert abs(m["cost"][idx].mean() - n_o.mean()) < 0.01 * n_o.mean()
    assert exact >= exact1 - 0.01
