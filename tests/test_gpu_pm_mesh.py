"""-m gpu: the periodic PM force at mesh sizes that are NOT powers of two, against tests/pm_reference.py (numpy fp64, any N;
pinned to the oracle and to explicit DFT matrices by tests/test_pm_reference.py).

The oracle's pmforce_periodic only knows PMGRID = 2^k, so every other PM test sees N = 16, 32, 64 (all tiles of every kernel
full, one x-block of the force-mesh march, no edge tile in the slab transposes).  Real runs use 96, 192, 384, 768.  Here:
the force-mesh march with full and partial (z, y) tiles in one launch, several x-blocks and a last x-block shorter than the
stencil; the slab transposes with edge tiles; the three deposit paths (tiles, loose particles, no tile level at all) and the
direct-atomic branch of a refit tree whose cells outgrew their patches; the fused gather of world_size > 2; the slab path on
one, three and five tasks; and the TreePM total at N = 48 between N = 32 and N = 64.

Tolerance: 1e-10 of max |GravPM| against the truth (TOL of test_gpu_parity.py: summation order / exp / FFT rounding only);
1e-12 between two kernels of ours that evaluate the same expressions in another order.
"""
import os
import sys

import numpy as np
import pytest

import pm_reference
from conftest import rel_err

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TOL = 1e-10          # kernel vs truth
SAME = 1e-12         # kernel vs kernel, same expressions


def _config(pkg, wiring, ng, N, L, **kw):
    n_eps = kw.pop("n_eps", 20000)
    eps = L / (40 * n_eps ** (1 / 3))
    return pkg.make_config(n_gravs=ng, periodic=1, pmgrid=N, box_size=L, G=43007.1 if L > 1 else 1.7, theta=0.5,
                           softening=[eps] * 6, type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, **kw)


BOX = {12: 1e4, 20: 1.0, 36: 1e4, 48: 1.0, 80: 1e4, 96: 1.0, 130: 1e4}


def _box_of(N):
    """half of the cases in a box of 1e4, the others in a unit box"""
    return BOX[N]


def _standard(pkg, n, L, ng, N, seed):
    """uniform box with a third squeezed into a clump; rows 0..5: the origin, (L, L, L), L(1 - 2^-53), a cell corner, and a pair
    that straddles the periodic seam in z"""
    pos, _, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=seed)
    pos[: n // 3] = 0.2 * L + 0.3 * (pos[: n // 3] - 0.2 * L)
    pos[0] = 0.0
    pos[1] = L
    pos[2] = L * (1 - 2.0 ** -53)
    pos[3] = (3 * L / N, 0.0, (N - 1) * L / N)
    pos[4] = (0.61 * L, 0.37 * L, L * (1 - 1e-9))
    pos[5] = (0.61 * L, 0.37 * L, 1e-9 * L)
    mass = np.random.default_rng(seed + 1000).uniform(0.5, 1.5, n) / n
    return pos, mass, typ


def _gpu_pm(pkg, cfg, pos, mass, typ):
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.pmforce_periodic()
    pm = eng.get_pm()
    eng.close()
    return pm


def _err(a, b):
    return np.abs(a - b).max() / np.abs(b).max()


# N: 12 the root is the tile, patch origin -1 | 20 partial y tile, z < 32 | 36, 48 full + partial z tiles in one launch |
# 80 two x-blocks + partial z tile | 96 x-blocks 64 + 32, all tiles full | 130 N % 8 = 2, x-blocks 64 + 64 + 2
SWEEP = [(N, "c4", 2) for N in (12, 20, 36, 48, 80, 96, 130)] + \
        [(N, w, g) for N in (48, 80) for w, g in (("newton", 1), ("coloyuk", 2), ("yukawa_offdiag", 2), ("c4", 3))]


@pytest.mark.parametrize("N,wiring,ng", SWEEP)
def test_mesh_size_sweep(pkg, N, wiring, ng):
    n, L = 20000, _box_of(N)
    pos, mass, typ = _standard(pkg, n, L, ng, N, seed=300 + N)
    cfg = _config(pkg, wiring, ng, N, L)
    pm = _gpu_pm(pkg, cfg, pos, mass, typ)
    ref = pm_reference.pm_periodic(cfg, pos, mass, typ)
    err = _err(pm, ref)
    print("PM mesh sweep [%s/%d N=%d L=%g]: %.2e" % (wiring, ng, N, L, err))
    assert np.isfinite(pm).all()
    assert err < TOL


@pytest.mark.parametrize("case", ["octants_96", "sparse_130"])
def test_deposit_without_a_tile_level(pkg, case):
    """8 particles, one per octant: the tree has level 0 only, no level of cells <= 16 mesh cells, the deposit is one thread per
    particle.  300 particles at N = 130: the tile level is thinly populated, particles hang off the nodes above it (loose
    particles) beside the tiles."""
    if case == "octants_96":
        N, L, ng = 96, _box_of(96), 2
        rng = np.random.default_rng(5)
        corner = np.array([(i, j, k) for i in (0, 1) for j in (0, 1) for k in (0, 1)], dtype=float)
        pos = (corner * 0.5 + rng.uniform(0.05, 0.45, (8, 3))) * L
        mass = rng.uniform(0.5, 1.5, 8) / 8
        typ = (1 + np.arange(8) % ng).astype(np.int32)
    else:
        N, L, ng = 130, _box_of(130), 2
        pos, mass, typ = pkg.ic.uniform_box(300, box=L, n_gravs=ng, seed=17)
        mass = np.random.default_rng(18).uniform(0.5, 1.5, 300) / 300
    cfg = _config(pkg, "c4", ng, N, L)
    pm = _gpu_pm(pkg, cfg, pos, mass, typ)
    ref = pm_reference.pm_periodic(cfg, pos, mass, typ)
    err = _err(pm, ref)
    print("PM deposit without tiles [%s]: %.2e" % (case, err))
    assert np.isfinite(pm).all() and np.abs(pm).max() > 0
    assert err < TOL


def test_refit_tree_cells_overrun_their_patches(pkg):
    """update_particles keeps the tree; pmforce_periodic refits it, and cells that grew by up to 3 mesh cells a side no longer fit
    the 18^3 patch of the tiled deposit: those particles take the direct-atomic branch.  Truth at the new positions, and the
    same positions through set_particles on a fresh engine (only the summation order differs)."""
    N, n, ng = 48, 20000, 2
    L = _box_of(N)
    pos, mass, typ = _standard(pkg, n, L, ng, N, seed=41)
    cfg = _config(pkg, "c4", ng, N, L)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ)
    eng.domain_Decomposition()
    eng.pmforce_periodic()
    pm0 = eng.get_pm()
    rng = np.random.default_rng(42)
    new = np.mod(pos + rng.uniform(-3.0, 3.0, (n, 3)) * L / N, L)
    new[new >= L] = 0.0
    eng.update_particles(new, mass, typ)
    eng.pmforce_periodic()
    pm1 = eng.get_pm()
    eng.close()
    ref0 = pm_reference.pm_periodic(cfg, pos, mass, typ)
    ref1 = pm_reference.pm_periodic(cfg, new, mass, typ)
    fresh = _gpu_pm(pkg, cfg, new, mass, typ)
    print("PM on a refit tree N=%d: before %.2e, after the move %.2e, refit vs fresh build %.2e" %
          (N, _err(pm0, ref0), _err(pm1, ref1), _err(pm1, fresh)))
    assert _err(pm0, ref0) < TOL
    assert _err(pm1, ref1) < TOL
    assert _err(pm1, fresh) < SAME


@pytest.mark.parametrize("where", ["inner", "last"])
@pytest.mark.parametrize("N", [20, 80])
def test_everything_in_one_cell(pkg, N, where):
    """5000 particles inside ONE mesh cell -- an inner one, or the last cell (N-1, N-1, N-1), all eight corners of which wrap --
    plus 100 spread-out particles so that the force scale is not degenerate"""
    L, ng, n = _box_of(N), 2, 5100
    rng = np.random.default_rng(60 + N)
    cell = np.array([3, N // 2, N - 2] if where == "inner" else [N - 1, N - 1, N - 1], dtype=float)
    pos = np.empty((n, 3))
    pos[:5000] = (cell + rng.uniform(0.001, 0.999, (5000, 3))) * L / N
    pos[5000:] = rng.uniform(0, L, (100, 3))
    pos = np.minimum(pos, L * (1 - 2.0 ** -53))
    mass = rng.uniform(0.5, 1.5, n) / n
    typ = (1 + np.arange(n) % ng).astype(np.int32)
    cfg = _config(pkg, "c4", ng, N, L)
    pm = _gpu_pm(pkg, cfg, pos, mass, typ)
    ref = pm_reference.pm_periodic(cfg, pos, mass, typ)
    err = _err(pm, ref)
    print("PM with 5000 particles in the %s cell, N=%d: %.2e" % (where, N, err))
    assert np.isfinite(pm).all()
    assert err < TOL


@pytest.mark.parametrize("N", [20, 80])
def test_fused_gather_of_three_shards(pkg, N):
    """world_size > 2 without slabs: every task gathers its target shard with the fused gradient + gather kernel instead of the
    force mesh + gather of one or two tasks.  Same expressions: the merged shards are the single-task GravPM to rounding."""
    n, ng, L = 20000, 2, _box_of(N)
    pos, mass, typ = _standard(pkg, n, L, ng, N, seed=80 + N)
    single = _gpu_pm(pkg, _config(pkg, "c4", ng, N, L), pos, mass, typ)
    merged, seen = np.zeros_like(single), np.zeros(n, dtype=np.int64)
    for r in range(3):
        eng = pkg.Engine(_config(pkg, "c4", ng, N, L, rank=r, world_size=3))
        eng.set_particles(pos, mass, typ)
        eng.domain_Decomposition()
        eng.pmforce_periodic()
        pm = eng.get_pm()
        first, count = eng.shard()
        assert (first, count) == pkg.shard_range(n, r, 3)
        o = eng.order()[first:first + count]
        eng.close()
        assert np.all(np.delete(pm, o, axis=0) == 0)          # rows outside the shard: exactly zero
        merged[o] = pm[o]
        seen[o] += 1
    assert np.all(seen == 1)
    ref = pm_reference.pm_periodic(_config(pkg, "c4", ng, N, L), pos, mass, typ)
    print("PM fused gather, 3 shards, N=%d: vs two-pass gather %.2e, vs truth %.2e" % (N, _err(merged, single), _err(merged, ref)))
    assert _err(merged, single) < SAME
    assert _err(merged, ref) < TOL


@pytest.mark.parametrize("N", [20, 48, 80])
def test_slab_path_one_task(pkg, N):
    """the slab-decomposed mesh (brick deposit, plane exchanges, 2-D + 1-D FFTs, Green's function on the transposed layout, brick
    gather) on ONE task, where the 32 x 32 tiles of the k-space transposes have edge tiles in x (N % 32 != 0)"""
    import importlib
    import torch.distributed as dist
    dd = importlib.import_module("ngravs_amd.distributed")
    if not dist.is_initialized():
        dist.init_process_group("gloo", init_method="tcp://127.0.0.1:%d" % (29400 + os.getpid() % 500), rank=0, world_size=1)
    n, ng, L = 20000, 2, _box_of(N)
    pos, mass, typ = _standard(pkg, n, L, ng, N, seed=120 + N)
    plain = _gpu_pm(pkg, _config(pkg, "c4", ng, N, L, walk_mode=pkg.WALK_GROUP), pos, mass, typ)
    deng = dd.DistributedEngine(_config(pkg, "c4", ng, N, L, walk_mode=pkg.WALK_GROUP))
    deng.set_particles(pos, mass, typ)
    deng.domain_Decomposition()
    deng.pmforce_periodic()
    deng.n = deng.num_local()
    pm_slab = deng.get_pm()
    ids = deng.local_ids()
    deng.close()
    full = np.zeros_like(plain)
    full[ids] = pm_slab
    ref = pm_reference.pm_periodic(_config(pkg, "c4", ng, N, L), pos, mass, typ)
    print("slab PM on one task, N=%d: vs 3-D transform %.2e, vs truth %.2e" % (N, _err(full, plain), _err(full, ref)))
    assert len(ids) == n
    assert _err(full, plain) < SAME
    assert _err(full, ref) < TOL


def _slab_case(pkg, N):
    n, ng, L = 12000, 2, _box_of(N)
    pos, mass, typ = _standard(pkg, n, L, ng, N, seed=150 + N)
    return pos, mass, typ, _config(pkg, "c4", ng, N, L, walk_mode=pkg.WALK_GROUP, n_eps=n)


def _slab_worker(rank, world, port, out_dir, N):
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    import importlib
    import torch.distributed as dist
    import __graft_entry__ as ge
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    dd = importlib.import_module("ngravs_amd.distributed")
    pos, mass, typ, cfg = _slab_case(pkg, N)
    mine = np.arange(rank, len(pos), world)
    eng = dd.DistributedEngine(cfg)
    eng.set_particles(pos[mine], mass[mine], typ[mine], ids=mine)
    eng.compute_accelerations(pm_step=True)
    pm = eng.get_accel(want_pm=True)[3]
    np.savez(os.path.join(out_dir, "m%d.npz" % rank), ids=eng.local_ids(), pm=pm)
    eng.close()
    dist.destroy_process_group()


@pytest.mark.parametrize("world,N", [(3, 20), (5, 48)])
def test_slab_path_several_tasks(pkg, tmp_path, world, N):
    """x-slabs of uneven width (20 planes on 3 tasks: 6 + 7 + 7; 48 on 5: 9 + 10 + 9 + 10 + 10), every task's rows spread over the
    whole box: the merged GravPM is the truth"""
    import torch.multiprocessing as mp
    port = 31200 + (os.getpid() % 2000) + world
    mp.spawn(_slab_worker, args=(world, port, str(tmp_path), N), nprocs=world, join=True)
    pos, mass, typ, cfg = _slab_case(pkg, N)
    n = len(pos)
    pm, seen = np.zeros((n, 3)), np.zeros(n, dtype=np.int64)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "m%d.npz" % r))
        pm[d["ids"]] = d["pm"]
        seen[d["ids"]] += 1
    assert np.all(seen == 1)
    ref = pm_reference.pm_periodic(cfg, pos, mass, typ)
    err = _err(pm, ref)
    print("slab PM on %d tasks, N=%d: %.2e" % (world, N, err))
    assert err < TOL


def test_treepm_total_at_a_mesh_that_is_no_power_of_two(pkg):
    """asmth, rcut and the short-range table must follow N: the TreePM total (reference walk, relative criterion after one
    Barnes-Hut pass) against the periodic direct sum of 600 targets, on the same particles at N = 32, 48 and 64.  The error of
    the force split is set by asmth and rcut in mesh units, independent of N to first order, so N = 48 must lie with its
    neighbours (1.5: sampling noise of 600 targets) and inside the absolute band of test_group_walk_treepm_accuracy_vs_ewald."""
    n, ng, L = 20000, 2, 1.0
    pos, _, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=201)
    pos[: n // 3] = 0.2 * L + 0.3 * (pos[: n // 3] - 0.2 * L)
    mass = np.random.default_rng(202).uniform(0.5, 1.5, n) / n
    idx = np.arange(0, n, n // 600, dtype=np.int32)[:600]
    rms, truth = {}, None
    for N in (32, 48, 64):
        eng = pkg.Engine(_config(pkg, "c4", ng, N, L, walk_mode=pkg.WALK_STRICT))
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=True)
        _, old, _ = eng.get_accel()
        eng.set_old_acc(old)
        eng.set_opening(0.0, 0.005)
        eng.gravity_tree()
        acc, _, _, pm = eng.get_accel(want_pm=True)
        if truth is None:
            truth = eng.direct_sum(idx)
        eng.close()
        e = rel_err((acc + pm)[idx], truth)
        rms[N] = float(np.sqrt(np.mean(e ** 2)))
    print("TreePM total vs direct sum, rms over 600 targets: N=32 %.3e, N=48 %.3e, N=64 %.3e" % (rms[32], rms[48], rms[64]))
    assert rms[48] <= 1.5 * max(rms[32], rms[64])
    assert rms[48] < 1e-2
