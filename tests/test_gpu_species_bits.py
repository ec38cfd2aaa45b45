"""The group walk sorts the particles it hands over into per-species lists.  These tests pin what the lists must hold when the
species is NOT a function of the particle index: six particle types drawn at random, two of them mapped onto one species, on the
production path (TreePM, wiring c4, N_GRAVS 2 and 3) -- against the oracle's cut direct sum (O.direct_shortrange) with the
thresholds of test_gpu_parity.test_production_walk_is_the_cut_direct_sum, and bit for bit between paths that must agree
(refit against fresh build, fused against split kernels).

2^15 particles in a PMGRID 40 box: two mesh cells per particle, the density of the C4 benchmark, so that every source inside the
cut sphere reaches the force loop as a particle (see the production test's docstring)."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N, L, PMGRID = 1 << 15, 1.0, 40
REACH = 4.5 * 1.25 * L / PMGRID
ERRTOL = 0.005        # ErrTolForceAcc of the benchmark's steady-state step
# The cut direct sum is the truth while every source inside the cut sphere reaches the force loop as a particle.  The benchmark's
# criterion does that for the 256 targets of a unit of four groups (some target is always close enough to open a cell); a unit of
# one group, or one target per wave, accepts cells inside the sphere.  Tests of those paths therefore open by a criterion under
# which no cell inside the sphere is accepted: a cell of two particles (mass 2/N) and side len at distance r is opened if
# 2/N len^2 > r^4 |OldAcc| ErrTolForceAcc; with r <= REACH = 0.14 and |OldAcc| = O(1) this holds down to len = L / 1024, a
# thirtieth of the mean particle spacing, for ErrTolForceAcc = 1e-7.
ERRTOL_OPEN_ALL = 1e-7
T2G = {2: [0, 1, 1, 0, 1, 0], 3: [0, 1, 2, 2, 1, 0]}   # two types on one species
NCLUMP = 20


@functools.lru_cache(maxsize=None)
def _particles(clump):
    rng = np.random.default_rng(2024)
    pos = rng.uniform(0.0, L, (N, 3)).astype(np.float32).astype(np.float64)
    pos[pos >= L] = float(np.nextafter(np.float32(L), np.float32(0)))
    mass = np.full(N, 1.0 / N)
    typ = rng.integers(0, 6, N).astype(np.int32)
    members = None
    if clump:
        # 20 coincident particles of mixed species: one key, one bucket beyond the 8 particles a lane hands over at once
        members = np.sort(rng.choice(N, NCLUMP, replace=False))
        pos[members] = pos[members[0]]
        typ[members] = np.arange(NCLUMP) % 6
    for a in (pos, mass, typ):
        a.setflags(write=False)
    return pos, mass, typ, members


def _config(pkg, ng):
    eps = L / (40 * N ** (1 / 3))
    return pkg.make_config(n_gravs=ng, periodic=1, pmgrid=PMGRID, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                           type_to_grav=T2G[ng], wiring="c4", walk_mode=pkg.WALK_GROUP)


_old_cache = {}


def _old_acc(pkg, ng, clump):
    """OldAcc of the set from one Barnes-Hut pass, computed once: every walk compared below opens by the same numbers"""
    if (ng, clump) not in _old_cache:
        pos, mass, typ, _ = _particles(clump)
        eng = pkg.Engine(_config(pkg, ng))
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=True)
        _, old, _ = eng.get_accel()
        eng.close()
        old.setflags(write=False)
        _old_cache[(ng, clump)] = old
    return _old_cache[(ng, clump)]


def _production_walk(pkg, ng, clump, tuning=None, errtol=ERRTOL, want_order=False):
    """the steady-state step of the benchmark (relative criterion, PM step) on a fresh engine"""
    pos, mass, typ, _ = _particles(clump)
    eng = pkg.Engine(_config(pkg, ng))
    if tuning:
        eng.set_tuning(**tuning)
    eng.set_particles(pos, mass, typ, old_acc=_old_acc(pkg, ng, clump))
    eng.set_opening(0.0, errtol)
    eng.compute_accelerations(pm_step=True)
    acc, _, cost = eng.get_accel()
    st = eng.stats()
    order = eng.order() if want_order else None
    eng.close()
    return (acc, cost, st, order) if want_order else (acc, cost, st)


_truth_cache = {}


def _truth(pkg, O, ng, clump, idx):
    key = (ng, clump, idx.tobytes())
    if key not in _truth_cache:
        pos, mass, typ, _ = _particles(clump)
        cfg = _config(pkg, ng)
        tab, _ = O.shortrange_table(cfg)
        _truth_cache[key] = O.direct_shortrange(cfg, pos, mass, typ, idx, tab, REACH)
    return _truth_cache[key]


def _targets():
    return np.sort(np.random.default_rng(11).choice(N, 512, replace=False)).astype(np.int32)


def _targets_around_clump(order):
    """The clump is a cell of the deepest level: far too small for the relative criterion to open it from outside, so a target
    gets its 20 members one by one only if the cell lies inside the box of the target's traversal unit (the walk's inside-cell
    test), and otherwise as one exact monopole per species -- the same force, but not the same count.  Targets in and around the
    clump are therefore the members of every unit (256 consecutive particles of the Peano order) whose box holds the clump."""
    pos, _, _, members = _particles(True)
    centre = pos[members[0]]
    idx = []
    for u0 in range(0, N, 256):
        unit = order[u0:u0 + 256]
        lo, hi = pos[unit].min(axis=0), pos[unit].max(axis=0)
        if np.all(lo <= centre) and np.all(centre <= hi):
            idx.append(unit)
    idx = np.sort(np.concatenate(idx)).astype(np.int32)
    assert np.all(np.isin(members, idx)) and len(idx) >= 256
    return idx


def _check_against_cut_direct_sum(pkg, O, ng, clump, acc, cost, what, idx=None):
    idx = _targets() if idx is None else idx
    a_o, n_o = _truth(pkg, O, ng, clump, idx)
    err = np.linalg.norm(acc[idx] - a_o, axis=1) / np.linalg.norm(a_o, axis=1)
    same = cost[idx].astype(np.int64) == n_o.astype(np.int64)
    exact = err < 1e-10
    print("%s [N_GRAVS=%d]: %.1f (oracle %.1f) pairs/target; counts equal for %d, force equal to rounding for %d of %d targets "
          "(median %.1e); worst %.1e" % (what, ng, cost[idx].mean(), n_o.mean(), same.sum(), exact.sum(), len(idx), np.median(err),
                                         err.max()))
    assert same.mean() > 0.97 and exact.mean() > 0.97
    assert err.max() < 2e-3


@pytest.mark.parametrize("ng", [2, 3])
def test_production_walk_with_random_types(pkg, O, ng):
    """default tuning: units of four groups, leaf hand-over at 8, start table, split kernels"""
    acc, cost, st = _production_walk(pkg, ng, False)
    assert st.reserved[5] >= 1   # the traversal + evaluation kernels ran
    _check_against_cut_direct_sum(pkg, O, ng, False, acc, cost, "random types, production walk")


@pytest.mark.parametrize("ng", [2, 3])
def test_coincident_bucket_of_mixed_species(pkg, O, ng):
    """a bucket of 20: its first 8 particles are handed over with the node, the other 12 one by one"""
    acc, cost, _, order = _production_walk(pkg, ng, True, want_order=True)
    idx = _targets_around_clump(order)
    _check_against_cut_direct_sum(pkg, O, ng, True, acc, cost, "coincident bucket, %d targets" % len(idx), idx)


@pytest.mark.parametrize("ng", [2, 3])
def test_no_leaf_handover_units_of_one_group(pkg, O, ng):
    """walk_nleaf 0, walk_sg 1: every node but a bucket is opened child by child, down to its last two particles (ERRTOL_OPEN_ALL)"""
    acc, cost, _ = _production_walk(pkg, ng, False, tuning={"walk_nleaf": 0, "walk_sg": 1}, errtol=ERRTOL_OPEN_ALL)
    _check_against_cut_direct_sum(pkg, O, ng, False, acc, cost, "walk_nleaf 0, walk_sg 1")


@pytest.mark.parametrize("ng", [2, 3])
def test_refit_after_type_change_equals_fresh_build(pkg, ng):
    """a tenth of the particles change type while the tree is kept (ngravs_update_particles + ngravs_force_update_tree): the walk of
    the refit tree must give what the walk of a tree built from the new types gives, bit for bit"""
    pos, mass, typ, _ = _particles(True)
    old = _old_acc(pkg, ng, True)
    rng = np.random.default_rng(5)
    typ2 = typ.copy()
    ch = rng.choice(N, N // 10, replace=False)
    typ2[ch] = (typ[ch] + rng.integers(1, 6, len(ch))) % 6   # every one of them to another type
    cfg = _config(pkg, ng)
    assert np.any(np.asarray(T2G[ng])[typ2[ch]] != np.asarray(T2G[ng])[typ[ch]])

    def run(first_types, refit):
        eng = pkg.Engine(cfg)
        eng.set_particles(pos, mass, first_types, old_acc=old)
        eng.set_opening(0.0, ERRTOL)
        eng.compute_accelerations(pm_step=False)   # decomposition, build, walk
        if refit:
            eng.update_particles(pos, mass, typ2, old_acc=old)
            eng.force_update_tree()
            eng.gravity_tree()
        acc, _, cost = eng.get_accel()
        eng.close()
        return acc, cost

    acc_r, cost_r = run(typ, True)
    acc_f, cost_f = run(typ2, False)
    acc_0, _ = run(typ, False)
    assert not np.array_equal(acc_0, acc_f)        # (the type change matters to the forces)
    assert np.array_equal(acc_r, acc_f) and np.array_equal(cost_r, cost_f)


@pytest.mark.parametrize("ng", [2, 3])
def test_fused_kernel_equals_split_kernels(pkg, O, ng):
    """The fused kernel walks units of one group; with the split pair on the same units (walk_sg 1) both record the same lists in
    the same order: the same accelerations bit for bit.  With lists far too short (walk_lcap 1024, as
    test_group_walk_leftover_groups) the fused kernel redoes every overflowed unit of the split walk in sub-groups: other
    boxes, so not the same bits, but still the cut direct sum once no cell inside the sphere is accepted (ERRTOL_OPEN_ALL)."""
    acc_s, cost_s, st = _production_walk(pkg, ng, False, tuning={"walk_sg": 1})
    assert st.reserved[5] >= 1
    acc_f, cost_f, _ = _production_walk(pkg, ng, False, tuning={"walk_sg": 1, "walk_fused": 1})
    assert np.array_equal(acc_f, acc_s) and np.array_equal(cost_f, cost_s)
    acc_l, cost_l, _ = _production_walk(pkg, ng, False, tuning={"walk_lcap": 1024}, errtol=ERRTOL_OPEN_ALL)
    _check_against_cut_direct_sum(pkg, O, ng, False, acc_l, cost_l, "split walk with short lists, redone by the fused kernel")
