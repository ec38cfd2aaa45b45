"""The group walk's traversal reads a 16-byte node head (flags, first, count, a lower bound of the node's mass) and opens a node
from the head and the geometry alone when the opening criterion holds for an upper bound of every species' distance: the
multipole moments of such a node are never fetched.  The shortcut may change no decision and no append order, so a walk with the
head (tuning walk_head 1, the default) and one without (walk_head 0: the separate arrays, moments always fetched) must give the
same GravAccel and GravCost bit for bit, and the same list and traversal statistics -- on every kind of set the decision depends
on: species count, mass spread, massless particles, a species missing from half the box, a clump in which monopoles are accepted,
a tree-only non-periodic walk (which is handed the head but, by design, does not read it), a sparse active set.  A refit tree
has no valid head: its walk must not use one.

Each set is walked twice per engine: the Barnes-Hut pass (theta 0.5) that gives OldAcc, then the relative criterion with it."""
import functools

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

L, PMGRID = 1.0, 32
ERRTOL = 0.005
T2G = {1: [0] * 6, 2: [0, 1, 1, 0, 1, 0], 3: [0, 1, 2, 2, 1, 0]}
CASES = {
    # name: (particles, N_GRAVS, TreePM?)
    "uniform_ng2": (1 << 15, 2, True),
    "uniform_ng1": (1 << 14, 1, True),
    "uniform_ng3": (1 << 14, 3, True),
    "mass_spread": (1 << 14, 2, True),
    "clump": (1 << 16, 2, True),
    "plummer": (1 << 14, 2, False),
    "sparse_active": (1 << 15, 2, True),
}


@functools.lru_cache(maxsize=None)
def _particles(case):
    n, ng, _ = CASES[case]
    rng = np.random.default_rng(606 + n + ng)
    pos = rng.uniform(0.0, L, (n, 3))
    mass = np.full(n, 1.0 / n)
    typ = rng.integers(0, 6, n).astype(np.int32)
    active = None
    if case == "mass_spread":
        mass = 10.0 ** rng.uniform(-6.0, 0.0, n) / n          # spread over 10^6
        mass[rng.choice(n, n // 100, replace=False)] = 0.0      # 1 % massless
        left = pos[:, 0] < 0.5 * L                              # species 1 absent from half the box
        typ[left] = np.where(np.asarray(T2G[ng])[typ[left]] == 1, 0, typ[left])
        assert not np.any(np.asarray(T2G[ng])[typ[left]] == 1) and np.any(np.asarray(T2G[ng])[typ[~left]] == 1)
    elif case == "clump":
        k = (6 * n) // 10                                       # 60 % of the particles in one clump
        pos[:k] = np.mod(0.37 * L + 0.004 * L * rng.standard_normal((k, 3)), L)
    elif case == "plummer":
        a = 0.05
        r = a / np.sqrt(rng.uniform(1e-6, 0.999, n) ** (-2.0 / 3.0) - 1.0)
        mu, ph = rng.uniform(-1.0, 1.0, n), rng.uniform(0.0, 2.0 * np.pi, n)
        s = np.sqrt(1.0 - mu * mu)
        pos = 3.0 + r[:, None] * np.stack([s * np.cos(ph), s * np.sin(ph), mu], axis=1)   # (away from the origin)
    elif case == "sparse_active":
        active = (rng.uniform(size=n) < 0.02).astype(np.uint8)
    for a_ in (pos, mass, typ) + ((active,) if active is not None else ()):
        a_.setflags(write=False)
    return pos, mass, typ, active


def _config(pkg, case):
    n, ng, pm = CASES[case]
    eps = L / (40 * n ** (1 / 3))
    if pm:
        return pkg.make_config(n_gravs=ng, periodic=1, pmgrid=PMGRID, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                               type_to_grav=T2G[ng], wiring="c4", walk_mode=pkg.WALK_GROUP)
    return pkg.make_config(n_gravs=ng, periodic=0, pmgrid=0, G=1.0, theta=0.5, softening=[0.05 * eps] * 6, type_to_grav=T2G[ng],
                           wiring="newton", walk_mode=pkg.WALK_GROUP)


def _record(eng):
    acc, old, cost = eng.get_accel()
    st = eng.stats()
    skips, within = eng.walk_moment_skips()
    return {"acc": acc, "old": old, "cost": cost, "entries": st.reserved[0], "nodes": st.reserved[1], "skips": skips, "within": within}


@functools.lru_cache(maxsize=None)
def _walks(pkg, case, head):
    """(theta pass, relative pass) of one engine"""
    pos, mass, typ, active = _particles(case)
    pm = CASES[case][2]
    eng = pkg.Engine(_config(pkg, case))
    eng.set_tuning(walk_head=head)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=pm)
    first = _record(eng)
    eng.set_particles(pos, mass, typ, old_acc=first["old"], active=active)
    eng.set_opening(0.0, ERRTOL)
    eng.compute_accelerations(pm_step=pm)
    second = _record(eng)
    eng.close()
    return first, second


def _same(a, b, what):
    print("%s: list entries per group %.2f / %.2f, nodes tested per group %.2f / %.2f, skips %d of %d within reach" %
          (what, a["entries"], b["entries"], a["nodes"], b["nodes"], a["skips"], a["within"]))
    assert np.array_equal(a["acc"], b["acc"]) and np.array_equal(a["cost"], b["cost"])
    assert a["entries"] == b["entries"] and a["nodes"] == b["nodes"]
    assert a["entries"] > 0 and a["nodes"] > 0 and np.any(a["acc"] != 0.0)
    assert b["skips"] == 0 and b["within"] == 0           # walk_head 0 hands the kernel no head
    assert 0 <= a["skips"] <= a["within"]


@pytest.mark.parametrize("case", list(CASES))
def test_walk_with_head_equals_walk_without(pkg, case):
    on, off = _walks(pkg, case, 1), _walks(pkg, case, 0)
    _same(on[0], off[0], case + ", theta pass")
    _same(on[1], off[1], case + ", relative criterion")
    if CASES[case][2]:
        assert on[0]["within"] > 0 and on[1]["within"] > 0    # the head was read
    else:
        # tree-only walks take no head: most of what they test is accepted (9 % of this sphere's nodes would take the shortcut)
        assert on[0]["within"] == 0 and on[1]["within"] == 0


def test_shortcut_fires_in_a_uniform_box(pkg):
    on = _walks(pkg, "uniform_ng2", 1)
    assert on[0]["skips"] > 0 and on[1]["skips"] > 0


def test_both_branches_run_in_a_clump(pkg):
    """monopoles are accepted around the clump: some nodes within reach are opened from the head, others need their moments"""
    on = _walks(pkg, "clump", 1)[1]
    assert on["cost"].max() > 0
    assert 0 < on["skips"] < on["within"]


def test_refit_tree_walks_without_the_head(pkg):
    """ngravs_force_update_tree() grows cells and recomputes moments: the head of the build is stale, and the walk must not read it"""
    case = "uniform_ng2"
    pos, mass, typ, _ = _particles(case)
    old = _walks(pkg, case, 1)[0]["old"]
    rng = np.random.default_rng(77)
    pos2 = np.mod(pos + 2e-3 * L * rng.standard_normal(pos.shape), L)

    def run(head):
        eng = pkg.Engine(_config(pkg, case))
        eng.set_tuning(walk_head=head)
        eng.set_particles(pos, mass, typ, old_acc=old)
        eng.set_opening(0.0, ERRTOL)
        eng.compute_accelerations(pm_step=False)
        built = eng.walk_moment_skips()
        eng.update_particles(pos2, mass, typ, old_acc=old)
        eng.force_update_tree()
        eng.gravity_tree()
        r = _record(eng)
        eng.close()
        return built, r

    (built_on, on), (built_off, off) = run(1), run(0)
    assert built_on[0] > 0 and built_off == (0, 0)
    assert on["skips"] == 0 and on["within"] == 0
    assert np.array_equal(on["acc"], off["acc"]) and np.array_equal(on["cost"], off["cost"])
    assert on["entries"] == off["entries"] and on["nodes"] == off["nodes"]
