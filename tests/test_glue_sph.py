"""The first guess of the smoothing lengths (ngravs_sph_hsml_guess, csrc/kernels_sph.hip) against a numpy restatement of the
reference's setup_smoothinglengths() (init.c:229-247, 3-D branch).

The reference's rule, on its gas-only tree (ngb_treebuild -> force_treebuild(N_gas), ngb.c:408) in the domain cube of ALL
particles: an internal node exists for exactly the octree cells that hold two or more gas particles, plus the root; Father[i]
is the deepest such cell containing i; the loop climbs from there while 10 DesNumNgb m_i > mass(no) and stops at the root; then
Hsml = (3 / (4 pi) DesNumNgb m_i / mass(no))^(1/3) len(no).

guess_restated() says that by integer cell coordinates: a particle's coordinates at 21 + 30 bits are floor((x - corner) fac21
2^30) (the tree build's own cell arithmetic, k_keys, continued by exact powers of two below its deepest level), the cell of level
L is those coordinates >> (51 - L), and np.unique counts the gas rows and sums the gas mass of every cell of every level.  It
climbs, as the reference does; the device descends from the root.  tree_by_insertion() builds the gas-only octree the way
force_treebuild does, particle by particle, and runs the loop of init.c on it word for word.

Tolerance: TOL of tests/test_sph_reference.py (1e-11 relative).  The choice of the cell is discrete: a row whose cell mass lies
within 1e-9 relative of its threshold, at the chosen cell or the next one down, may be left out -- with the seeds below no row is
(checked on the CPU when the seeds were picked, asserted in the tests).

The second half of the module holds host/gadget_glue.c under -DNGRAVS_GLUE_SPH (density(), hydro_force(), ngb_tree*() of a gas run on
one task): the link closure of the extended recipe and the refused switches (CPU), the stubs of tests/glue_stub_sph against the
reference's headers (CPU), and the glue EXECUTED on the GPU with tests/glue_stub_sph/glue_sph_driver.c -- SphP[] bit for bit what
the Python host gives for the same library calls, and within TOL of the reference's own density() / hydro_force() (oracle/_ref/).
"""
import ctypes as C
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


SR = _load("test_sph_reference", os.path.join(HERE, "test_sph_reference.py"))
TOL, D = SR.TOL, SR.D
TREE_BITS, SUB = 21, 30           # levels of the device tree; halvings below its deepest level (SPH_GUESS_SUB)
NL = TREE_BITS + SUB
MARGIN = 1e-9


# ---- the restatement ------------------------------------------------------------------------------------------------------
def domain_of(pos):
    """DomainCorner, DomainCenter, DomainLen, DomainFac of all particles (domain.c:909-923): what Engine.domain() returns"""
    lo, hi = pos.min(axis=0), pos.max(axis=0)
    length = float(np.max(hi - lo)) * 1.001
    centre = 0.5 * (lo + hi)
    return np.concatenate([centre - 0.5 * length, centre, [length, 1.0 / length * float(1 << 18)]])


def cell_coords(pos, dom):
    """integer coordinates at NL bits per dimension"""
    fac21 = dom[7] * float(1 << (TREE_BITS - 18))
    u = (pos - dom[:3]) * fac21
    return np.floor(u * float(1 << SUB)).astype(np.int64)


def guess_restated(pos, mass, ptype, des, dom):
    """(gas rows, hsml, level of the chosen cell, margin) over the gas rows"""
    gas = np.nonzero(ptype == 0)[0]
    ng = len(gas)
    coords, m = cell_coords(pos[gas], dom), mass[gas]
    thr = 10 * des * m
    cnt = np.empty((NL + 1, ng), dtype=np.int64)
    ms = np.empty((NL + 1, ng))
    for lv in range(NL + 1):
        _, inv, counts = np.unique(coords >> (NL - lv), axis=0, return_inverse=True, return_counts=True)
        inv = inv.ravel()
        cnt[lv] = counts[inv]
        ms[lv] = np.bincount(inv, weights=m)[inv]
    ar = np.arange(ng)
    is_node = cnt >= 2
    is_node[0] = True
    father = is_node.sum(axis=0) - 1           # counts never grow going down: the nodes containing i are levels 0..father
    assert np.all(is_node[father, ar]) and np.all(father < NL), "two gas rows share all %d bits" % NL
    lv = father.copy()
    while True:
        up = (lv > 0) & (thr > ms[lv, ar])      # init.c:235-243
        if not up.any():
            break
        lv[up] -= 1
    chosen = ms[lv, ar]
    hsml = np.cbrt(3.0 / (4 * np.pi) * des * m / chosen) * (dom[6] * 0.5 ** lv)   # init.c:246-247
    margin = np.abs(chosen - thr) / thr
    below = lv < father
    margin[below] = np.minimum(margin[below], (np.abs(ms[lv + 1, ar] - thr) / thr)[below])
    return gas, hsml, lv, margin


def tree_by_insertion(pos, mass, ptype, des, dom):
    """force_treebuild(N_gas) by insertion (forcetree.c:138-300: a cell is split when a second particle arrives), the node masses,
    Father[], and the loop of init.c:229-247 on that tree.  Returns hsml over the gas rows."""
    gas = np.nonzero(ptype == 0)[0]
    coords, m = cell_coords(pos[gas], dom), mass[gas]

    def octant(i, level):                       # which child of a node of `level` holds particle i
        c = (coords[i] >> (NL - level - 1)) & 1
        return int(c[0]) * 4 + int(c[1]) * 2 + int(c[2])

    nodes = [dict(level=0, father=-1, child=[None] * 8, mass=0.0)]
    for i in range(len(gas)):
        no = 0
        while True:
            k = octant(i, nodes[no]["level"])
            slot = nodes[no]["child"][k]
            if slot is None:
                nodes[no]["child"][k] = ("p", i)
                break
            if slot[0] == "n":
                no = slot[1]
                continue
            j = slot[1]                          # occupied by a particle: a new internal node takes both
            assert nodes[no]["level"] + 1 < NL
            nodes.append(dict(level=nodes[no]["level"] + 1, father=no, child=[None] * 8, mass=0.0))
            new = len(nodes) - 1
            nodes[no]["child"][k] = ("n", new)
            nodes[new]["child"][octant(j, nodes[new]["level"])] = ("p", j)
            no = new
    father = np.zeros(len(gas), dtype=np.int64)
    for i in range(len(gas)):
        no = 0
        while True:
            nodes[no]["mass"] += m[i]
            slot = nodes[no]["child"][octant(i, nodes[no]["level"])]
            if slot[0] == "p":
                assert slot[1] == i
                father[i] = no
                break
            no = slot[1]
    hsml = np.zeros(len(gas))
    for i in range(len(gas)):
        no = father[i]
        while 10 * des * m[i] > nodes[no]["mass"]:
            p = nodes[no]["father"]
            if p < 0:
                break
            no = p
        hsml[i] = (3.0 / (4 * np.pi) * des * m[i] / nodes[no]["mass"]) ** (1.0 / 3) * (dom[6] * 0.5 ** nodes[no]["level"])
    return hsml


# ---- inputs -------------------------------------------------------------------------------------------------------------
def gas_set(pkg, kind, ngas, nother, seed, box=1000.0):
    """ngas type-0 rows mixed with nother type-1 rows; gas masses with a seeded +-10 % jitter (no cell mass ties with a threshold)"""
    n = ngas + nother
    rng = np.random.default_rng(seed)
    if kind == "uniform":
        pos, mass, _ = pkg.ic.uniform_box(n, box=box, n_gravs=1, seed=seed)
    else:
        pos, mass, _ = pkg.ic.plummer_sphere(n, seed=seed)
    ptype = np.where(rng.permutation(n) < ngas, 0, 1).astype(np.int32)
    mass = np.where(ptype == 0, mass * rng.uniform(0.9, 1.1, n), mass)
    return pos, mass, ptype


def heavy_neighbours(pos, mass, ptype, seed):
    """test B: 8 gas rows of 2000 x the mean gas mass, each within 1e-4 of a light gas row (1e-4 / 8^k, k = 0..7: some pairs share
    cells above the device tree's deepest level, some only below it).  Returns the set and the rows of the 8 light partners."""
    rng = np.random.default_rng(seed)
    gas = np.nonzero(ptype == 0)[0]
    partner = np.sort(rng.choice(gas, 8, replace=False))
    direction = rng.normal(size=(8, 3))
    direction /= np.linalg.norm(direction, axis=1)[:, None]
    extra = pos[partner] + direction * (1e-4 * 0.125 ** np.arange(8))[:, None]
    heavy_mass = np.full(8, 2000 * mass[gas].mean()) * rng.uniform(0.9, 1.1, 8)
    return (np.concatenate([pos, extra]), np.concatenate([mass, heavy_mass]), np.concatenate([ptype, np.zeros(8, dtype=np.int32)]),
            partner)


def make_engine(pkg, periodic, pos, mass, ptype, box=1000.0, **kw):
    cfg = pkg.make_config(n_gravs=1, periodic=int(periodic), box_size=box if periodic else 0.0, softening=[0.01] * 6,
                          walk_mode=pkg.WALK_GROUP, **kw)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.domain_Decomposition()
    eng.force_treebuild()
    return eng


def against_restatement(eng, pos, mass, ptype, des, what, res=None):
    ref_gas, ref, lv, margin = guess_restated(pos, mass, ptype, des, eng.domain())
    sentinel = np.full(len(pos), -3.25)
    res = eng.sph_hsml_guess(des, sentinel) if res is None else res
    err = np.abs(res[ref_gas] - ref) / ref
    print("hsml guess %s, DesNumNgb %g: worst %.2e over %d gas rows, levels %d..%d, smallest margin %.2e, %.3f ms"
          % (what, des, err.max(), len(ref_gas), lv.min(), lv.max(), margin.min(), eng.last_hsml_guess_ms))
    assert margin.min() >= MARGIN, "a row lies within %g of a threshold: pick another seed" % MARGIN
    assert err.max() <= TOL, (what, des, err.max(), int(np.argmax(err)))
    other = np.ones(len(pos), dtype=bool)
    other[ref_gas] = False
    assert np.all(res[other] == -3.25)
    return ref_gas, ref, lv


SETS = [("plummer", False, 4000, 2000, 31), ("uniform", True, 3000, 3000, 32)]


# ---- CPU ----------------------------------------------------------------------------------------------------------------
def test_restatement_is_the_loop_of_init_c_on_an_insertion_built_gas_tree(pkg):
    for kind, seed in (("plummer", 41), ("uniform", 42)):
        pos, mass, ptype = gas_set(pkg, kind, 600, 300, seed)
        dom = domain_of(pos)
        for des in (32.0, 5.0, 0.5):
            _, hsml, lv, _ = guess_restated(pos, mass, ptype, des, dom)
            plain = tree_by_insertion(pos, mass, ptype, des, dom)
            assert np.max(np.abs(hsml - plain) / plain) <= 1e-14
            assert des > 1 or lv.max() > lv.min() + 1
    # a heavy particle beside light ones: the light one's cell lies far below the rest
    pos, mass, ptype = gas_set(pkg, "plummer", 600, 300, 41)
    pos, mass, ptype, partner = heavy_neighbours(pos, mass, ptype, 43)
    dom = domain_of(pos)
    gas, hsml, lv, _ = guess_restated(pos, mass, ptype, 32.0, dom)
    plain = tree_by_insertion(pos, mass, ptype, 32.0, dom)
    assert np.max(np.abs(hsml - plain) / plain) <= 1e-14
    assert lv[np.isin(gas, partner)].max() > TREE_BITS


@pytest.mark.parametrize("kind,periodic,ngas,nother,seed", SETS)
def test_seeds_leave_no_row_near_a_threshold(pkg, kind, periodic, ngas, nother, seed):
    """the condition of the GPU tests A and B, on the host's own domain cube"""
    pos, mass, ptype = gas_set(pkg, kind, ngas, nother, seed)
    for des in (32.0, 50.0):
        assert guess_restated(pos, mass, ptype, des, domain_of(pos))[3].min() >= MARGIN
    if not periodic:
        pos, mass, ptype, _ = heavy_neighbours(pos, mass, ptype, seed + 100)
        for des in (32.0, 50.0):
            assert guess_restated(pos, mass, ptype, des, domain_of(pos))[3].min() >= MARGIN


def test_library_exports_the_guess(pkg, have_lib):
    assert "ngravs_sph_hsml_guess" in pkg.EXPORTS and hasattr(have_lib, "ngravs_sph_hsml_guess")
    hdr = open(os.path.join(os.path.dirname(pkg.__file__), "..", "include", "ngravs_hip.h")).read()
    assert "int ngravs_sph_hsml_guess(ngravs_ctx *ctx, double des_num_ngb, double *hsml, int64_t hsml_stride," in hdr
    assert pkg.abi.SPH_HSML_GUESS_ARGTYPES == [C.c_void_p, C.c_double, C.c_void_p, C.c_int64, C.c_int32, C.c_int32, C.c_void_p]
    assert have_lib.ngravs_abi_version() == 3
    assert pkg.lib().ngravs_sph_hsml_guess(None, 32.0, None, 8, 0, 0, None) == -1      # no context: NGRAVS_ERR_ARG, no GPU touched


# ---- GPU ----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic,ngas,nother,seed", SETS)
def test_guess_against_the_restatement(pkg, kind, periodic, ngas, nother, seed):
    pos, mass, ptype = gas_set(pkg, kind, ngas, nother, seed)
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    assert np.allclose(eng.domain(), domain_of(pos), rtol=1e-12, atol=0)
    for des in (32.0, 50.0):
        against_restatement(eng, pos, mass, ptype, des, kind)
    # nothing passed: NaN in the rows that are no gas
    res = eng.sph_hsml_guess(32.0)
    assert np.all(np.isnan(res[ptype != 0])) and np.all(res[ptype == 0] > 0)
    eng.close()


@pytest.mark.gpu
def test_guess_below_the_deepest_device_level(pkg):
    kind, periodic, ngas, nother, seed = SETS[0]
    pos, mass, ptype = gas_set(pkg, kind, ngas, nother, seed)
    pos, mass, ptype, partner = heavy_neighbours(pos, mass, ptype, seed + 100)
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    for des in (32.0, 50.0):
        gas, ref, lv = against_restatement(eng, pos, mass, ptype, des, "heavy neighbours")
        near = np.isin(gas, partner)
        assert lv[near].max() > TREE_BITS and lv[near].min() <= TREE_BITS, lv[near]
    eng.close()


@pytest.mark.gpu
def test_guess_on_a_device_tensor_is_the_host_result(pkg):
    import torch
    kind, periodic, ngas, nother, seed = SETS[1]
    pos, mass, ptype = gas_set(pkg, kind, ngas, nother, seed)
    eng = make_engine(pkg, periodic, pos, mass, ptype)
    start = np.where(np.arange(len(pos)) % 4 == 0, 0.37, -3.25)
    for only_unset in (False, True):
        host = eng.sph_hsml_guess(32.0, start, only_unset=only_unset)
        dev = eng.sph_hsml_guess(32.0, torch.from_numpy(start).cuda(), only_unset=only_unset)
        assert dev.is_cuda and np.array_equal(dev.cpu().numpy(), host)
    assert np.all(host[(ptype == 0) & (np.arange(len(pos)) % 4 == 0)] == 0.37)
    eng.close()


def _raw(pkg, eng, des, arr, only_unset=0):
    rc = pkg.lib().ngravs_sph_hsml_guess(eng._h, des, None if arr is None else arr.ctypes.data, 8, only_unset, 0, None)
    msg = pkg.lib().ngravs_last_error(eng._h)
    return rc, (msg.decode() if msg else "")


@pytest.mark.gpu
def test_only_unset_refusals_and_density_from_the_guess(pkg):
    kind, periodic, ngas, nother, seed = SETS[0]
    pos, mass, ptype = gas_set(pkg, kind, ngas, nother, seed)
    des = 50.0
    gas, ref, _, _ = guess_restated(pos, mass, ptype, des, domain_of(pos))
    n = len(pos)
    cfg_kw = dict(n_gravs=1, periodic=0, softening=[0.01] * 6, walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(pkg.make_config(**cfg_kw))
    eng.set_particles(pos, mass, ptype)
    keep = np.full(n, -3.25)
    rc, msg = _raw(pkg, eng, des, keep)
    assert rc == -4 and "ngravs_sph_hsml_guess" in msg and "built tree" in msg and np.all(keep == -3.25), (rc, msg)
    eng.domain_Decomposition()
    eng.force_treebuild()
    # only_unset: the preset half keeps its value bit for bit, the other half (0, negative, NaN) gets the guess
    preset = np.full(n, -3.25)
    preset[gas[0::2]] = 0.37
    preset[gas[1::6]] = 0.0
    preset[gas[3::6]] = -1.0
    preset[gas[5::6]] = np.nan
    res = eng.sph_hsml_guess(des, preset, only_unset=True)
    assert np.all(res[gas[0::2]] == 0.37) and np.all(res[ptype != 0] == -3.25)
    assert np.max(np.abs(res[gas[1::2]] - ref[1::2]) / ref[1::2]) <= TOL
    full = eng.sph_hsml_guess(des, np.full(n, -3.25))
    assert np.array_equal(full[gas[1::2]], res[gas[1::2]])
    # refusals: code, message, nothing written
    rc, msg = _raw(pkg, eng, des, None)
    assert rc == -1 and "hsml must not be NULL" in msg, (rc, msg)
    for bad_des in (0.0, -2.0, float("nan")):
        rc, msg = _raw(pkg, eng, bad_des, keep)
        assert rc == -1 and "des_num_ngb must be > 0" in msg and np.all(keep == -3.25), (rc, msg)
    two = pkg.Engine(pkg.make_config(world_size=2, rank=0, **cfg_kw))
    two.set_particles(pos, mass, ptype)
    rc, msg = _raw(pkg, two, des, keep)
    assert rc == -4 and "single task only" in msg and np.all(keep == -3.25), (rc, msg)
    two.close()
    for bad_mass in (0.0, -1.0):
        m2 = mass.copy()
        m2[gas[11]] = bad_mass
        bad = pkg.Engine(pkg.make_config(**cfg_kw))
        bad.set_particles(pos, m2, ptype)
        bad.domain_Decomposition()
        bad.force_treebuild()
        rc, msg = _raw(pkg, bad, des, keep)
        assert rc == -1 and "mass is <= 0 or not finite" in msg and np.all(keep == -3.25), (bad_mass, rc, msg)
        bad.close()
    none = make_engine(pkg, False, pos, mass, np.ones(n, dtype=np.int32))
    rc, msg = _raw(pkg, none, des, keep)
    assert rc == 0 and np.all(keep == -3.25)
    none.close()
    # after update_particles the tree is refit first, and the walk's state is not disturbed
    eng.update_particles(pos, mass, ptype)
    again = eng.sph_hsml_guess(des, np.full(n, -3.25))
    assert np.array_equal(again, full)
    eng.gravity_tree()
    acc1, _, cost1 = eng.get_accel()
    plain = make_engine(pkg, False, pos, mass, ptype)
    plain.gravity_tree()
    acc0, _, cost0 = plain.get_accel()
    assert np.array_equal(acc0, acc1) and np.array_equal(cost0, cost1)
    plain.close()
    # density() started from the device's guess converges, and equals density() started from the restatement's guess
    vel = np.random.default_rng(7).normal(0.0, 1.0, (n, 3))
    start = np.zeros(n)
    start[gas] = ref
    a = eng.sph_density(vel, full, des, D.DEV)
    b = eng.sph_density(vel, start, des, D.DEV)
    assert 0 < a["max_rounds"] < D.MAXITER
    for k in ("hsml", "density", "num_ngb", "dhsml_factor"):
        assert np.max(np.abs(a[k][gas] - b[k][gas]) / np.abs(b[k][gas])) <= TOL, k
    eng.close()


# ==== the glue of a gas run: gadget_glue.c under -DNGRAVS_GLUE_SPH ===============================================================
H, R = SR.H, SR.R
ROOT = os.path.join(HERE, "..")
GLUE_DEFS = ["-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION", "-DUNEQUALSOFTENINGS"]
SPH_OPTION_SETS = [[], ["-DPERIODIC"], ["-DPERIODIC", "-DPMGRID=64"], ["-DPERIODIC", "-DISOTHERM_EQS"], ["-DPERIODIC", "-DNOVISCOSITYLIMITER"]]
SPH_SYMBOLS = ("density", "hydro_force", "ngb_treeallocate", "ngb_treefree", "ngb_treebuild")


def _glue(pkg):
    return os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")


def _includes():
    return ["-I" + os.path.join(ROOT, "tests", "glue_stub_sph"), "-I" + os.path.join(ROOT, "tests", "glue_stub"), "-I" + os.path.join(ROOT, "include")]


def _defined(obj):
    import subprocess
    nm = subprocess.run(["nm", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
    return {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TtDdBb"}


@pytest.mark.parametrize("flags", SPH_OPTION_SETS)
def test_sph_glue_closes_the_extended_link_recipe(pkg, flags, tmp_path):
    """INTEGRATION.md's recipe of a gas run drops density.o, hydra.o and ngb.o as well: with -DNGRAVS_GLUE_SPH the glue, compiled
    -Wall -Wextra -Werror against tests/glue_stub_sph, defines every name of tests/golden/glue_required_symbols_sph.json under
    its guards; without the macro it defines none of the five SPH entry points"""
    import json
    import subprocess
    obj = str(tmp_path / "gadget_glue.o")
    base = ["gcc", "-c", "-O0", "-Wall", "-Wextra", "-Werror"] + GLUE_DEFS + _includes() + flags
    out = subprocess.run(base + ["-DNGRAVS_GLUE_SPH", _glue(pkg), "-o", obj], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    defined = _defined(obj)
    macros = {f[2:].split("=")[0] for f in flags}
    golden = json.load(open(os.path.join(ROOT, "tests", "golden", "glue_required_symbols_sph.json")))
    assert golden["recipe_drops"][-3:] == ["density.c", "hydra.c", "ngb.c"]
    req = golden["required"]
    assert {"density", "hydro_force", "ngb_treeallocate", "ngb_treebuild"} <= set(req)
    missing = []
    for name, rec in req.items():
        on = True
        for g in rec["guards"]:
            assert g.startswith("#ifdef"), g
            on = on and g.replace("#ifdef", "").strip() in macros
        if on and name not in defined:
            missing.append("%s (%s, called from %s)" % (name, rec["defined"], rec["used_by"][0]))
    assert not missing, "gadget_glue.o does not define: " + ", ".join(missing)
    assert set(SPH_SYMBOLS) <= defined
    undefined = {ln.split()[-1] for ln in subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout.splitlines()}
    assert {"ngravs_sph_hsml_guess", "ngravs_sph_density", "ngravs_sph_hydro", "endrun"} <= undefined
    assert "ngravs_sph_accelerations" not in undefined        # density() does what its name says, alone
    # without the macro: what the glue defines today
    out = subprocess.run(base + [_glue(pkg), "-o", obj], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    plain = _defined(obj)
    assert not (set(SPH_SYMBOLS) & plain) and plain == defined - set(SPH_SYMBOLS) - {"DummyNode", "FatherLen", "FatherOnDummy", "SphCol",
                                                                                    "SphTs", "SphColLen", "sph_columns", "sph_begin"}


@pytest.mark.parametrize("switch", ["-DTWODIMS", "-DLONG_X=2", "-DLONG_Y=2", "-DLONG_Z=2", "-DSPH_BND_PARTICLES"])
def test_sph_glue_refuses_what_the_library_does_not_provide(pkg, switch):
    import subprocess
    cmd = ["gcc", "-fsyntax-only"] + GLUE_DEFS + _includes() + ["-DPERIODIC", "-DNGRAVS_GLUE_SPH", switch, _glue(pkg)]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode != 0 and "#error" in out.stderr and switch[2:].split("=")[0] in out.stderr, out.stderr
    cmd.remove("-DNGRAVS_GLUE_SPH")                            # the plain glue does not look at these switches
    assert subprocess.run(cmd, capture_output=True, text=True).returncode == 0


def test_sph_stubs_declare_what_the_reference_declares(pkg):
    """tests/glue_stub_sph/{allvars,proto}.h against tests/golden/glue_stub_sph_check.json (tools/glue_stub_check.py --sph, from the
    reference's headers: names, types, extents, field order, lines): same types and extents, the fields of struct
    sph_particle_data and struct particle_data in the reference's order, same prototypes, nothing the reference lacks; and a
    superset of what tests/glue_stub declares"""
    import json
    spec = importlib.util.spec_from_file_location("glue_stub_check", os.path.join(ROOT, "tools", "glue_stub_check.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    want = json.load(open(os.path.join(ROOT, "tests", "golden", "glue_stub_sph_check.json")))
    assert want["missing_in_reference"] == []
    sv = g.stub_view(g.STUB_SPH, g.STRUCTS_SPH)
    n = 0
    for sname, fields in sv["structs"].items():
        last = -1
        for name, t, ext in fields:
            r = want["structs"][sname].get(name)
            assert r is not None, "struct %s: the stub declares %s, the reference does not" % (sname, name)
            assert [t, ext] in r["forms"], (sname, name, t, ext, r)
            if sname in ("particle_data", "sph_particle_data", "NODE"):
                assert r["order"] > last, "struct %s: %s is out of the reference's order" % (sname, name)
                last = r["order"]
            n += 1
    assert [f[0] for f in sv["structs"]["sph_particle_data"]] == ["Entropy", "Density", "Hsml", "Left", "Right", "NumNgb", "Pressure", "DtEntropy",
                                                                  "HydroAccel", "VelPred", "DivVel", "CurlVel", "Rot", "DhsmlDensityFactor",
                                                                  "MaxSignalVel"]
    assert len(want["structs"]["sph_particle_data"]) == 15 and {"len", "mass", "father"} <= set(want["structs"]["NODE"])
    for name, (t, ext) in sv["globals"].items():
        r = want["globals"].get(name)
        assert r is not None and (r["type"], r["extent"]) == (t, ext), (name, t, ext, r)
        n += 1
    for name, (ret, params) in sv["prototypes"].items():
        r = want["prototypes"].get(name)
        assert r is not None and (r["returns"], r["parameters"]) == (ret, list(params)), (name, ret, params, r)
        n += 1
    assert {"N_gas", "RestartFlag", "Ngblist"} <= set(sv["globals"]) and set(SPH_SYMBOLS) <= set(sv["prototypes"])
    for k in ("DesNumNgb", "MaxNumNgbDeviation", "ArtBulkViscConst", "Timebase_interval", "Omega0", "OmegaLambda", "Hubble", "CPU_HydCompWalk",
              "CPU_HydCommSumm", "CPU_HydImbalance", "CPU_EnsureNgb"):
        assert k in [f[0] for f in sv["structs"]["global_data_all_processes"]], k
    base = g.stub_view()                                        # defaults unchanged: the stubs of tests/glue_stub
    for sname, fields in base["structs"].items():
        assert set(fields) <= set(sv["structs"][sname]), sname
    assert set(base["globals"].items()) <= set(sv["globals"].items()) and set(base["prototypes"]) <= set(sv["prototypes"])
    print("%d declarations of the SPH stubs agree with the reference's headers" % n)
    assert n > 120


# ---- the glue, executed -----------------------------------------------------------------------------------------------------
SPH_FIELDS = ("Entropy", "Density", "Hsml", "Left", "Right", "NumNgb", "Pressure", "DtEntropy", "HydroAccel0", "HydroAccel1", "HydroAccel2",
              "VelPred0", "VelPred1", "VelPred2", "DivVel", "CurlVel", "Rot0", "Rot1", "Rot2", "DhsmlDensityFactor", "MaxSignalVel")
GLUE_CASES = [("plummer", False), ("uniform", True)]
NGAS_GLUE, NOTHER_GLUE, BOX = 3000, 3000, 1000.0
T_DRIVER = 60.0                  # a driver run takes about 2 s (three stages on 6 000 particles); the limit only ends a hung child
_GLUE_RUNS = {}


def glue_inputs(pkg, kind):
    n = NGAS_GLUE + NOTHER_GLUE
    rng = np.random.default_rng(77)
    if kind == "uniform":
        pos, mass, _ = pkg.ic.uniform_box(n, box=BOX, n_gravs=1, seed=77)
        soft = [BOX / (40 * n ** (1 / 3))] * 6
    else:
        pos, mass, _ = pkg.ic.plummer_sphere(n, seed=77)
        soft = [0.01] * 6
    ptype = np.where(np.arange(n) < NGAS_GLUE, 0, 1).astype(np.int32)      # the gas particles are the first N_gas rows of P[]
    mass = np.where(ptype == 0, mass * rng.uniform(0.9, 1.1, n), mass)
    vel = rng.normal(0.0, 1.0, (n, 3)) - (0.02 * (pos - 0.5 * BOX) if kind == "uniform" else 2.0 * pos)   # a converging flow
    u = 10.0 ** rng.uniform(-0.5, 0.5, n)
    return pos, mass, ptype, vel, u, soft


def read_stages(path, n, ngas):
    raw = np.fromfile(path, dtype=np.float64)
    per = 12 + 21 * ngas + 9 * n
    assert len(raw) == 3 * per
    stages = []
    for s in range(3):
        blk = raw[s * per:(s + 1) * per]
        hd = blk[:12]
        assert (hd[0], hd[1], hd[2]) == (s, n, ngas)
        sph = blk[12:12 + 21 * ngas].reshape(ngas, 21)
        st = {k: sph[:, j] for j, k in enumerate(SPH_FIELDS)}
        st["sph"] = sph
        st["P"] = blk[12 + 21 * ngas:].reshape(n, 9)
        st["timers"] = hd[3:7]
        st["father_reset"], st["node_untouched"], st["host_loop_ok"] = hd[7], hd[8], hd[9]
        stages.append(st)
    return stages


def glue_run(pkg, kind, periodic):
    """the driver built with the glue and run twice (with and without the gas calls of the two steps), each child under its own
    time limit; once per case and module"""
    import subprocess
    import tempfile
    if kind in _GLUE_RUNS:
        return _GLUE_RUNS[kind]
    pos, mass, ptype, vel, u, soft = glue_inputs(pkg, kind)
    n = len(pos)
    tbi = H.KIND_TBI[kind]
    opts = ["-DPERIODIC", "-DPMGRID=32"] if periodic else []
    libdir = os.path.dirname(pkg.LIB_PATH)
    with tempfile.TemporaryDirectory(prefix="glue_sph_") as tmp:
        exe = os.path.join(tmp, "glue_sph_run")
        cmd = ["gcc", "-O1", "-Wall", "-Wextra", "-Werror"] + GLUE_DEFS + ["-DNGRAVS_GLUE_SPH", "-DN_GRAVS=1", "-DYUKAWA_IMASS=60"] + opts + \
            _includes() + [_glue(pkg), os.path.join(ROOT, "tests", "glue_stub_sph", "glue_sph_driver.c"), "-o", exe, "-L" + libdir,
                           "-lngravs_hip", "-lm", "-lpthread", "-Wl,-rpath," + libdir]
        b = subprocess.run(cmd, capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        rows = np.column_stack([pos, mass, ptype.astype(np.float64), vel, u])
        runs = {}
        for gas_calls in (1, 0):
            hd = np.array([n, NGAS_GLUE, gas_calls, 1.0, BOX if periodic else 0.0, 0.5, 0.005, SR.DES, SR.DEV, SR.VISC, tbi] + soft)
            fin, fout = os.path.join(tmp, "in%d.bin" % gas_calls), os.path.join(tmp, "out%d.bin" % gas_calls)
            with open(fin, "wb") as f:
                f.write(hd.tobytes())
                f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
            r = subprocess.run([exe, fin, fout, tmp + "/"], capture_output=True, text=True, timeout=T_DRIVER)
            assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
            assert "Begin Ngb-tree construction." in r.stdout and "Ngb-Tree contruction finished" in r.stdout
            runs[gas_calls] = read_stages(fout, n, NGAS_GLUE)
    _GLUE_RUNS[kind] = dict(pos=pos, mass=mass, ptype=ptype, vel=vel, u=u, soft=soft, tbi=tbi, gas=runs[1], plain=runs[0])
    return _GLUE_RUNS[kind]


def _full(n, gas, values, fill=0.0):
    return H.full(n, gas, values, fill=fill)


@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", GLUE_CASES)
def test_sph_glue_runs_on_the_gpu(pkg, have_lib, kind, periodic):
    """gadget_glue.c -DNGRAVS_GLUE_SPH EXECUTED with tests/glue_stub_sph/glue_sph_driver.c, one task: init()'s sequence, a first step,
    a step on the kept tree with one gas particle in three active.  SphP[] is what Engine.sph_hsml_guess / sph_density / sph_hydro
    give for the same inputs, bit for bit (the same library, the same calls); the pressure and the entropy conversion are the numpy
    lines (pow of the C library against numpy's: 1e-15)."""
    g = glue_run(pkg, kind, periodic)
    pos, mass, ptype, vel, u, tbi = g["pos"], g["mass"], g["ptype"], g["vel"], g["u"], g["tbi"]
    s0, s1, s2 = g["gas"]
    n, gas = len(pos), np.arange(NGAS_GLUE)
    GAMMA = SR.GAMMA
    for st in g["gas"] + g["plain"]:
        assert st["host_loop_ok"] == 1 and st["father_reset"] == 1 and st["node_untouched"] == 1
    cfg = pkg.make_config(n_gravs=1, periodic=int(periodic), pmgrid=32 if periodic else 0, box_size=BOX if periodic else 0.0, G=1.0, theta=0.5,
                          err_tol_force_acc=0.005, softening=g["soft"], walk_mode=pkg.WALK_GROUP, tree_alloc_factor=0.8)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.domain_Decomposition()
    eng.force_treebuild()
    # ---- init(): the guess, then density() from it
    h0 = eng.sph_hsml_guess(SR.DES, np.zeros(n), only_unset=True)
    d0 = eng.sph_density(vel, h0, SR.DES, SR.DEV)
    g["h0"], g["rounds0"] = h0, d0["max_rounds"]
    pairs = (("Hsml", "hsml"), ("Density", "density"), ("NumNgb", "num_ngb"), ("DivVel", "div_vel"), ("CurlVel", "curl_vel"),
             ("DhsmlDensityFactor", "dhsml_factor"))
    for a, b in pairs:
        assert np.array_equal(s0[a], d0[b][gas]), a
    assert SR.rel(s0["Pressure"], u[gas] * s0["Density"] ** GAMMA) <= 1e-15
    assert SR.rel(s0["Entropy"], (GAMMA - 1) * u[gas] / s0["Density"] ** (GAMMA - 1)) <= 1e-15
    assert np.all(s0["sph"][:, 8:11] == 0) and np.all(s0["DtEntropy"] == 0) and np.all(s0["Left"] == 0) and np.all(s0["Right"] == 0)
    # ---- step 1: density() again (from the converged lengths), the pressure line, hydro_force()
    d1 = eng.sph_density(vel, _full(n, gas, s0["Hsml"]), SR.DES, SR.DEV)
    for a, b in pairs:
        assert np.array_equal(s1[a], d1[b][gas]), a
    assert SR.rel(s1["Pressure"], s0["Entropy"] * s1["Density"] ** GAMMA) <= 1e-15
    col = {"hsml": "Hsml", "density": "Density", "pressure": "Pressure", "dhsml_factor": "DhsmlDensityFactor", "div_vel": "DivVel",
           "curl_vel": "CurlVel"}
    hy1 = H.call(eng, vel, {k: _full(n, gas, s1[v]) for k, v in col.items()}, art_bulk_visc_const=SR.VISC, timestep=np.zeros(n, dtype=np.int32),
                 timebase_interval=tbi)
    assert np.array_equal(s1["sph"][:, 8:11], hy1["hydro_accel"][gas]) and np.array_equal(s1["DtEntropy"], hy1["dt_entropy"][gas])
    assert np.array_equal(s1["MaxSignalVel"], hy1["max_signal_vel"][gas])
    assert np.any(s1["DtEntropy"] != 0) and np.all(s1["MaxSignalVel"] > 0)
    assert np.array_equal(s1["Entropy"], s0["Entropy"])
    # ---- step 2: the kept tree, drifted positions, one in three active, two rungs
    ids = np.arange(n)
    act = ids % 3 == 1
    beg = np.where(ids % 2 == 1, 4, 0)
    end = np.where(act, 8, np.where(ids % 2 == 1, 12, 16))
    assert np.array_equal(s2["P"][:, 5], beg) and np.array_equal(s2["P"][:, 6], end)
    pos2 = pos + 1e-3 * (BOX if periodic else 1.0) * np.sin(0.37 * (ids + 1.0)[:, None] + 1.3 * np.arange(3)[None, :])
    eng.update_particles(pos2, mass, ptype, active=act.astype(np.uint8))
    d2 = eng.sph_density(vel, _full(n, gas, s1["Hsml"]), SR.DES, SR.DEV)
    on, off = gas[act[gas]], gas[~act[gas]]
    assert len(on) == NGAS_GLUE // 3
    for a, b in pairs:
        assert np.array_equal(s2[a][on], d2[b][on]), a
    dt_entr = (8 - (beg + end) // 2) * tbi
    assert SR.rel(s2["Pressure"][on], ((s1["Entropy"] + s1["DtEntropy"] * dt_entr[gas]) * s2["Density"] ** GAMMA)[on]) <= 1e-15
    assert np.any(s2["Pressure"][on] != (s1["Entropy"] * s2["Density"] ** GAMMA)[on])          # DtEntropy of step 1 entered
    hy2 = H.call(eng, vel, {k: _full(n, gas, s2[v]) for k, v in col.items()}, art_bulk_visc_const=SR.VISC, timestep=(end - beg).astype(np.int32),
                 timebase_interval=tbi)
    assert np.array_equal(s2["sph"][on, 8:11], hy2["hydro_accel"][on]) and np.array_equal(s2["DtEntropy"][on], hy2["dt_entropy"][on])
    assert np.array_equal(s2["MaxSignalVel"][on], hy2["max_signal_vel"][on])
    assert np.array_equal(s2["sph"][off], s1["sph"][off])                                      # inactive gas rows keep every field
    eng.close()
    # ---- gravity is what the same driver gives without the gas calls; the timers grew
    # (P[].OldAcc holds |GravAccel + GravPM|, and the mesh force is summed by atomics: equal to rounding in a TreePM run)
    for a, b in zip(g["gas"], g["plain"]):
        assert np.array_equal(a["P"][:, 0:3], b["P"][:, 0:3]) and np.array_equal(a["P"][:, 4:], b["P"][:, 4:])
        assert np.abs(a["P"][:, 3] - b["P"][:, 3]).max() <= 1e-12 * np.abs(b["P"][:, 3]).max()
    assert np.any(s1["P"][:, 0:3] != 0) and np.any(s2["P"][:, 0:3] != s1["P"][:, 0:3])
    t0, t1, t2 = s0["timers"], s1["timers"], s2["timers"]
    assert 0 < t0[0] < t1[0] < t2[0] and 0 <= t0[1] <= t1[1] <= t2[1]                          # CPU_HydCompWalk, CPU_HydCommSumm
    assert t2[2] == 0 and t2[3] == 0                                                           # one task: no imbalance; EnsureNgb is not reported
    assert np.all(g["plain"][2]["timers"] == g["plain"][0]["timers"])


@pytest.mark.gpu
@pytest.mark.parametrize("kind,periodic", GLUE_CASES)
def test_sph_glue_against_the_reference_itself(pkg, have_lib, kind, periodic):
    """SphP[] after the first step of the driver against oracle/ref_sph.run on the same inputs: density() from the device's guess,
    then hydro_force(), with the entropy as init() converted it.  The comparisons and TOL of tests/test_sph_reference.py."""
    assert R.available(), "oracle/_ref/ref_sph_* are absent on this machine (%s where the reference tree is)" % R.MAKE_TARGET
    g = glue_run(pkg, kind, periodic)
    pos, mass, ptype, vel, tbi = g["pos"], g["mass"], g["ptype"], g["vel"], g["tbi"]
    n, gas = len(pos), np.arange(NGAS_GLUE)
    s0, s1, _ = g["gas"]
    if "h0" not in g:
        eng = make_engine(pkg, periodic, pos, mass, ptype)
        g["h0"] = eng.sph_hsml_guess(SR.DES, np.zeros(n), only_unset=True)
        g["rounds0"] = eng.sph_density(vel, g["h0"], SR.DES, SR.DEV)["max_rounds"]
        eng.close()
    box = BOX if periodic else 0.0
    ts = np.zeros(n, dtype=np.int32)
    out = R.run(pos, mass, ptype, vel, g["h0"], box=box, des=SR.DES, dev=SR.DEV, entropy=_full(n, gas, s0["Entropy"]), visc=SR.VISC, timestep=ts,
                tbi=tbi, timeout=SR.T_SMALL)
    assert g["rounds0"] == out["passes"], (g["rounds0"], out["passes"])
    res = {b: _full(n, gas, s1[a]) for a, b in (("Hsml", "hsml"), ("Density", "density"), ("NumNgb", "num_ngb"), ("DivVel", "div_vel"),
                                                ("CurlVel", "curl_vel"), ("DhsmlDensityFactor", "dhsml_factor"))}
    SR.device_density_vs_reference(res, out, pos, mass, vel, ptype, gas, box, "glue, " + kind)
    assert SR.rel(s1["Pressure"], out["pressure"][gas]) <= TOL
    hyd = {"hydro_accel": np.zeros((n, 3)), "dt_entropy": _full(n, gas, s1["DtEntropy"]), "max_signal_vel": _full(n, gas, s1["MaxSignalVel"])}
    hyd["hydro_accel"][gas] = s1["sph"][:, 8:11]
    ref_col = {k: H.full(n, gas, out[k][gas]) for k in H.COLS}
    SR.device_hydro_vs_reference(hyd, out, pos, mass, vel, ptype, gas, ref_col, box, "glue, " + kind, timestep=ts, tbi=tbi)
