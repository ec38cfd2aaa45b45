"""Lattice corrections for user-defined force laws in periodic runs (ngravs_create_with_lattice): the host tabulation of a
model's own LatticeForce functions, the creation checks, and the periodic tree-only walks and the periodic direct sum with
user laws against the built-in wirings, the oracle, an Ewald golden and an independent numpy image sum."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from conftest import rel_err

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
YM_IMASS = 60.0
EN = 64


@pytest.fixture(scope="module")
def fx(tmp_path_factory):
    """tests/user_lattice/laws.c as a shared library"""
    out = str(tmp_path_factory.mktemp("user_lattice") / "liblaws.so")
    r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror",
                        os.path.join(HERE, "user_lattice", "laws.c"), "-o", out, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    for name in ("fx_set_box", "fx_set_yukawa_imass", "fx_set_screen_len"):
        getattr(lib, name).argtypes = [C.c_double]
        getattr(lib, name).restype = None
    lib.fx_set_yukawa_imass(YM_IMASS)
    return lib


def law(pkg, lib, name):
    return pkg.abi.GravityFn((name, lib))


def lattice(pkg, lib, name):
    return pkg.abi.LATTICE_FN((name, lib))


def _status(pkg, cfg, fns, lat):
    try:
        eng = pkg.Engine(cfg, user_fns=fns, user_lattice=lat)
    except pkg.NgravsError as e:
        return int(str(e).split("status ")[1].split()[0]), str(e)
    eng.close()
    return 0, ""


def user_wiring(pkg, cfg_b):
    """the built-in wiring of cfg_b with every Newton / Coloyuk accel and every Plummer spline replaced by the user copies of
    registry entries 0 (newton), 1 (plummer), 2 (coloyuk); the lattice function of each user pair"""
    ng = cfg_b.n_gravs
    U, US = pkg.abi.LAW_USER0, pkg.abi.SPLINE_USER0
    acc = {pkg.LAW_NEWTON: (U, "fx_ewald_lattice"), pkg.LAW_COLOYUK: (U + 2, "fx_coloyuk_lattice")}
    w = {"accel": [[acc[cfg_b.law_accel[i][j]][0] for j in range(ng)] for i in range(ng)],
         "spline": [[US + 1 for j in range(ng)] for i in range(ng)]}
    lat = [(i, j, acc[cfg_b.law_accel[i][j]][1]) for i in range(ng) for j in range(ng)]
    return w, lat


def trilinear(tab, box, d):
    """lat_lookup of the kernels in numpy: tab [3][65][65][65] (already / box^2), d (n, 3) nearest-image separations"""
    s = np.where(d < 0, 1.0, -1.0)
    u = np.abs(d) * (2 * EN / box)
    i = np.minimum(u.astype(np.int64), EN - 1)
    f = u - i
    out = np.zeros_like(d)
    for a in (0, 1):
        for b in (0, 1):
            for c in (0, 1):
                w = (f[:, 0] if a else 1 - f[:, 0]) * (f[:, 1] if b else 1 - f[:, 1]) * (f[:, 2] if c else 1 - f[:, 2])
                for k in range(3):
                    out[:, k] += w * tab[k][i[:, 0] + a, i[:, 1] + b, i[:, 2] + c]
    return s * out


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_new_exports_and_header_is_c(pkg, have_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("ngravs_create_with_lattice", "ngravs_user_lattice_table", "ngravs_create_with_laws"):
        assert (" T " + sym) in nm, sym
    src = ('#include "ngravs_hip.h"\n'
           'typedef void (*latforce)(int, int, int, double *, double *);\n'
           'static void g(int i, int j, int k, double *x, double *f) { (void)i; (void)j; (void)k; (void)x; f[0] = 0; }\n'
           'int main(void) { latforce l = g; ngravs_user_lattice_t e = {0, 1, l}; ngravs_ctx *c = 0; double t[3 * 65 * 65 * 65];\n'
           '  return ngravs_user_lattice_table(e.fn, 1.0, t) + ngravs_create_with_lattice(0, 0, 0, &e, 1, &c); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name,wiring", [("fx_ewald_lattice", "newton"), ("fx_yukawa_lattice", "yukawa")])
def test_lattice_table_equals_the_oracle(pkg, O, have_lib, fx, name, wiring):
    box = 1000.0
    w = wiring if wiring == "newton" else {"accel": [[pkg.LAW_YUKAWA]], "spline": [[1]]}
    cfg = pkg.make_config(n_gravs=1, periodic=1, box_size=box, softening=[1.0] * 6, wiring=w)
    cfg.yukawa_imass = YM_IMASS
    want = O.lattice_tables(cfg)[0, 0]
    got = pkg.user_lattice_table(lattice(pkg, fx, name), box)
    assert got.shape == want.shape
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()
    assert np.all(got[:, 0, 0, 0] == 0)            # fx_yukawa_lattice returns at the origin without writing force[]


def test_lattice_table_origin_and_non_finite(pkg, have_lib, fx):
    def early(i, j, k, x, force):   # a Python callable that writes nothing at the origin (and 1 elsewhere)
        if i or j or k:
            force[0] = force[1] = force[2] = 1.0
    t = pkg.user_lattice_table(early, 2.0)
    assert np.all(t[:, 0, 0, 0] == 0) and np.all(t[:, 1:, :, :] == 0.25)
    with pytest.raises(pkg.NgravsError) as e:
        pkg.user_lattice_table(lattice(pkg, fx, "fx_nan_lattice"), 1.0)
    assert "(3, 4, 5)" in str(e.value)


def test_refusals_need_no_gpu(pkg, have_lib, fx):
    WIRING = -6
    U = pkg.abi.LAW_USER0
    fns = [(pkg.abi.USER_ACCEL, law(pkg, fx, "fx_newton")), (pkg.abi.USER_SPLINE, law(pkg, fx, "fx_plummer"))]
    ew = lattice(pkg, fx, "fx_ewald_lattice")
    uw = {"accel": [[U, U], [U, U]], "spline": [[U + 1] * 2] * 2}
    per = dict(n_gravs=2, periodic=1, box_size=10.0, softening=[0.01] * 6, wiring=uw)
    full = [(i, j, ew) for i in range(2) for j in range(2)]
    # pair out of range, no function
    for bad in [(2, 0, ew), (0, -1, ew), (0, 0, None)]:
        rc, msg = _status(pkg, pkg.make_config(**per), fns, full[1:] + [bad])
        assert rc == WIRING and "out of range or no function" in msg, (bad, msg)
    # two entries for one pair
    rc, msg = _status(pkg, pkg.make_config(**per), fns, full + [(1, 1, ew)])
    assert rc == WIRING and "second entry" in msg
    # an entry on a pair wired with a built-in law
    cfg = pkg.make_config(**dict(per, wiring={"accel": [[1, U], [U, U]], "spline": [[U + 1] * 2] * 2}))
    rc, msg = _status(pkg, cfg, fns, full)
    assert rc == WIRING and "built-in" in msg
    # any entry in a non-periodic configuration
    cfg = pkg.make_config(n_gravs=2, softening=[0.01] * 6, wiring=uw)
    rc, msg = _status(pkg, cfg, fns, full[:1])
    assert rc == WIRING and "non-periodic" in msg
    # periodic tree-only: every user-accel pair needs one
    rc, msg = _status(pkg, pkg.make_config(**per), fns, full[:3])
    assert rc == WIRING and "periodic" in msg and "law_accel[1][1]" in msg


def test_screened_table_interpolation_error(pkg, have_lib, fx):
    """the trilinear-interpolation error of the 65^3 table of the screened law, which bounds its periodic direct sum below"""
    box = 100.0
    eps, scale = screened_interp_error(pkg, fx, box)
    print("screened lattice table: max trilinear error %.3e of max |correction| %.3e" % (eps, scale))
    assert 0 < eps < 5e-3 * scale


def screened_interp_error(pkg, fx, box, n=20000):
    fx.fx_set_screen_len(SCREEN)
    tab = pkg.user_lattice_table(lattice(pkg, fx, "fx_screened_lattice"), box)
    d = np.random.default_rng(4).uniform(-0.5 * box, 0.5 * box, (n, 3))
    got = trilinear(tab, box, d)
    f = lattice(pkg, fx, "fx_screened_lattice")
    want = np.zeros_like(d)
    for k in range(n):
        x = (C.c_double * 3)(*(np.abs(d[k]) / box))
        o = (C.c_double * 3)(0, 0, 0)
        f(-1, -1, -1, x, o)
        want[k] = -np.sign(d[k]) * np.array(o[:]) / box ** 2
    return np.abs(got - want).max(), np.abs(want).max()


# ---- GPU: periodic tree-only -------------------------------------------------------------------------------------------
def _case(pkg, wiring, ng, n=6000, L=100.0, seed=3, **kw):
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=seed)
    eps = L / (40 * n ** (1 / 3))
    cfg = pkg.make_config(n_gravs=ng, periodic=1, pmgrid=0, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, **kw)
    cfg.yukawa_imass = YM_IMASS
    return cfg, pos, mass, typ


def with_laws(cfg_b, w, walk_mode=None):
    """a copy of cfg_b with the accel / spline ids of w"""
    cfg = type(cfg_b).from_buffer_copy(cfg_b)
    for i in range(cfg.n_gravs):
        for j in range(cfg.n_gravs):
            cfg.law_accel[i][j], cfg.law_spline[i][j] = w["accel"][i][j], w["spline"][i][j]
    if walk_mode is not None:
        cfg.walk_mode = walk_mode
    return cfg


def _user_engine(pkg, fx, cfg_b, box):
    w, lat = user_wiring(pkg, cfg_b)
    fx.fx_set_box(box)
    fns = [(pkg.abi.USER_ACCEL, law(pkg, fx, "fx_newton")), (pkg.abi.USER_SPLINE, law(pkg, fx, "fx_plummer")),
           (pkg.abi.USER_ACCEL, law(pkg, fx, "fx_coloyuk"))]
    return pkg.Engine(with_laws(cfg_b, w), user_fns=fns, user_lattice=[(i, j, lattice(pkg, fx, f)) for i, j, f in lat])


def _rel(a, b):
    return np.abs(a - b).max() / np.sqrt(np.mean(np.sum(b * b, axis=1)))


@pytest.mark.gpu
@pytest.mark.parametrize("wiring,ng", [("newton", 1), ("c4", 2)])
def test_periodic_tree_only_user_copies_against_builtin(pkg, O, fx, wiring, ng):
    cfg_b, pos, mass, typ = _case(pkg, wiring, ng, walk_mode=pkg.WALK_STRICT)
    L = cfg_b.box_size
    idx = np.arange(0, len(pos), 30, dtype=np.int32)
    res = {}
    for user in (False, True):
        eng = _user_engine(pkg, fx, cfg_b, L) if user else pkg.Engine(cfg_b)
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=False)
        a_s, _, c_s = eng.get_accel()
        k_s = eng.last_walk_kernel()
        eng.set_walk_mode(pkg.WALK_GROUP)
        eng.gravity_tree()
        a_g, _, _ = eng.get_accel()
        k_g = eng.last_walk_kernel()
        res[user] = (a_s, c_s, k_s, a_g, k_g, eng.direct_sum(idx))
        eng.close()
    (a_sb, c_sb, k_sb, a_gb, k_gb, d_b), (a_su, c_su, k_su, a_gu, k_gu, d_u) = res[False], res[True]
    assert (k_sb, k_gb) == (pkg.abi.KERNEL_STRICT, pkg.abi.KERNEL_GROUP)
    assert (k_su, k_gu) == (pkg.abi.KERNEL_STRICT_USER, pkg.abi.KERNEL_GROUP_USER)
    assert np.array_equal(c_su, c_sb)
    assert _rel(a_su, a_sb) <= 1e-9
    assert _rel(a_gu, a_gb) <= 1e-9
    assert _rel(d_u, d_b) <= 1e-9
    # the user tables in the oracle's lattice-corrected direct sum and walk
    _, lat = user_wiring(pkg, cfg_b)
    tabs = np.zeros((ng, ng, 3, EN + 1, EN + 1, EN + 1))
    for i, j, f in lat:
        tabs[i, j] = pkg.user_lattice_table(lattice(pkg, fx, f), L)
    assert rel_err(d_u, O.direct_lattice(cfg_b, pos, mass, typ, idx, tabs)).max() < 1e-9
    T = O.Tree(cfg_b, pos, mass, typ)
    a_o, n_o = T.walk()
    a_o, n_o = O.lattice_walk(T, a_o, n_o, tabs)
    a_o, _ = O.finish(cfg_b, a_o)
    assert np.abs(a_su - a_o).max() / np.abs(a_o).max() < 1e-9
    assert np.array_equal(c_su.astype(np.int64), n_o)


# ---- GPU: TreePM with user Coloyuk copies and their lattice functions ---------------------------------------------------
@pytest.mark.gpu
def test_treepm_user_coloyuk_direct_sum_against_ewald_golden(pkg, fx):
    import sys
    sys.path.insert(0, os.path.join(HERE, "golden"))
    from make_ewald_golden import N, L, SEED, case_config
    gold = np.load(os.path.join(HERE, "golden", "ewald_truth_c4.npz"))
    pos, mass, typ = pkg.ic.uniform_box(N, box=L, n_gravs=2, seed=SEED)
    cfg_b, _ = case_config(pkg, "c4", 2, walk_mode=pkg.WALK_GROUP)
    idx = gold["idx"].astype(np.int32)
    out = {}
    for user in (False, True):
        if user:
            U = pkg.abi.LAW_USER0
            fx.fx_set_box(L)
            cfg = with_laws(cfg_b, {"accel": [[1, U], [U, 1]], "spline": [[1, 1], [1, 1]]})
            fx.fx_set_yukawa_imass(cfg.yukawa_imass)
            eng = pkg.Engine(cfg, user_fns=[(pkg.abi.USER_ACCEL, law(pkg, fx, "fx_coloyuk"))],
                             user_lattice=[(0, 1, lattice(pkg, fx, "fx_coloyuk_lattice")), (1, 0, lattice(pkg, fx, "fx_coloyuk_lattice"))])
        else:
            eng = pkg.Engine(cfg_b)
        eng.set_particles(pos, mass, typ, old_acc=gold["old_acc"])
        eng.set_opening(0.0, 0.005)
        eng.compute_accelerations(pm_step=True)
        acc, _, _, pm = eng.get_accel(want_pm=True)
        out[user] = (acc + pm, eng.direct_sum(idx), eng.last_walk_kernel())
        eng.close()
    (t_b, d_b, _), (t_u, d_u, k_u) = out[False], out[True]
    fx.fx_set_yukawa_imass(YM_IMASS)
    assert k_u == pkg.abi.KERNEL_GROUP_USER
    assert rel_err(d_u, gold["truth"]).max() < 2e-4
    assert _rel(d_u, d_b) <= 1e-9
    e = rel_err(t_u[idx], d_u)
    assert float(np.sqrt(np.mean(e ** 2))) < 1e-2


# ---- GPU: a screened law with no built-in counterpart ------------------------------------------------------------------
SCREEN = 0.1   # screening length in units of the box: the images beyond |n_i| <= 3 fall below exp(-25)


@pytest.mark.gpu
def test_screened_law_direct_sum_and_walks(pkg, fx):
    n, L = 3000, 100.0
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=1, seed=41)
    eps = L / (40 * n ** (1 / 3))
    h = 2.8 * eps
    lam = SCREEN * L
    fx.fx_set_box(L)
    fx.fx_set_screen_len(SCREEN)
    U, US = pkg.abi.LAW_USER0, pkg.abi.SPLINE_USER0
    cfg = pkg.make_config(n_gravs=1, periodic=1, box_size=L, G=1.0, theta=0.5, softening=[eps] * 6,
                          wiring={"accel": [[U]], "spline": [[US + 1]]}, walk_mode=pkg.WALK_STRICT)
    eng = pkg.Engine(cfg, user_fns=[(pkg.abi.USER_ACCEL, law(pkg, fx, "fx_screened")), (pkg.abi.USER_SPLINE, law(pkg, fx, "fx_plummer"))],
                     user_lattice=[(0, 0, lattice(pkg, fx, "fx_screened_lattice"))])
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    _, old, _ = eng.get_accel()
    idx = np.arange(0, n, 100, dtype=np.int32)
    d_gpu = eng.direct_sum(idx)
    # numpy: nearest image (softened inside h) plus every other image with |n_i| <= 3
    shifts = np.array([(a, b, c) for a in range(-3, 4) for b in range(-3, 4) for c in range(-3, 4) if a or b or c], dtype=float) * L
    want = np.zeros((len(idx), 3))
    for k, i in enumerate(idx):
        d = pos - pos[i]
        d -= L * np.round(d / L)
        r = np.sqrt(np.sum(d * d, axis=1))
        fac = np.zeros(n)
        far = r >= h
        fac[far] = mass[far] * np.exp(-r[far] / lam) / r[far] ** 3
        u = r / h
        near = (~far) & (r > 0)
        un = u[near]
        v = np.where(un < 0.5, 10.666666666667 + un * un * (32.0 * un - 38.4),
                     21.333333333333 - 48.0 * un + 38.4 * un * un - 10.666666666667 * un ** 3 - 0.066666666667 / un ** 3)
        fac[near] = mass[near] * v / h ** 3
        acc = np.sum(d * fac[:, None], axis=0)
        keep = r > 1e-5 * h
        di = d[keep][:, None, :] + shifts[None, :, :]
        ri = np.sqrt(np.sum(di * di, axis=2))
        acc += np.sum(di * (mass[keep][:, None] * np.exp(-ri / lam) / ri ** 3)[:, :, None], axis=(0, 1))
        want[k] = acc
    # tolerance: every source's image sum comes from the 65^3 table by trilinear interpolation, whose largest error eps_int
    # is measured on the host; the sum over the sources is off by at most sum(m) * eps_int
    eps_int, _ = screened_interp_error(pkg, fx, L)
    tol = mass.sum() * eps_int
    err = np.abs(d_gpu - want).max()
    print("screened law: direct sum vs numpy image sum %.3e, tolerance sum(m) * eps_int = %.3e" % (err, tol))
    assert err <= tol
    # the walks against the direct sum, at the accuracy tests/test_lattice.py accepts for built-in laws
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.gravity_tree()
    a_s, _, _ = eng.get_accel()
    assert eng.last_walk_kernel() == pkg.abi.KERNEL_STRICT_USER
    eng.set_walk_mode(pkg.WALK_GROUP)
    eng.gravity_tree()
    a_g, _, _ = eng.get_accel()
    assert eng.last_walk_kernel() == pkg.abi.KERNEL_GROUP_USER
    rms = lambda e: float(np.sqrt(np.mean(e ** 2)))  # noqa: E731
    e_s, e_g = rms(rel_err(a_s[idx], d_gpu)), rms(rel_err(a_g[idx], d_gpu))
    print("screened law: strict walk rms %.2e, group walk rms %.2e" % (e_s, e_g))
    assert e_s < 1e-2 and e_g <= e_s * 1.05
    eng.close()


# ---- GPU: two tasks over gloo ------------------------------------------------------------------------------------------
def _dist_worker(rank, world, port, out_dir, lib_path):
    import sys
    import importlib
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    import torch.distributed as dist
    import __graft_entry__ as ge
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    dd = importlib.import_module("ngravs_amd.distributed")
    lib = C.CDLL(lib_path)
    lib.fx_set_box.argtypes = [C.c_double]
    lib.fx_set_yukawa_imass.argtypes = [C.c_double]
    lib.fx_set_yukawa_imass(YM_IMASS)
    cfg_b, pos, mass, typ = _case(pkg, "c4", 2, walk_mode=pkg.WALK_STRICT)
    w, lat = user_wiring(pkg, cfg_b)
    lib.fx_set_box(cfg_b.box_size)
    cfg = with_laws(cfg_b, w)
    fns = [(pkg.abi.USER_ACCEL, law(pkg, lib, "fx_newton")), (pkg.abi.USER_SPLINE, law(pkg, lib, "fx_plummer")),
           (pkg.abi.USER_ACCEL, law(pkg, lib, "fx_coloyuk"))]
    mine = np.arange(rank, len(pos), world)
    eng = dd.DistributedEngine(cfg, user_fns=fns, user_lattice=[(i, j, lattice(pkg, lib, f)) for i, j, f in lat])
    eng.set_particles(pos[mine], mass[mine], typ[mine], ids=mine)
    eng.compute_accelerations(pm_step=False)
    acc, _, cost = eng.get_accel()
    np.savez(os.path.join(out_dir, "r%d.npz" % rank), ids=eng.local_ids(), acc=acc, cost=cost, kern=eng.last_walk_kernel())
    eng.close()
    dist.destroy_process_group()


@pytest.mark.gpu
def test_periodic_tree_only_user_law_two_tasks_gloo(pkg, fx, tmp_path):
    import torch.multiprocessing as mp
    world = 2
    port = 32900 + (os.getpid() % 2000)
    mp.spawn(_dist_worker, args=(world, port, str(tmp_path), fx._name), nprocs=world, join=True)
    cfg_b, pos, mass, typ = _case(pkg, "c4", 2, walk_mode=pkg.WALK_STRICT)
    eng = _user_engine(pkg, fx, cfg_b, cfg_b.box_size)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    a1, _, c1 = eng.get_accel()
    eng.close()
    acc, cost = np.zeros_like(a1), np.zeros_like(c1)
    for r in range(world):
        d = np.load(os.path.join(str(tmp_path), "r%d.npz" % r))
        assert int(d["kern"]) == pkg.abi.KERNEL_STRICT_USER
        acc[d["ids"]] = d["acc"]
        cost[d["ids"]] = d["cost"]
    assert _rel(acc, a1) <= 1e-9
    assert np.array_equal(cost, c1)


# ---- GPU: the glue with a model that brings its own LatticeForce ------------------------------------------------------------
def _glue_run(pkg, out_dir, opts, user, n):
    os.makedirs(out_dir, exist_ok=True)
    L = 1.0
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=5)
    eps = L / (40 * n ** (1 / 3))
    soft = [eps, eps, 1.5 * eps, eps, eps, eps]
    hd = np.array([n, 1.0, L, 0.5, 0.005] + soft, dtype=np.float64)
    fin, fout = os.path.join(out_dir, "in.bin"), os.path.join(out_dir, "out.bin")
    with open(fin, "wb") as f:
        f.write(hd.tobytes())
        f.write(np.ascontiguousarray(np.column_stack([pos, mass, typ.astype(np.float64)]), dtype=np.float64).tobytes())
    exe = os.path.join(out_dir, "glue")
    libdir = os.path.dirname(pkg.LIB_PATH)
    base = ["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION", "-DUNEQUALSOFTENINGS",
            "-DN_GRAVS=2", "-DYUKAWA_IMASS=60"] + opts + ["-I" + os.path.join(HERE, "glue_stub"), "-I" + os.path.join(ROOT, "include")]
    o = os.path.join(out_dir, "glue.o")
    b = subprocess.run(base + (["-Dset_softenings=glue_set_softenings"] if user else []) +
                       ["-c", os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c"), "-o", o], capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    more = [os.path.join(HERE, "glue_stub", "glue_driver.c")]
    if user:
        more.append(os.path.join(HERE, "glue_user_lattice_model", "model.c"))
    b = subprocess.run(base + [o] + more + ["-o", exe, "-L" + libdir, "-lngravs_hip", "-lm", "-lpthread", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    if user:
        assert " LatticeForce" in subprocess.run(["nm", "--defined-only", exe], capture_output=True, text=True).stdout
    r = subprocess.run([exe, fin, fout, out_dir + "/"], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0 and "endrun" not in r.stdout + r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    ntask = max([int(x.split("=")[1]) for x in opts if x.startswith("-DGLUE_NTASK")] + [1])
    out = np.zeros((3, n, 8))
    for t in range(ntask):
        raw = np.fromfile(fout + ".%d" % t, dtype=np.float64)
        at = 0
        for step in range(3):
            k = int(raw[at])
            blk = raw[at + 1: at + 1 + 9 * k].reshape(k, 9)
            at += 1 + 9 * k
            out[step, blk[:, 8].astype(np.int64) - 1] = blk[:, :8]
    ft = os.path.join(out_dir, "forcetest.txt")
    lines = [ln.split() for ln in open(ft)] if os.path.exists(ft) else []
    return out, lines


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [["-DPERIODIC"], ["-DPERIODIC", "-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0"],
                                  ["-DPERIODIC", "-DPMGRID=32", "-DFORCETEST=0.02"]])
def test_glue_with_a_models_own_lattice_force(pkg, have_lib, tmp_path, opts):
    """a model that wires its own Newton / Coloyuk copies and their LatticeForce: the periodic tree-only run and FORCETEST's
    periodic direct sum of a TreePM run give the built-in wiring's results"""
    n = 12000
    ob, lb = _glue_run(pkg, str(tmp_path / "b"), opts, False, n)
    ou, lu = _glue_run(pkg, str(tmp_path / "u"), opts, True, n)
    for step in range(3):
        for cols in (slice(0, 3), slice(3, 6)):
            b, u = ob[step, :, cols], ou[step, :, cols]
            scale = np.sqrt(np.mean(np.sum(b * b, axis=1)))
            if scale > 0:
                assert np.abs(u - b).max() <= 1e-9 * scale, (step, cols)
    if "-DFORCETEST=0.02" in opts:
        assert len(lb) > 0 and len(lu) == len(lb)
        db = np.array([[float(v) for v in ln[6:9]] for ln in lb])
        du = np.array([[float(v) for v in ln[6:9]] for ln in lu])
        assert _rel(du, db) <= 1e-9
