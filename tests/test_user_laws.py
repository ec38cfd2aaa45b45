"""User-defined force laws (ngravs_create_with_laws): host tabulation, creation checks, and the tree-only kernels that
evaluate the tables (strict walk, group walk, direct sum) against the built-in laws and a numpy direct sum."""
import math
import os
import shutil
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
YM_IMASS = 60.0


# ---- Python copies of the reference's laws (same formulas, other addresses) ----------------------------------------------
def newton(t, s, r2, r, N):
    return s / r2


def plummer(t, s, h, r, N):
    hi = 1.0 / h
    u = r * hi
    if u < 0.5:
        return s * hi ** 3 * (10.666666666667 + u * u * (32.0 * u - 38.4))
    return s * hi ** 3 * (21.333333333333 - 48.0 * u + 38.4 * u * u - 10.666666666667 * u ** 3 - 0.066666666667 / u ** 3)


def yukawa_of(box):
    ym = YM_IMASS / box

    def yukawa(t, s, r2, r, N):
        return s * math.exp(-r * ym) * (ym / r + 1.0 / r2)
    return yukawa


def coloyuk_of(box):
    y = yukawa_of(box)

    def coloyuk(t, s, r2, r, N):
        return y(t, s, r2, r, N) + s / r2
    return coloyuk


def power25(t, s, r2, r, N):
    return s / r ** 2.5


def wiring(ng, accel, spline):
    return {"accel": [[accel(i, j) for j in range(ng)] for i in range(ng)],
            "spline": [[spline(i, j) for j in range(ng)] for i in range(ng)]}


# ---- CPU ---------------------------------------------------------------------------------------------------------------
def test_new_exports_and_header_is_c(pkg, have_lib):
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("ngravs_create_with_laws", "ngravs_shortrange_table_with_laws", "ngravs_user_table_eval", "ngravs_last_walk_kernel"):
        assert (" T " + sym) in nm, sym
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("no C compiler")
    src = '#include "ngravs_hip.h"\nstatic double f(double a, double b, double c, double d, long N) { return b / c; }\n' \
          'int main(void) { ngravs_user_fn_t u = {NGRAVS_USER_ACCEL, 0, f}; return u.fn == 0; }\n'
    r = subprocess.run([cc, "-std=c99", "-Wall", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"), "-x", "c", "-"],
                       input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr


@pytest.mark.parametrize("name", ["newton", "yukawa", "power2.5"])
def test_accel_tabulation_error(pkg, have_lib, name):
    box = 1000.0
    f = {"newton": newton, "yukawa": yukawa_of(box), "power2.5": power25}[name]
    r_lo, r_hi = 0.05, math.sqrt(3.0) * box
    rng = np.random.default_rng(5)
    r = np.exp(rng.uniform(math.log(r_lo), math.log(r_hi), 100000))
    got, fit_err = pkg.user_table_eval(pkg.abi.USER_ACCEL, f, r, r_lo=r_lo, r_hi=r_hi)
    want = np.array([f(1.0, 1.0, x * x, x, 1) for x in r])
    rel = np.abs(got - want) / np.abs(want)
    assert rel.max() <= 1e-9, (name, rel.max(), fit_err)


def test_spline_tabulation_error(pkg, have_lib):
    h = 0.028
    r = np.random.default_rng(6).uniform(0, h, 100000)
    got, _ = pkg.user_table_eval(pkg.abi.USER_SPLINE, plummer, r, h=h)
    want = np.array([plummer(1.0, 1.0, h, x, 1) for x in r])
    assert (np.abs(got - want) / np.abs(want)).max() <= 1e-9


def test_user_normed_gives_the_builtin_shortrange_table(pkg, have_lib):
    L, N = 1000.0, 64
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=N, box_size=L, wiring="c4")
    force_b, pot_b = pkg.shortrange_table(cfg)
    asmth = pkg.abi.ASMTH * L / N
    ym = 4 * math.pi * asmth * (YM_IMASS / (2 * math.pi)) / L

    def normed_pgdelta(t, s, k2, k, n):
        return 1.0

    def normed_pgcoloyuk(t, s, k2, k, n):
        return k2 / (k2 + ym * ym) * math.exp(-ym * ym * 0.25) + 1.0
    U = pkg.abi.LAW_USER0
    cfg.law_normed[0][0], cfg.law_normed[1][1] = U, U
    cfg.law_normed[0][1], cfg.law_normed[1][0] = U + 1, U + 1
    force_u, pot_u = pkg.shortrange_table_with_laws(cfg, [(pkg.abi.USER_NORMED, normed_pgdelta), (pkg.abi.USER_NORMED, normed_pgcoloyuk)])
    assert np.abs(force_u - force_b).max() <= 1e-12 * np.abs(force_b).max()
    assert np.abs(pot_u - pot_b).max() <= 1e-12 * np.abs(pot_b).max()


def _create_status(pkg, cfg, fns):
    try:
        eng = pkg.Engine(cfg, user_fns=fns)
    except pkg.NgravsError as e:
        return int(str(e).split("status ")[1].split()[0]), str(e)
    eng.close()
    return 0, ""


def test_refusals_need_no_gpu(pkg, have_lib):
    A, S = pkg.abi.USER_ACCEL, pkg.abi.USER_SPLINE
    U, US = pkg.abi.LAW_USER0, pkg.abi.SPLINE_USER0
    WIRING = -6
    # not linear in the source mass
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6, wiring=wiring(1, lambda i, j: U, lambda i, j: 1))
    rc, msg = _create_status(pkg, cfg, [(A, lambda t, s, r2, r, N: s * s / r2)])
    assert rc == WIRING and "linear in the source mass" in msg
    # depends on the target mass / on N
    rc, _ = _create_status(pkg, cfg, [(A, lambda t, s, r2, r, N: t * s / r2)])
    assert rc == WIRING
    rc, _ = _create_status(pkg, cfg, [(A, lambda t, s, r2, r, N: N * s / r2)])
    assert rc == WIRING
    # asymmetric user pair: [0][1] and [1][0] are different laws
    cfg = pkg.make_config(n_gravs=2, softening=[0.01] * 6,
                          wiring=wiring(2, lambda i, j: U if i <= j else U + 1, lambda i, j: 1))
    rc, msg = _create_status(pkg, cfg, [(A, newton), (A, lambda t, s, r2, r, N: 2 * s / r2)])
    assert rc == WIRING and "Newton's third law" in msg
    # a user law with periodic tree-only
    cfg = pkg.make_config(n_gravs=1, periodic=1, box_size=10.0, softening=[0.01] * 6, wiring=wiring(1, lambda i, j: U, lambda i, j: 1))
    rc, msg = _create_status(pkg, cfg, [(A, newton)])
    assert rc == WIRING and "periodic" in msg
    # registry index out of range / wrong kind
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6, wiring=wiring(1, lambda i, j: U + 3, lambda i, j: 1))
    rc, msg = _create_status(pkg, cfg, [(A, newton)])
    assert rc == WIRING and "outside the registry" in msg
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6, wiring=wiring(1, lambda i, j: U, lambda i, j: US))
    rc, msg = _create_status(pkg, cfg, [(A, newton)])
    assert rc == WIRING and "another kind" in msg
    # a Green's function must not depend on masses
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6, wiring=dict(wiring(1, lambda i, j: 1, lambda i, j: 1), greens=[[U]]))
    rc, _ = _create_status(pkg, cfg, [(pkg.abi.USER_GREENS, lambda t, s, k2, k, N: s / k2)])
    assert rc == WIRING
    # a user spline paired with a built-in the host cannot probe (a BAM spline)
    cfg = pkg.make_config(n_gravs=2, softening=[0.01] * 6,
                          wiring=wiring(2, lambda i, j: 1, lambda i, j: US if i <= j else pkg.abi.SPLINE_SOURCEBAM))
    rc, msg = _create_status(pkg, cfg, [(S, plummer)])
    assert rc == WIRING and "cannot be probed" in msg


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _run(pkg, cfg, pos, mass, typ, fns=None, mode=None):
    eng = pkg.Engine(cfg, user_fns=fns)
    if mode is not None:
        eng.set_walk_mode(mode)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=False)
    acc, _, cost = eng.get_accel()
    return eng, acc, cost


def _rel(a, b):
    return np.abs(a - b).max() / np.sqrt(np.mean(np.sum(b * b, axis=1)))


def _plummer_ic(pkg, n, ng, seed):
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=seed)
    if ng == 2:
        typ = np.where(np.arange(n) % 2 == 0, 1, 2).astype(np.int32)
    return pos, mass, typ


@pytest.mark.gpu
@pytest.mark.parametrize("ng", [1, 2])
@pytest.mark.parametrize("mode", ["strict", "group"])
def test_user_copies_of_newton_and_plummer_tree_only(pkg, ng, mode):
    n = 20000
    pos, mass, typ = _plummer_ic(pkg, n, ng, seed=31 + ng)
    wm = pkg.WALK_STRICT if mode == "strict" else pkg.WALK_GROUP
    t2g = [0, 0, 1 if ng == 2 else 0, 0, 0, 0]
    base = dict(n_gravs=ng, G=1.0, theta=0.5, softening=[0.01] * 6, type_to_grav=t2g, walk_mode=wm)
    cfg_b = pkg.make_config(wiring="newton", **base)
    cfg_u = pkg.make_config(wiring=wiring(ng, lambda i, j: pkg.abi.LAW_USER0, lambda i, j: pkg.abi.SPLINE_USER0 + 1), **base)
    e_b, a_b, c_b = _run(pkg, cfg_b, pos, mass, typ)
    e_u, a_u, c_u = _run(pkg, cfg_u, pos, mass, typ, fns=[(pkg.abi.USER_ACCEL, newton), (pkg.abi.USER_SPLINE, plummer)])
    want = pkg.abi.KERNEL_STRICT_USER if mode == "strict" else pkg.abi.KERNEL_GROUP_USER
    assert e_u.last_walk_kernel() == want
    assert e_b.last_walk_kernel() == (pkg.abi.KERNEL_STRICT if mode == "strict" else pkg.abi.KERNEL_GROUP)
    if mode == "strict":
        assert np.array_equal(c_u, c_b)
    assert _rel(a_u, a_b) <= 1e-9
    e_b.close()
    e_u.close()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["strict", "group"])
def test_user_yukawa_copies_beside_builtin_newton(pkg, mode):
    """tree-only C4-like wiring: [0][0] built-in Newton, the other three slots user Coloyuk copies"""
    n, box = 20000, 1000.0
    pos, mass, typ = pkg.ic.uniform_box(n, box=box, n_gravs=2, seed=17)
    wm = pkg.WALK_STRICT if mode == "strict" else pkg.WALK_GROUP
    base = dict(n_gravs=2, box_size=box, G=1.0, theta=0.5, softening=[box / 2000] * 6,
                type_to_grav=pkg.ic.default_type_to_grav(2), walk_mode=wm)
    U = pkg.abi.LAW_USER0
    cfg_b = pkg.make_config(wiring=wiring(2, lambda i, j: 1 if i == j == 0 else pkg.LAW_COLOYUK, lambda i, j: 1), **base)
    cfg_u = pkg.make_config(wiring=wiring(2, lambda i, j: 1 if i == j == 0 else U, lambda i, j: 1), **base)
    e_b, a_b, c_b = _run(pkg, cfg_b, pos, mass, typ)
    e_u, a_u, c_u = _run(pkg, cfg_u, pos, mass, typ, fns=[(pkg.abi.USER_ACCEL, coloyuk_of(box))])
    if mode == "strict":
        assert np.array_equal(c_u, c_b)
    assert _rel(a_u, a_b) <= 1e-9
    e_b.close()
    e_u.close()


@pytest.mark.gpu
def test_law_without_builtin_direct_sum_and_walk(pkg):
    """F = m (1 + alpha exp(-r/lambda)) / r^2 with lambda unlike YUKAWA_IMASS"""
    n, alpha, lam, eps = 6000, 0.7, 0.37, 0.01
    pos, mass, typ = pkg.ic.plummer_sphere(n, seed=9)
    h = 2.8 * eps

    def fifth(t, s, r2, r, N):
        return s * (1.0 + alpha * math.exp(-r / lam)) / r2
    cfg = pkg.make_config(n_gravs=1, G=1.0, theta=0.3, softening=[eps] * 6,
                          wiring=wiring(1, lambda i, j: pkg.abi.LAW_USER0, lambda i, j: pkg.abi.SPLINE_USER0 + 1),
                          walk_mode=pkg.WALK_STRICT)
    eng, a_w, _ = _run(pkg, cfg, pos, mass, typ, fns=[(pkg.abi.USER_ACCEL, fifth), (pkg.abi.USER_SPLINE, plummer)])
    idx = np.arange(0, n, 23, dtype=np.int32)
    a_d = eng.direct_sum(idx)
    # numpy fp64 direct sum
    want = np.zeros((len(idx), 3))
    for k, i in enumerate(idx):
        d = pos - pos[i]
        r = np.sqrt(np.sum(d * d, axis=1))
        fac = np.zeros(n)
        far = r >= h
        fac[far] = mass[far] * (1.0 + alpha * np.exp(-r[far] / lam)) / r[far] ** 3
        near = (~far) & (r > 0)
        fac[near] = np.array([plummer(1.0, m, h, x, 1) for m, x in zip(mass[near], r[near])])
        want[k] = np.sum(d * fac[:, None], axis=0)
    assert _rel(a_d, want) <= 1e-9
    err = np.linalg.norm(a_w[idx] - a_d, axis=1) / np.linalg.norm(a_d, axis=1)
    assert np.sqrt(np.mean(err ** 2)) <= 2e-3
    eng.close()


def test_glue_registers_unknown_laws_instead_of_ending_the_run(pkg):
    """host/gadget_glue.c: a wired function the glue has no built-in for becomes a registry entry of ngravs_create_with_laws"""
    glue = os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")
    src = open(glue).read()
    assert "has no device implementation" not in src and "endrun(1051)" not in src
    obj = os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue_user_laws_test.o")
    cmd = ["gcc", "-c", "-O0", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION",
           "-DUNEQUALSOFTENINGS", "-I" + os.path.join(ROOT, "tests", "glue_stub"), "-I" + os.path.join(ROOT, "include"), glue, "-o", obj]
    try:
        out = subprocess.run(cmd, capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        undefined = subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout
        assert "ngravs_create_with_laws" in undefined and "ngravs_create\n" in undefined
    finally:
        if os.path.exists(obj):
            os.remove(obj)


# ---- TreePM ---------------------------------------------------------------------------------------------------------------
TPM_N, TPM_L, TPM_GRID = 20000, 1000.0, 64


def treepm_user_fns():
    """user copies of coloyuk / pgcoloyuk / normed_pgcoloyuk for the TreePM box (ngravs.c:826-834; k2 as pm_periodic.c:490 and
    the short-range table pass it)"""
    asmth = 1.25 * TPM_L / TPM_GRID
    ym2 = (YM_IMASS / (2 * math.pi)) ** 2
    yfac = math.exp(-ym2 * (2 * math.pi * asmth / TPM_L) ** 2)
    ymn = 4 * math.pi * asmth * (YM_IMASS / (2 * math.pi)) / TPM_L

    def pgcoloyuk(t, s, k2, k, n):
        return 1.0 / k2 + yfac / (k2 + ym2)

    def normed_pgcoloyuk(t, s, k2, k, n):
        return k2 / (k2 + ymn * ymn) * math.exp(-ymn * ymn * 0.25) + 1.0
    return [(0, coloyuk_of(TPM_L)), (2, pgcoloyuk), (3, normed_pgcoloyuk)]


def treepm_config(pkg, user, walk_mode):
    U = pkg.abi.LAW_USER0
    diag = lambda i, j: i == j == 0  # noqa: E731
    w = {"accel": [[1 if diag(i, j) else (U if user else pkg.LAW_COLOYUK) for j in range(2)] for i in range(2)],
         "spline": [[1, 1], [1, 1]],
         "greens": [[1 if diag(i, j) else (U + 1 if user else pkg.LAW_COLOYUK) for j in range(2)] for i in range(2)],
         "normed": [[1 if diag(i, j) else (U + 2 if user else pkg.LAW_COLOYUK) for j in range(2)] for i in range(2)]}
    return pkg.make_config(n_gravs=2, periodic=1, pmgrid=TPM_GRID, box_size=TPM_L, G=1.0, theta=0.5,
                           softening=[TPM_L / (40 * TPM_N ** (1 / 3))] * 6, type_to_grav=pkg.ic.default_type_to_grav(2),
                           wiring=w, walk_mode=walk_mode)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["strict", "group"])
def test_treepm_user_yukawa_copies_one_task(pkg, mode):
    pos, mass, typ = pkg.ic.uniform_box(TPM_N, box=TPM_L, n_gravs=2, seed=23)
    wm = pkg.WALK_STRICT if mode == "strict" else pkg.WALK_GROUP
    out = {}
    for user in (False, True):
        eng = pkg.Engine(treepm_config(pkg, user, wm), user_fns=treepm_user_fns() if user else None)
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=True)
        acc, _, cost, pm = eng.get_accel(want_pm=True)
        out[user] = (acc, cost, pm, eng.last_walk_kernel())
        eng.close()
    (a_b, c_b, p_b, k_b), (a_u, c_u, p_u, k_u) = out[False], out[True]
    assert k_u == (pkg.abi.KERNEL_STRICT_USER if mode == "strict" else pkg.abi.KERNEL_GROUP_USER)
    assert k_b == (pkg.abi.KERNEL_STRICT if mode == "strict" else pkg.abi.KERNEL_GROUP)
    assert np.abs(p_u - p_b).max() <= 1e-12 * np.abs(p_b).max()
    assert _rel(a_u + p_u, a_b + p_b) <= 1e-9
    if mode == "strict":
        assert np.array_equal(c_u, c_b)


def _treepm_dist_worker(rank, world, port, out_dir, mode):
    import sys
    os.environ["MASTER_ADDR"] = "127.0.0.1"
    os.environ["MASTER_PORT"] = str(port)
    sys.path.insert(0, ROOT)
    import importlib
    import torch.distributed as dist
    import __graft_entry__ as ge
    dist.init_process_group("gloo", rank=rank, world_size=world)
    pkg = ge.load_package()
    dd = importlib.import_module("ngravs_amd.distributed")
    pos, mass, typ = pkg.ic.uniform_box(TPM_N, box=TPM_L, n_gravs=2, seed=23)
    mine = np.arange(rank, TPM_N, world)
    wm = pkg.WALK_STRICT if mode == "strict" else pkg.WALK_GROUP
    res = {}
    for user in (0, 1):
        eng = dd.DistributedEngine(treepm_config(pkg, user, wm), user_fns=treepm_user_fns() if user else None)
        eng.set_particles(pos[mine], mass[mine], typ[mine], ids=mine)
        eng.compute_accelerations(pm_step=True)
        acc, _, _, pm = eng.get_accel(want_pm=True)
        res["ids%d" % user], res["acc%d" % user], res["pm%d" % user] = eng.local_ids(), acc, pm
        eng.close()
    np.savez(os.path.join(out_dir, "u%d.npz" % rank), **res)
    dist.destroy_process_group()


@pytest.mark.gpu
@pytest.mark.parametrize("mode", ["strict", "group"])
def test_treepm_user_yukawa_copies_two_tasks_gloo(pkg, tmp_path, mode):
    import torch.multiprocessing as mp
    world = 2
    port = 31700 + (os.getpid() % 2000) + (0 if mode == "strict" else 7)
    mp.spawn(_treepm_dist_worker, args=(world, port, str(tmp_path), mode), nprocs=world, join=True)
    full = {}
    for user in (0, 1):
        acc, pm = np.zeros((TPM_N, 3)), np.zeros((TPM_N, 3))
        for r in range(world):
            d = np.load(os.path.join(str(tmp_path), "u%d.npz" % r))
            acc[d["ids%d" % user]] = d["acc%d" % user]
            pm[d["ids%d" % user]] = d["pm%d" % user]
        full[user] = (acc, pm)
    (a_b, p_b), (a_u, p_u) = full[0], full[1]
    assert np.abs(p_u - p_b).max() <= 1e-12 * np.abs(p_b).max()
    assert _rel(a_u + p_u, a_b + p_b) <= 1e-9


# ---- the glue with a model's own laws ---------------------------------------------------------------------------------------
def _glue_run(pkg, tmp_path, opts, user, n, periodic):
    root = ROOT
    L = 1.0
    if periodic:
        pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=2, seed=5)
    else:
        pos, mass, typ = pkg.ic.plummer_sphere(n, seed=5)
        typ = (1 + (np.arange(n) % 2)).astype(np.int32)
    eps = (L / (40 * n ** (1 / 3))) if periodic else 0.01
    soft = [eps, eps, 1.5 * eps, eps, eps, eps]
    hd = np.array([n, 1.0, L if periodic else 0.0, 0.5, 0.005] + soft, dtype=np.float64)
    tag = "u" if user else "b"
    fin, fout = str(tmp_path / ("in_%s.bin" % tag)), str(tmp_path / ("out_%s.bin" % tag))
    with open(fin, "wb") as f:
        f.write(hd.tobytes())
        f.write(np.ascontiguousarray(np.column_stack([pos, mass, typ.astype(np.float64)]), dtype=np.float64).tobytes())
    exe = str(tmp_path / ("glue_%s" % tag))
    libdir = os.path.dirname(pkg.LIB_PATH)
    extra = (["-Dset_softenings=glue_set_softenings"] if user else [])
    srcs = [os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")]
    objs = []
    base = ["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION", "-DUNEQUALSOFTENINGS",
            "-DN_GRAVS=2", "-DYUKAWA_IMASS=60"] + opts + ["-I" + os.path.join(root, "tests", "glue_stub"), "-I" + os.path.join(root, "include")]
    for k, src in enumerate(srcs):
        o = str(tmp_path / ("glue_%s_%d.o" % (tag, k)))
        b = subprocess.run(base + extra + ["-c", src, "-o", o], capture_output=True, text=True)
        assert b.returncode == 0, b.stderr[-3000:]
        objs.append(o)
    more = [os.path.join(root, "tests", "glue_stub", "glue_driver.c")]
    if user:
        more.append(os.path.join(root, "tests", "glue_user_model", "user_model.c"))
    b = subprocess.run(base + objs + more + ["-o", exe, "-L" + libdir, "-lngravs_hip", "-lm", "-lpthread", "-Wl,-rpath," + libdir],
                       capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, fin, fout, str(tmp_path) + "/"], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "endrun" not in r.stdout + r.stderr, (r.stdout[-2000:], r.stderr[-2000:])
    ntask = max([int(o.split("=")[1]) for o in opts if o.startswith("-DGLUE_NTASK")] + [1])
    out = np.zeros((3, n, 8))
    for t in range(ntask):
        raw = np.fromfile(fout + ".%d" % t, dtype=np.float64)
        at = 0
        for step in range(3):
            k = int(raw[at])
            blk = raw[at + 1: at + 1 + 9 * k].reshape(k, 9)
            at += 1 + 9 * k
            out[step, blk[:, 8].astype(np.int64) - 1] = blk[:, :8]
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("opts", [[], ["-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0"], ["-DPERIODIC", "-DPMGRID=32"],
                                  ["-DPERIODIC", "-DPMGRID=32", "-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0"]])
def test_glue_with_a_models_own_newton_and_plummer(pkg, have_lib, tmp_path, opts):
    """the glue registers the model's copies (unknown addresses) as user-defined laws instead of ending the run: the same
    GravAccel and GravPM as the built-in wiring, on 1 and 2 tasks, tree-only and TreePM"""
    periodic = "-DPERIODIC" in opts
    n = 20000 if periodic else 6000
    ob = _glue_run(pkg, tmp_path, opts, False, n, periodic)
    ou = _glue_run(pkg, tmp_path, opts, True, n, periodic)
    for step in range(3):
        for cols in (slice(0, 3), slice(3, 6)):
            b, u = ob[step, :, cols], ou[step, :, cols]
            scale = np.sqrt(np.mean(np.sum(b * b, axis=1)))
            if scale > 0:
                assert np.abs(u - b).max() <= 1e-9 * scale, (step, cols)
