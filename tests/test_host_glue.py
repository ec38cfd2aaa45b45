"""The plain-C host (same call sequence and AoS strides as gadget-2.0.7-ngravs_amd/host/gadget_glue.c)."""
import os
import subprocess

import pytest


def _build(pkg):
    host = os.path.join(os.path.dirname(pkg.__file__), "host")
    exe = os.path.join(host, "host_shim_test")
    inc = os.path.join(os.path.dirname(pkg.__file__), "..", "include")
    libdir = os.path.dirname(pkg.LIB_PATH)
    subprocess.check_call(["gcc", "-O2", "-Wall", "-DWITH_RCCL", os.path.join(host, "host_shim_test.c"), "-I" + inc, "-L" + libdir,
                           "-lngravs_hip", "-lngravs_rccl", "-lm", "-lpthread", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe])
    return exe


def test_c_host_links_against_the_abi(pkg, have_lib):
    """CPU: the C host compiles against include/ngravs_hip.h and links against the library"""
    exe = _build(pkg)
    assert os.path.exists(exe)


@pytest.mark.parametrize("flags", [[], ["-DPERIODIC", "-DPMGRID=64"], ["-DPERIODIC", "-DPMGRID=64", "-DFORCETEST=0.1"],
                                   ["-DFORCETEST=0.1", "-DN_GRAVS=3"], ["-DPERIODIC"], ["-DPERIODIC", "-DPMGRID=64", "-DNGRAVS_WITH_RCCL"]])
def test_glue_compiles_against_the_reference_interface(pkg, flags):
    """gadget_glue.c is what a maintainer drops into the reference tree.  The reference cannot be built here (GSL, FFTW-2),
    so the glue is compiled -fsyntax-only -Wall -Wextra -Werror against tests/glue_stub/: declarations of exactly the
    globals / prototypes it touches (names and layouts from SURVEY.md 8(a'), 8(b)), for the tree-only, TreePM and FORCETEST
    variants of the reference's Makefile options."""
    root = os.path.join(os.path.dirname(pkg.__file__), "..")
    glue = os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")
    cmd = ["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION",
           "-DUNEQUALSOFTENINGS", "-I" + os.path.join(root, "tests", "glue_stub"), "-I" + os.path.join(root, "include")] + flags + [glue]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    # single precision P[] must be refused at compile time, not read as garbage
    cmd.remove("-DDOUBLEPRECISION")
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode != 0 and "DOUBLEPRECISION" in out.stderr


def test_glue_refuses_an_odd_pmgrid(pkg):
    """The library's mesh is [N][N][N+2], the in-place transform's padding only for even N (the reference pads to
    PMGRID2 = 2*(PMGRID/2+1)): an odd PMGRID is refused when the glue is compiled, an even one that is no power of two is not."""
    root = os.path.join(os.path.dirname(pkg.__file__), "..")
    glue = os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")
    base = ["gcc", "-fsyntax-only", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION",
            "-DUNEQUALSOFTENINGS", "-I" + os.path.join(root, "tests", "glue_stub"), "-I" + os.path.join(root, "include")]
    out = subprocess.run(base + ["-DPERIODIC", "-DPMGRID=33", glue], capture_output=True, text=True)
    assert out.returncode != 0 and "even PMGRID" in out.stderr
    out = subprocess.run(base + ["-DPERIODIC", "-DPMGRID=96", glue], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr


OPTION_SETS = [[], ["-DPERIODIC", "-DPMGRID=64"], ["-DPERIODIC", "-DPMGRID=64", "-DFORCETEST=0.1"], ["-DFORCETEST=0.1", "-DN_GRAVS=3"],
               ["-DPERIODIC"], ["-DPERIODIC", "-DPMGRID=64", "-DNGRAVS_WITH_RCCL"]]


@pytest.mark.parametrize("flags", OPTION_SETS)
def test_glue_defines_every_symbol_the_link_recipe_needs(pkg, flags, tmp_path):
    """INTEGRATION.md's recipe drops gravtree.o forcetree.o pm_periodic.o domain.o peano.o gravtree_forcetest.o from the
    reference's OBJS and adds gadget_glue.o.  tests/golden/glue_required_symbols.json (written by tools/glue_required_symbols.py
    in the build container: NAMES of the non-static functions those six units define and a kept unit calls, with the #if guards
    of their definitions) says what the kept objects will look for; the glue, compiled to an object against the interface
    stubs, must define every one of them under the same options -- checked with nm, so a forgotten symbol is a test failure
    here instead of a link error in the maintainer's tree."""
    import json
    root = os.path.join(os.path.dirname(pkg.__file__), "..")
    glue = os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")
    obj = str(tmp_path / "gadget_glue.o")
    cmd = ["gcc", "-c", "-O0", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION",
           "-DUNEQUALSOFTENINGS", "-I" + os.path.join(root, "tests", "glue_stub"), "-I" + os.path.join(root, "include")] + flags + \
          [glue, "-o", obj]
    out = subprocess.run(cmd, capture_output=True, text=True)
    assert out.returncode == 0, out.stderr
    nm = subprocess.run(["nm", "--defined-only", obj], capture_output=True, text=True, check=True).stdout
    defined = {ln.split()[-1] for ln in nm.splitlines() if len(ln.split()) >= 3 and ln.split()[-2] in "TtDdBb"}
    macros = {f[2:].split("=")[0] for f in flags}
    req = json.load(open(os.path.join(root, "tests", "golden", "glue_required_symbols.json")))["required"]
    assert len(req) >= 16
    missing = []
    for name, rec in req.items():
        on = True
        for g in rec["guards"]:
            m = g.replace("#ifdef", "").strip()
            assert g.startswith("#ifdef"), g      # the only guard form on these definitions
            on = on and m in macros
        if on and name not in defined:
            missing.append("%s (%s, called from %s)" % (name, rec["defined"], rec["used_by"][0]))
    assert not missing, "gadget_glue.o does not define: " + ", ".join(missing)
    # and it must not define what a KEPT unit defines (duplicate symbols at link time)
    undefined = {ln.split()[-1] for ln in subprocess.run(["nm", "-u", obj], capture_output=True, text=True).stdout.splitlines()}
    for kept_symbol in ("endrun", "second", "timediff", "do_box_wrapping", "get_random_number"):
        assert kept_symbol not in defined
    assert {"endrun", "ngravs_create", "ngravs_gravity_tree"} <= undefined
    if "-DNGRAVS_WITH_RCCL" in flags:      # the exchanges go through the C RCCL communicator, MPI only broadcasts the id
        assert {"ngravs_rccl_create", "ngravs_rccl_fill", "MPI_Bcast"} <= undefined and "MPI_Isend" not in undefined


def test_glue_source_mentions_every_entry_point(pkg):
    src = open(os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c")).read()
    for name in ("void domain_Decomposition(void)", "int force_treebuild(int npart)", "void gravity_tree(void)",
                 "void pmforce_periodic(void)", "void force_treeallocate(int maxnodes, int maxpart)",
                 "void force_treefree(void)", "peanokey peano_hilbert_key(int x, int y, int z, int bits)",
                 "void peano_hilbert_order(void)", "void pm_init_periodic(void)"):
        assert name in src, name


@pytest.mark.gpu
def test_c_host_runs_on_gpu(pkg, have_lib):
    exe = _build(pkg)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout, out.stderr)
    assert out.returncode == 0, out.stdout + out.stderr


@pytest.mark.gpu
@pytest.mark.parametrize("opts,ng,nsmall", [(["-DPERIODIC", "-DPMGRID=32", "-DFORCETEST=0.02"], 2, 0), ([], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=32", "-DFORCETEST=0.02", "-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0"], 2, 0),
                                            (["-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0"], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=32", "-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0"], 3, 0),
                                            (["-DPERIODIC", "-DFORCETEST=0.02", "-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0"], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=32", "-DNGRAVS_WITH_RCCL"], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=16", "-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0"], 2, 2),
                                            (["-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0"], 2, 40),
                                            (["-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0", "-DNGRAVS_GLUE_WALK_STRICT"], 2, 0),
                                            (["-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0", "-DNGRAVS_GLUE_WALK_STRICT", "-DLOOSE_THETA"], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=32", "-DGLUE_NTASK=2", "-DNGRAVS_GLUE_DEVICE=0", "-DNGRAVS_GLUE_WALK_STRICT"], 2, 0),
                                            (["-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0", "-DNGRAVS_GLUE_TEST_KEPT_FALLBACK"], 2, 0),
                                            (["-DPERIODIC", "-DPMGRID=32", "-DGLUE_NTASK=3", "-DNGRAVS_GLUE_DEVICE=0", "-DNGRAVS_GLUE_TEST_KEPT_FALLBACK"], 2, 0)])
def test_glue_runs_on_the_gpu(pkg, have_lib, tmp_path, opts, ng, nsmall):
    """gadget_glue.c EXECUTED, not only compiled: built against the interface stubs together with tests/glue_stub/glue_driver.c (the
    reference's globals, MPI for 1-3 tasks as forked processes over shared memory, second / endrun / do_box_wrapping /
    get_random_number) it runs the reference's own call sequence of a first step -- pm_init_periodic, domain_Decomposition,
    pmforce_periodic, gravity_tree twice (accel.c:44-52: the second call must see the OldAcc the first one wrote),
    gravity_forcetest -- and of a short-range step with one particle in five active, on P[] with the byte strides of struct
    particle_data.  One task: P[].GravAccel / GravCost are what the library gives the Python host for the same calls, bit for bit
    (GravPM, summed by atomics, and the OldAcc it enters to rounding).  Two / three tasks (P[] migrated by the glue with whole
    particle_data records, exchanges staged through host memory by the MPI vtable): every particle on exactly one task, GravPM of
    the single mesh to 1e-10, the production walk's force as two valid groupings agree; with the glue built for the reference walk
    (-DNGRAVS_GLUE_WALK_STRICT) several tasks give the single task's GravAccel to 1e-10 with IDENTICAL GravCost after the second
    gravity_tree() of the first step -- also with a loose opening angle and a tight ErrTolForceAcc (-DLOOSE_THETA: 0.9 / 0.0005),
    where the relative criterion of the second call opens top leaves the Barnes-Hut call never asked for: the glue decides the import
    again before it (accel.c:44-52).  A third step keeps decomposition and tree (domain.c:76, drifted particles, another active set); the
    two -DNGRAVS_GLUE_TEST_KEPT_FALLBACK variants make the glue take its way out of a kept step whose walk missed a leaf (wrap, decompose
    again, walk again) although nothing was missing.  Always: inactive rows keep their values;
    forcetest.txt holds one line per tested particle (appended task by task) whose direct sum agrees with tree + PM.  The last variant
    builds the glue with -DNGRAVS_WITH_RCCL: its communicator is libngravs_rccl.so (created from an MPI_Bcast id, self-tested), one task."""
    import numpy as np
    root = os.path.join(os.path.dirname(pkg.__file__), "..")
    pm = any(o.startswith("-DPMGRID") for o in opts)
    pmg = max([int(o.split("=")[1]) for o in opts if o.startswith("-DPMGRID")] + [0])
    ntask = max([int(o.split("=")[1]) for o in opts if o.startswith("-DGLUE_NTASK")] + [1])
    periodic = "-DPERIODIC" in opts
    n, L = (20000 if pm or not periodic else 6000), 1.0      # (periodic tree-only: the lattice walk and its direct sum are the slow ones)
    if nsmall:
        n = nsmall                                            # a handful of particles on three tasks: a task with NumPart = 0
    if periodic:
        pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=5)
    else:
        pos, mass, typ = pkg.ic.plummer_sphere(n, seed=5)
        typ = (1 + (np.arange(n) % ng)).astype(np.int32)
    eps = (L / (40 * n ** (1 / 3))) if periodic else 0.01
    soft = [eps, eps, 1.5 * eps, eps, eps, eps]
    strict = "-DNGRAVS_GLUE_WALK_STRICT" in opts
    theta, etfa = (0.9, 0.0005) if "-DLOOSE_THETA" in opts else (0.5, 0.005)
    opts = [o for o in opts if o != "-DLOOSE_THETA"]
    hd = np.array([n, 1.0, L if periodic else 0.0, theta, etfa] + soft, dtype=np.float64)
    rows = np.column_stack([pos, mass, typ.astype(np.float64)])
    fin, fout = str(tmp_path / "in.bin"), str(tmp_path / "out.bin")
    with open(fin, "wb") as f:
        f.write(hd.tobytes())
        f.write(np.ascontiguousarray(rows, dtype=np.float64).tobytes())
    exe = str(tmp_path / "glue_run")
    libdir = os.path.dirname(pkg.LIB_PATH)
    cmd = ["gcc", "-O1", "-Wall", "-Wextra", "-Werror", "-DNGRAVS_BUILD_INSIDE_REFERENCE", "-DDOUBLEPRECISION", "-DUNEQUALSOFTENINGS",
           "-DN_GRAVS=%d" % ng, "-DYUKAWA_IMASS=60"] + opts + ["-I" + os.path.join(root, "tests", "glue_stub"), "-I" + os.path.join(root, "include"),
           os.path.join(os.path.dirname(pkg.__file__), "host", "gadget_glue.c"), os.path.join(root, "tests", "glue_stub", "glue_driver.c"),
           "-o", exe, "-L" + libdir, "-lngravs_hip"] + (["-lngravs_rccl"] if "-DNGRAVS_WITH_RCCL" in opts else []) + ["-lm", "-lpthread", "-Wl,-rpath," + libdir]
    b = subprocess.run(cmd, capture_output=True, text=True)
    assert b.returncode == 0, b.stderr[-3000:]
    r = subprocess.run([exe, fin, fout, str(tmp_path) + "/"], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0, (r.stdout[-2000:], r.stderr[-2000:])
    nstep = 3
    out = np.zeros((nstep, n, 8))
    seen = np.zeros((nstep, n), dtype=np.int64)
    own = []
    for t in range(ntask):
        raw = np.fromfile(fout + ".%d" % t, dtype=np.float64)
        at = 0
        for step in range(nstep):
            k = int(raw[at])
            blk = raw[at + 1: at + 1 + 9 * k].reshape(k, 9)
            at += 1 + 9 * k
            ids = blk[:, 8].astype(np.int64) - 1
            out[step, ids] = blk[:, :8]
            seen[step, ids] += 1
            own.append(k)
        assert at == len(raw)
    assert np.all(seen == 1)                                                # every particle on exactly one task, both steps
    # the same calls from the Python host (one task)
    cfg = pkg.make_config(n_gravs=ng, periodic=1 if periodic else 0, pmgrid=pmg if pm else 0, box_size=L if periodic else 0.0, G=1.0, theta=theta,
                          err_tol_force_acc=etfa, softening=soft, type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="c4",
                          walk_mode=pkg.WALK_STRICT if strict else pkg.WALK_GROUP, tree_alloc_factor=0.8)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, typ, grav_cost=np.zeros(n, dtype=np.float32))
    eng.compute_accelerations(pm_step=pm)
    _, old1, _ = eng.get_accel()
    eng.set_old_acc(old1)
    eng.set_opening(0.0, etfa)
    eng.gravity_tree()
    if pm:
        a2, o2, c2, p2 = eng.get_accel(want_pm=True)
    else:
        a2, o2, c2 = eng.get_accel()
        p2 = np.zeros((n, 3))
    s1 = out[0]

    def same(x, y, tol=1e-12):   # GravPM is summed by atomics (order varies from run to run): rounding noise there and in what it enters
        return np.abs(x - y).max() <= tol * max(np.abs(y).max(), 1e-300)

    def walks_agree(x, y, tot, loose=1.0):  # two valid groupings of the production walk (each within ErrTolForceAcc of the truth)
        if len(x) == 0:
            return True
        e = np.linalg.norm(x - y, axis=1) / np.linalg.norm(tot, axis=1)
        print("   production walk on %d task(s) vs one: |da|/|a| median %.1e, 99 %% %.1e, max %.1e" % (ntask, np.median(e), np.quantile(e, 0.99), e.max()))
        # (small tree-only sets are walked with 4 lanes per target, i.e. in groups of 16: the two groupings differ a little more)
        return np.median(e) < 5e-4 * loose and np.quantile(e, 0.99) < 5e-3 * loose and e.max() < 5e-2 * loose
    if ntask == 1:
        assert np.array_equal(s1[:, 0:3], a2) and same(s1[:, 3:6], p2) and same(s1[:, 6], o2)
        assert np.array_equal(s1[:, 7], c2.astype(np.float64))
    elif strict:
        # the reference walk: the forces of one task, target by target, with identical interaction counts -- after BOTH calls of the
        # first step (the second walks with the criterion and the OldAcc the import was decided again for)
        assert same(s1[:, 3:6], p2, 1e-10) and same(s1[:, 0:3], a2, 1e-10) and same(s1[:, 6], o2, 1e-10)
        assert np.array_equal(s1[:, 7], c2.astype(np.float64))
    else:
        assert same(s1[:, 3:6], p2, 1e-10) and walks_agree(s1[:, 0:3], a2, a2 + p2)
        assert np.abs(s1[:, 6] - o2).max() < 5e-2 * o2.max() and abs(s1[:, 7].mean() / c2.mean() - 1) < 0.05
    # step 2: one particle in five active, no PM force
    act = (np.arange(n) % 5 == 2).astype(np.uint8)
    eng.set_particles(pos, mass, typ, old_acc=o2, active=act, grav_pm=p2 if pm else None, grav_cost=c2)
    eng.compute_accelerations(pm_step=False)
    a3, o3, c3 = a2.copy(), o2.copy(), c2.copy()
    eng.get_accel(into=(a3, o3, c3))
    if True:
        # step 3: the drifted tree (domain.c:76 keeps decomposition and tree; the glue hands drifted positions over, the library refits;
        # several tasks: the kept decomposition, ngravs_host_kept_step)
        idn = np.arange(1, n + 1, dtype=np.float64)
        pos3 = pos + 1e-3 * (L if periodic else 1.0) * np.sin(0.37 * idn[:, None] + 1.3 * np.arange(3)[None, :])
        act3 = (np.arange(n) % 3 == 1).astype(np.uint8)
        eng.update_particles(pos3, mass, typ, old_acc=o3, active=act3)
        eng.gravity_tree()
        a4, o4, c4 = a3.copy(), o3.copy(), c3.copy()
        eng.get_accel(into=(a4, o4, c4))
        s3 = out[2]
        idle3 = act3 == 0
        if ntask == 1:
            assert same(s3[:, 0:3], a4) and same(s3[:, 6], o4) and np.mean(s3[:, 7] == c4.astype(np.float64)) > 0.999
        elif strict:
            assert same(s3[~idle3, 0:3], a4[~idle3], 1e-10) and np.array_equal(s3[~idle3, 7], c4[~idle3].astype(np.float64))
        else:
            assert walks_agree(s3[~idle3, 0:3], a4[~idle3], (a4 + p2)[~idle3], loose=4.0)
        if "-DNGRAVS_GLUE_TEST_KEPT_FALLBACK" in opts:
            # the glue's way out when a kept step's walk wanted a leaf that was never imported (ngravs_walk_unopened, all-reduced): wrap,
            # decompose again, walk again -- taken here on purpose (the sets of this test never need it: their imports hold)
            assert ntask > 1 and "decomposing again" in r.stdout
        else:
            assert "decomposing again" not in r.stdout                 # the kept decomposition held what the walk opened
        assert np.array_equal(s3[idle3, 0:3], out[1][idle3, 0:3]) and np.array_equal(s3[:, 3:6], out[0][:, 3:6])
    eng.close()
    s2 = out[1]
    idle = act == 0
    if ntask == 1:
        assert same(s2[:, 0:3], a3) and same(s2[:, 6], o3) and np.mean(s2[:, 7] == c3.astype(np.float64)) > 0.999
    elif strict:
        assert same(s2[~idle, 0:3], a3[~idle], 1e-10) and np.array_equal(s2[~idle, 7], c3[~idle].astype(np.float64))
    else:
        # (groups of 64 consecutive ACTIVE own particles are five times as wide, and cut differently on several tasks)
        assert walks_agree(s2[~idle, 0:3], a3[~idle], (a3 + p2)[~idle], loose=4.0)
    assert np.array_equal(s2[:, 3:6], s1[:, 3:6])                          # GravPM untouched by the short-range step (it travels with P[])
    assert np.array_equal(s2[idle, 0:3], s1[idle, 0:3]) and np.array_equal(s2[idle, 6], s1[idle, 6])   # inactive rows keep their values
    assert np.array_equal(s2[idle, 7], s1[idle, 7])
    print("glue on %d task(s), particles per task and step: %s" % (ntask, own))
    # timings.txt: the reference's block per gravity_tree() call (gravtree.c:408-444), six lines + a blank one, in its formats
    import re
    blocks = open(str(tmp_path / "timings.txt")).read().split("\n\n")
    blocks = [b for b in blocks if b.strip()]
    assert len(blocks) == 4                                 # first step: two calls; then one per step
    pat = [r"^Step= -?\d+  t= \S+  dt= \S+ $", r"^Nf= \d+\d{9}  total-Nf= \d+\d{9}  ex-frac= \S+  iter= \d+$",
           r"^work-load balance: \S+  max=\S+ avg=\S+ PE0=\S+$", r"^particle-load balance: \S+$", r"^max\. nodes: \d+, filled: \S+$",
           r"^part/sec=\S+ \| \S+  ia/part=\S+ \(\S+\)$"]
    for b in blocks:
        lines = b.split("\n")
        assert len(lines) == 6 and all(re.match(p_, ln) for p_, ln in zip(pat, lines)), lines
    nf = [int(b.split("\n")[1].split()[1]) for b in blocks]
    assert nf[0] == n and nf[1] == n                          # every particle is active on the first step
    ia = float(blocks[1].split("\n")[5].split("ia/part=")[1].split()[0])
    assert abs(ia / s1[:, 7].mean() - 1) < 1e-5               # ia/part is the mean of P[].GravCost (printed with %g: six digits)
    exf = float(blocks[1].split("\n")[1].split("ex-frac=")[1].split()[0])
    assert exf == 0 if ntask == 1 else (exf > 0 or n <= 100)
    if "-DFORCETEST=0.02" in opts:
        lines = [ln.split() for ln in open(str(tmp_path / "forcetest.txt"))]
        want = sum(1 for i in range(n) if ((((i + 1) * 2654435761) & 0xffffffff) ^ ((((i + 1) * 2654435761) & 0xffffffff) >> 15)) % 1000 < 20)
        # gravtree_forcetest.c:297-311: 16 columns with PMGRID (%.15e, tree and tree + PM), 13 without (%g, the tree force is the total)
        ncol = 16 if pm else 13
        assert len(lines) == want and all(len(ln) == ncol for ln in lines)
        t = np.array([[float(v) for v in ln] for ln in lines])
        direct, total = t[:, 6:9], (t[:, 12:15] if pm else t[:, 9:12])
        err = np.linalg.norm(total - direct, axis=1) / np.linalg.norm(direct, axis=1)
        ids = t[:, ncol - 1].astype(int) - 1
        assert np.allclose(t[:, 9:12], s1[ids, 0:3], rtol=1e-14 if pm else 1e-5, atol=0)  # the GravAccel column is P[].GravAccel
        print("forcetest.txt: %d lines, tree+PM vs direct sum rms %.2e max %.2e" % (len(lines), np.sqrt(np.mean(err ** 2)), err.max()))
        assert np.sqrt(np.mean(err ** 2)) < 2e-2


def test_stubs_declare_what_the_reference_declares(pkg):
    """tests/glue_stub/{allvars,proto,ngravs}.h are hand-written stand-ins for the reference's headers (which need GSL and FFTW-2).
    tools/glue_stub_check.py recorded, from the reference's headers, type / array extent / order of every struct field, the type
    of every global and the signature of every prototype the stubs declare (tests/golden/glue_stub_check.json: names and types
    only).  The stubs, parsed the same way, must say the same: same types and extents, struct particle_data's fields in the
    reference's order (it travels as raw bytes in the glue's particle exchange), same prototypes -- and nothing the reference lacks."""
    import importlib.util
    import json
    root = os.path.join(os.path.dirname(pkg.__file__), "..")
    spec = importlib.util.spec_from_file_location("glue_stub_check", os.path.join(root, "tools", "glue_stub_check.py"))
    g = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(g)
    want = json.load(open(os.path.join(root, "tests", "golden", "glue_stub_check.json")))
    assert want["missing_in_reference"] == []
    sv = g.stub_view()
    n = 0
    for sname, fields in sv["structs"].items():
        last = -1
        for name, t, ext in fields:
            r = want["structs"][sname].get(name)
            assert r is not None, "struct %s: the stub declares %s, the reference does not" % (sname, name)
            assert [t, ext] in r["forms"], (sname, name, t, ext, r)      # (forms: one per #ifdef branch of the reference, e.g. LONGIDS)
            if sname == "particle_data":
                assert r["order"] > last, "struct particle_data: %s is out of the reference's order" % name
                last = r["order"]
            n += 1
    for name, (t, ext) in sv["globals"].items():
        if name in ("All", "P"):
            continue
        r = want["globals"].get(name)
        assert r is not None and (r["type"], r["extent"]) == (t, ext), (name, t, ext, r)
        n += 1
    for name, (ret, params) in sv["prototypes"].items():
        r = want["prototypes"].get(name)
        assert r is not None and (r["returns"], r["parameters"]) == (ret, list(params)), (name, ret, params, r)
        n += 1
    print("%d declarations of the stubs agree with the reference's headers" % n)
    assert n > 90
