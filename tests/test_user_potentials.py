"""Potentials for any wired law (ngravs_create_with_potentials): the model's own PotentialFxns, PotentialSplines, LatticePotential
and LatticeZero, tabulated on the host and evaluated by the potential walk.  The model is tests/user_potential/model.c, the truth
tests/potential_user_ref.py: numpy pair sums over the same functions.  The tests hold the library to what the functions say.

Bounds:
  * a column against its pair sum: (1e-9 + 1e-12) G sum_j |term_ij| per row -- 1e-9 is the fit the library guarantees per term
    (UL_FAIL of user_laws.cpp), 1e-12 the rounding bound of test_potential.py.  Against the built-in engine at theta = 0.5 the
    same bound is used: a node's term is its monopole's, which for the one-signed Newtonian terms is the sum of its particles'
    terms to the order of the opening error.
  * one particle: |pot| <= 4 ulp of G m |pot_spline(1, 1, h, 0, 1)| (the walk's own term and the self term are the same table
    read with opposite signs).
  * own rows handed in as targets: bit for bit; G is a power of two.
  * lattice table: 1e-10 of max|table| (libm on host and numpy); mesh: 1e-10 of max|pot|.
  * against exact image sums: at most 1.5 x the deviation the numpy restatement shows on the same rows.  At 1037 particles the
    exact sums are taken for the first 32 rows (the coincident pair, the close pairs and the planted pairs): every source enters.
"""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import potential_ref as R
import potential_user_ref as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SIZES = (1, 2, 63, 65, 1037)
T2G = U.T2G
BOX = 10.0
MU = 6.0                 # open sets: per unit length; periodic sets: MU / BOX, i.e. 6 in box units
FIT = 1e-9 + 1e-12
WIRING = -6


@pytest.fixture(scope="module")
def mdl(tmp_path_factory):
    """tests/user_potential/model.c as a shared library"""
    out = str(tmp_path_factory.mktemp("user_potential") / "libmodel.so")
    r = subprocess.run(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", "-Wall", "-Wextra", "-Werror",
                        os.path.join(HERE, "user_potential", "model.c"), "-o", out, "-lm"], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    lib = C.CDLL(out)
    lib.mdl_set.argtypes = [C.c_double, C.c_double]
    lib.mdl_set.restype = None
    return lib


def law(pkg, lib, name):
    return pkg.abi.GravityFn((name, lib))


def latpot(pkg, lib, name):
    return pkg.abi.LATTICE_POT_FN((name, lib))


def entries(pkg, lib, model, with_psi=False):
    """the user_potentials list of a model {(a, b): Entry}"""
    return [(a, b, law(pkg, lib, e.names[0]), law(pkg, lib, e.names[1]), latpot(pkg, lib, e.names[2]) if with_psi else None, e.zero)
            for (a, b), e in sorted(model.items())]


def _cross(pkg):
    A = pkg.abi
    lw = [[A.LAW_NEWTON, A.LAW_NEG_NEWTON], [A.LAW_NEG_NEWTON, A.LAW_NEWTON]]
    return {"accel": lw, "spline": [[A.SPLINE_PLUMMER, A.SPLINE_NEG_PLUMMER], [A.SPLINE_NEG_PLUMMER, A.SPLINE_PLUMMER]], "greens": lw, "normed": lw}


def _mixed(pkg):
    """[0][0] Newton (keeps its built-in companion), every other pair coloyuk"""
    A = pkg.abi
    return {"accel": [[A.LAW_NEWTON, A.LAW_COLOYUK], [A.LAW_COLOYUK, A.LAW_COLOYUK]], "spline": [[A.SPLINE_PLUMMER] * 2] * 2}


def _case(pkg, lib, name, eps, mu=MU, box=None, with_psi=False, G=2.0, theta=1e-6, **kw):
    """(cfg, model, engine arguments) of a named wiring with its entries"""
    lib.mdl_set(mu, box if box else 1.0)
    M = U.models(mu, box if with_psi else None)
    pairs = [(a, b) for a in range(2) for b in range(2)]
    if name == "newton":
        wiring, model = "newton", {p: M["newton"] for p in pairs}
    elif name == "cross":
        wiring, model = _cross(pkg), {(a, b): M["newton" if a == b else "neg_newton"] for a, b in pairs}
    elif name == "yukawa_offdiag":
        wiring, model = "yukawa_offdiag", {(0, 1): M["yukawa"], (1, 0): M["yukawa"]}
    elif name == "coloyuk":
        wiring, model = "coloyuk", {p: M["coloyuk"] for p in pairs}
    elif name == "mixed":
        wiring, model = _mixed(pkg), {p: M["coloyuk"] for p in pairs[1:]}
    else:
        raise ValueError(name)
    cfg = pkg.make_config(n_gravs=2, G=G, theta=theta, softening=eps, type_to_grav=T2G, wiring=wiring, walk_mode=pkg.WALK_STRICT,
                          periodic=int(box is not None), box_size=box or 0.0, yukawa_imass=mu * (box or 1.0), **kw)
    return cfg, model, entries(pkg, lib, model, with_psi)


def _load(eng, pos, mass, typ, old_acc=None):
    eng.set_particles(pos, mass, typ, old_acc=old_acc)
    eng.domain_Decomposition()
    eng.force_treebuild()


def _status(pkg, cfg, pots, fns=None):
    """(status, message, handle left in *out) of a creation"""
    A = pkg.abi
    arr, nfns, keep = A.user_registry(fns)
    parr, npot, pkeep = A.potential_registry(pots)
    h = C.c_void_p(0x5a5a)                     # a poison the refusals must replace by NULL and nothing else
    rc = pkg.lib().ngravs_create_with_potentials(C.byref(cfg), arr, nfns, None, 0, parr, npot, C.byref(h))
    msg = pkg.lib().ngravs_last_error(None)
    if rc == 0:
        pkg.lib().ngravs_destroy(h)
    del keep, pkeep
    return rc, (msg.decode() if msg else ""), h.value


# ---- CPU -------------------------------------------------------------------------------------------------------------------------
def test_export_header_and_tables_of_the_models_potentials(pkg, have_lib, mdl):
    nm = subprocess.run(["nm", "-D", "--defined-only", pkg.LIB_PATH], capture_output=True, text=True, check=True).stdout
    for sym in ("ngravs_create_with_potentials", "ngravs_create_with_lattice", "ngravs_user_table_eval"):
        assert (" T " + sym) in nm, sym
    assert "ngravs_create_with_potentials" in pkg.EXPORTS
    src = ('#include "ngravs_hip.h"\n'
           'typedef double (*gravity)(double, double, double, double, long);\n'
           'typedef double (*latpot)(double *);\n'
           'static double p(double a, double b, double h, double r, long N) { (void)a; (void)h; (void)N; return b / r; }\n'
           'static double psi(double *x) { return x[0]; }\n'
           'int main(void) { gravity g = p; latpot l = psi; ngravs_user_potential_t e = {0, 1, g, g, l, 2.8372975}; ngravs_ctx *c = 0;\n'
           '  return ngravs_create_with_potentials(0, 0, 0, 0, 0, &e, 1, &c) + (NGRAVS_USER_POT == 4) + (NGRAVS_USER_POT_SPLINE == 5)\n'
           '         + (NGRAVS_USER_NORMED == 3); }\n')
    r = subprocess.run(["gcc", "-std=c99", "-Wall", "-Wextra", "-Werror", "-fsyntax-only", "-I", os.path.join(ROOT, "include"),
                        "-x", "c", "-"], input=src, capture_output=True, text=True)
    assert r.returncode == 0, r.stderr
    # the tables against the model's own functions: 10 000 radii over four decades, 10 000 u in [0, 1) for two lengths
    A = pkg.abi
    mu = 3.0
    mdl.mdl_set(mu, 1.0)
    M = U.models(mu)
    rng = np.random.default_rng(5)
    r_lo, r_hi = 1e-3, 10.0
    radii = np.exp(rng.uniform(np.log(r_lo), np.log(r_hi), 10000))
    for name in ("newton", "yukawa"):
        e = M[name]
        got, err = pkg.user_table_eval(A.USER_POT, law(pkg, mdl, e.names[0]), radii, r_lo=r_lo, r_hi=r_hi)
        want = e.pot(1.0, 0.0, radii)
        dev = np.abs(got / want - 1).max()
        print("%s pot: max relative deviation %.2e, fit %.2e" % (name, dev, err))
        assert dev <= 1e-9 and err <= 1e-9
        for h in (0.0056, 0.0224):
            u = rng.uniform(0, 1, 10000)
            got, err = pkg.user_table_eval(A.USER_POT_SPLINE, law(pkg, mdl, e.names[1]), u * h, h=h)
            want = e.spline(1.0, h, u * h)
            dev = np.abs(got / want - 1).max()
            print("%s pot_spline, h = %g: max relative deviation %.2e, fit %.2e" % (name, h, dev, err))
            assert dev <= 1e-9 and err <= 1e-9
    # the numpy restatements are the model's functions
    for name, e in M.items():
        f, s = law(pkg, mdl, e.names[0]), law(pkg, mdl, e.names[1])
        for r in (0.01, 0.3, 2.5):
            assert abs(f(3.0, 1.0, 0.1, r, 1) / float(e.pot(1.0, 0.1, np.float64(r))) - 1) <= 1e-14, name
        for u in (0.0, 0.3, 0.7):
            assert abs(s(3.0, 1.0, 0.02, u * 0.02, 1) / float(e.spline(1.0, 0.02, np.float64(u * 0.02))) - 1) <= 1e-14, name
    # the two kinds do not travel in a registry
    cfg = pkg.make_config(n_gravs=1, softening=[0.01] * 6)
    for kind in (A.USER_POT, A.USER_POT_SPLINE):
        rc, msg, h = _status(pkg, cfg, None, fns=[(kind, law(pkg, mdl, "mdl_newton_pot"))])
        assert rc == -1 and h is None and "kind" in msg, (rc, msg)


def test_refusals_need_no_gpu(pkg, have_lib, mdl):
    A = pkg.abi
    mdl.mdl_set(MU, BOX)
    f = lambda name: law(pkg, mdl, name)                       # noqa: E731
    nw, pl = f("mdl_newton_pot"), f("mdl_plummer_pot")
    ew = latpot(pkg, mdl, "mdl_ewald_psi")
    eps = [0.01] * 6
    open_cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, wiring="newton")
    per_cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, wiring="newton", periodic=1, box_size=BOX)
    pm_cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, wiring="newton", periodic=1, box_size=BOX, pmgrid=16)
    none_cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, wiring="yukawa_offdiag")
    full = [(a, b, nw, pl, None, 2.8372975) for a in range(2) for b in range(2)]
    full_per = [(a, b, nw, pl, ew, 2.8372975) for a in range(2) for b in range(2)]

    def swap(lst, k, **kw):
        e = dict(zip(("t", "s", "pot", "spl", "lat", "zero"), lst[k]))
        e.update(kw)
        return lst[:k] + [(e["t"], e["s"], e["pot"], e["spl"], e["lat"], e["zero"])] + lst[k + 1:]

    cases = [
        (open_cfg, swap(full, 3, t=2), "out of range"),
        (open_cfg, swap(full, 3, s=-1), "out of range"),
        (open_cfg, full + [full[2]], "second entry"),
        (none_cfg, full, "NONE"),
        (open_cfg, swap(full, 0, pot=None), "no pot or no pot_spline"),
        (open_cfg, swap(full, 0, spl=None), "no pot or no pot_spline"),
        (open_cfg, swap(full, 1, pot=f("mdl_twice_pot")), "third law"),
        (open_cfg, swap(full, 1, spl=f("mdl_twice_spline")), "third law"),
        (per_cfg, swap(full_per, 1, lat=latpot(pkg, mdl, "mdl_other_psi")), "lattice_pot or lattice_zero differs"),
        (per_cfg, swap(full_per, 1, zero=1.0), "lattice_pot or lattice_zero differs"),
        (open_cfg, swap(full, 0, pot=f("mdl_quadratic_pot")), "linear in the source mass"),
        (open_cfg, swap(full, 0, pot=f("mdl_target_pot")), "linear in the source mass"),
        (open_cfg, swap(full, 0, pot=f("mdl_count_pot")), "linear in the source mass"),
        (open_cfg, swap(full, 0, spl=f("mdl_count_spline")), "linear in the source mass"),
        (open_cfg, swap(full, 0, pot=f("mdl_soft_pot")), "depends on its softening argument"),
        (per_cfg, swap(full_per, 3, lat=None), "needs the pair's lattice_pot"),
        (open_cfg, swap(full, 3, lat=ew), "non-periodic"),
        (open_cfg, full[:2] + full[3:], "mirrored pair"),
    ]
    for cfg, pots, word in cases:
        rc, msg, h = _status(pkg, cfg, pots)
        assert rc == WIRING and word in msg and h is None, (word, rc, msg, h)
    # accepted without a device only as far as the checks go: with a mesh lattice_pot is optional
    rc, msg, h = _status(pkg, pm_cfg, full)
    assert rc in (0, -2), (rc, msg)            # 0 with a GPU, NGRAVS_ERR_NO_DEVICE without: the checks passed
    # Engine() carries the entries and the message
    with pytest.raises(pkg.NgravsError, match="status -6") as e:
        pkg.Engine(open_cfg, user_potentials=full + [full[0]])
    assert "second entry" in str(e.value)


def test_the_models_yukawa_lattice_potential_against_a_wider_image_sum(pkg, mdl):
    """three points of the octant: the model's sum to |n_i| <= 6 against numpy's to |n_i| <= 10; what lies beyond 6 is below
    (21^3 - 13^3) exp(-6 x 6.5) / 6.5 = 1e-14"""
    mdl.mdl_set(MU / BOX, BOX)
    psi = latpot(pkg, mdl, "mdl_yuk_psi")
    for x in ([0.3, 0.1, 0.2], [0.5, 0.5, 0.5], [0.05, 0.4, 0.0]):
        got = psi((C.c_double * 3)(*x))
        want = float(U.yuk_psi(np.array(x), MU, nmax=10))
        print(x, got, want, got - want)
        assert abs(got - want) <= 1e-13 * max(1.0, abs(want))
    ew = latpot(pkg, mdl, "mdl_ewald_psi")
    for x in ([0.3, 0.1, 0.2], [0.5, 0.5, 0.5]):
        assert abs(ew((C.c_double * 3)(*x)) - float(R.ewald_psi(np.array(x)))) <= 1e-13


def test_planted_pairs_land_in_their_branches(pkg):
    for n in SIZES:
        for box in (None, BOX):
            pos, mass, typ, eps = U.particle_set(n, 100 + n, box)
            cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, periodic=int(box is not None), box_size=box or 0.0)
            fs = np.array(cfg.force_softening[:])
            assert len(set(fs[typ])) >= min(n, 2)
            if n >= 2:
                assert np.all(pos[0] == pos[1])
            if n < 63:
                continue
            _, r = R.separations(cfg, pos, pos)
            species = R.species(cfg, typ)
            seen = set()
            for a, b, ta, tb, frac in U.PLANTED:
                h = max(fs[typ[a]], fs[typ[b]])
                u = r[a, b] / h
                assert (typ[a], typ[b]) == (ta, tb) and abs(u - frac) < 1e-9 and (u < 0.5) == (frac < 0.5) and r[a, b] < h
                seen.add((species[a] == species[b], frac))
            assert seen == {(False, 0.3), (True, 0.7), (False, 0.7), (True, 0.3)}


# ---- GPU: 1. user copies of the Newton and Plummer potentials -----------------------------------------------------------------------
def _bound(G, terms, self_t, look=None):
    """(1e-9 + 1e-12) G sum_j |term_ij| per row.  The row's own term is one of them; where the row's own pair is wired NONE it is
    0, and the tail's built-in self term 2.8 m / h, which then cancels nothing, takes its place in the sum."""
    s = np.abs(terms).sum(1) + np.where(np.diag(terms) == 0, np.abs(self_t), 0.0)
    return FIT * G * (s if look is None else s + np.abs(look).sum(1))


def _ratio(tag, got, want, bound):
    ratio = (np.abs(got - want) / bound).max()
    print("%s: max deviation / bound = %.3e" % (tag, ratio))
    return ratio


@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["newton", "cross"])
@pytest.mark.parametrize("n", SIZES)
def test_user_newton_copies_are_the_builtin_potentials(pkg, mdl, n, wiring):
    pos, mass, typ, eps = U.particle_set(n, 100 + n)
    cfg, model, pots = _case(pkg, mdl, wiring, eps)
    eng_u, eng_b = pkg.Engine(cfg, user_potentials=pots), pkg.Engine(cfg)
    terms = U.pair_terms(cfg, model, pos, mass, typ)
    want = U.tail(cfg, model, None, pos, mass, typ, terms.sum(1))
    bound = FIT * cfg.G * np.abs(terms).sum(1)
    for theta in (1e-6, 0.5):
        out = []
        for eng in (eng_u, eng_b):
            eng.set_opening(theta, 0.005)
            _load(eng, pos, mass, typ)
            out.append(eng.compute_potential(want_nint=True))
        (pot_u, ni_u), (pot_b, ni_b) = out
        assert np.array_equal(ni_u, ni_b), theta
        assert _ratio("n = %d %s theta = %g: user copies against the built-in column" % (n, wiring, theta), pot_u, pot_b, bound) <= 1
        if theta < 0.1:
            assert _ratio("n = %d %s: user copies against the pair sum" % (n, wiring), pot_u, want, bound) <= 1
        elif n > 64:
            assert ni_u.max() < n              # nodes were used
    eng_u.close()
    eng_b.close()


# ---- 2. Yukawa companions, open, tree-only ----------------------------------------------------------------------------------------
def _self_values(pkg, cfg, pots):
    """pot_spline[g][g](1, 1, h_type, 0, 1) as the device reads it from its table, per type: the walk of a lone particle of mass 1"""
    v = np.zeros(6)
    for t in range(6):
        e = pkg.Engine(cfg, user_potentials=pots)
        p, m, ty = np.full((1, 3), 0.5), np.ones(1), np.array([t], dtype=np.int32)
        _load(e, p, m, ty)
        v[t] = e.potential_targets(p, ty, mass=m)[0] / cfg.G
        e.close()
    return v


@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["yukawa_offdiag", "coloyuk", "mixed"])
@pytest.mark.parametrize("n", SIZES)
def test_yukawa_companions_are_the_pair_sum(pkg, mdl, n, wiring):
    pos, mass, typ, eps = U.particle_set(n, 200 + n)
    cfg, model, pots = _case(pkg, mdl, wiring, eps)
    eng = pkg.Engine(cfg, user_potentials=pots)
    _load(eng, pos, mass, typ)
    pot, ni = eng.compute_potential(want_nint=True)
    terms = U.pair_terms(cfg, model, pos, mass, typ)
    want = U.tail(cfg, model, None, pos, mass, typ, terms.sum(1))
    bound = _bound(cfg.G, terms, U.self_term(cfg, model, mass, typ))
    assert _ratio("n = %d %s: Yukawa companions against the pair sum" % (n, wiring), pot, want, bound) <= 1
    if n == 1 and wiring == "coloyuk":
        h = cfg.force_softening[typ[0]]
        ulp4 = 4 * np.spacing(cfg.G * mass[0] * abs(float(model[0, 0].spline(1.0, h, np.float64(0.0)))))
        print("one particle: pot = %.3e, 4 ulp = %.3e" % (pot[0], ulp4))
        assert abs(pot[0]) <= ulp4
    if n == 1037:
        # own rows as targets, self term in numpy in the device's order of operations: compute_potential bit for bit
        own, ni_own = eng.potential_targets(pos, typ, mass=mass, want_nint=True)
        assert np.array_equal(ni, ni_own)
        v = _self_values(pkg, cfg, pots)
        fs = np.array(cfg.force_softening[:])[typ]
        has = np.array([(g, g) in model for g in R.species(cfg, typ)])
        assert np.array_equal(np.where(has, (own / cfg.G - mass * v[typ]) * cfg.G, (own / cfg.G + mass * (1.0 / fs) * 2.8) * cfg.G), pot)
    eng.close()


# ---- 3. periodic tree-only --------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("wiring", ["yukawa_offdiag", "newton"])
@pytest.mark.parametrize("n", [65, 1037])
def test_periodic_tree_only_lattice_potentials(pkg, mdl, n, wiring):
    pos, mass, typ, eps = U.particle_set(n, 300 + n, box=BOX)
    cfg, model, pots = _case(pkg, mdl, wiring, eps, mu=MU / BOX, box=BOX, with_psi=True)
    eng = pkg.Engine(cfg, user_potentials=pots)
    _load(eng, pos, mass, typ)
    # the tables at 4096 points and the origin
    rng = np.random.default_rng(9)
    idx = np.vstack([np.zeros((1, 3), dtype=np.int64), rng.integers(0, 65, (4096, 3))])
    idx = idx[(idx.sum(1) > 0) | (np.arange(len(idx)) == 0)]
    tabs = {}
    for (a, b), e in model.items():
        tabs[a, b] = t = eng.lattice_potential_table(a, b)
        ref = e.psi(0.5 * idx / 64.0) / BOX
        ref[0] = e.zero / BOX
        got = t[idx[:, 0], idx[:, 1], idx[:, 2]]
        err = np.abs(got - ref).max() / np.abs(ref).max()
        print("%s lattice table [%d][%d]: max err %.2e of max|table|" % (wiring, a, b, err))
        assert err <= 1e-10 and got[0] == e.zero / BOX
    if wiring == "newton":
        eng_b = pkg.Engine(cfg)
        for a, b in model:
            tb = eng_b.lattice_potential_table(a, b)
            err = np.abs(tabs[a, b] - tb).max() / np.abs(tb).max()
            print("newton lattice table [%d][%d] against the built-in engine's: %.2e" % (a, b, err))
            assert err <= 1e-10
        eng_b.close()
    # everything opened: the pair sum plus the lookup in that same table
    terms = U.pair_terms(cfg, model, pos, mass, typ)
    look = U.lookup_terms(cfg, tabs, pos, mass, typ)
    bound = _bound(cfg.G, terms, U.self_term(cfg, model, mass, typ), look)
    want = U.tail(cfg, model, None, pos, mass, typ, (terms + look).sum(1))
    pot = eng.compute_potential()
    assert _ratio("n = %d %s: periodic column against pair sum + lookup" % (n, wiring), pot, want, bound) <= 1
    # against exact image sums
    rows = np.arange(n) if n <= 65 else np.arange(32)
    exact = (terms[rows] + U.image_terms(cfg, model, pos, mass, typ, rows)).sum(1)
    exact = U.tail(cfg, model, None, pos[rows], mass[rows], typ[rows], exact)
    dev_gpu, dev_ref = np.abs(pot[rows] - exact).max(), np.abs(want[rows] - exact).max()
    print("n = %d %s: deviation from exact image sums: device %.3e, restatement %.3e (max |pot| %.3e)" %
          (n, wiring, dev_gpu, dev_ref, np.abs(exact).max()))
    assert dev_gpu <= 1.5 * dev_ref
    eng.close()


@pytest.mark.gpu
def test_a_non_finite_lattice_sample_names_the_pair_and_the_point(pkg, mdl):
    n = 65
    pos, mass, typ, eps = U.particle_set(n, 301, box=BOX)
    cfg, model, _ = _case(pkg, mdl, "newton", eps, mu=MU / BOX, box=BOX, with_psi=True)
    model[1, 1] = model[1, 1]._replace(names=model[1, 1].names[:2] + ("mdl_nan_psi",))
    eng = pkg.Engine(cfg, user_potentials=entries(pkg, mdl, model, with_psi=True))
    _load(eng, pos, mass, typ)
    out = np.full(n, -3.25)
    with pytest.raises(pkg.NgravsError, match="status -6") as e:
        eng.compute_potential(into=out)
    assert "[1][1]" in str(e.value) and "(3, 4, 5)" in str(e.value), str(e.value)
    assert np.all(out == -3.25)
    eng.close()


# ---- 4. TreePM --------------------------------------------------------------------------------------------------------------------
def _treepm(pkg, lib, eps, user):
    """[0][0] Newton with its built-in companion, the other pairs coloyuk: as user force laws with their Green's functions and
    potential entries, or built in (the restatement of the mesh and of the long-range table take the built-in ids)"""
    import math
    A = pkg.abi
    grid, mu = 16, MU / BOX
    lib.mdl_set(mu, BOX)
    asmth = 1.25 * BOX / grid
    ym2 = (MU / (2 * math.pi)) ** 2
    yfac = math.exp(-ym2 * (2 * math.pi * asmth / BOX) ** 2)
    ymn = 4 * math.pi * asmth * (MU / (2 * math.pi)) / BOX

    def coloyuk(t, s, r2, r, n):
        return s * math.exp(-r * mu) * (mu / r + 1.0 / r2) + s / r2

    def pgcoloyuk(t, s, k2, k, n):
        return 1.0 / k2 + yfac / (k2 + ym2)

    def normed_pgcoloyuk(t, s, k2, k, n):
        return k2 / (k2 + ymn * ymn) * math.exp(-ymn * ymn * 0.25) + 1.0
    U0 = A.LAW_USER0
    diag = lambda i, j: i == j == 0  # noqa: E731
    ids = (U0, U0 + 1, U0 + 2) if user else (A.LAW_COLOYUK,) * 3
    w = {"accel": [[1 if diag(i, j) else ids[0] for j in range(2)] for i in range(2)], "spline": [[1, 1], [1, 1]],
         "greens": [[1 if diag(i, j) else ids[1] for j in range(2)] for i in range(2)],
         "normed": [[1 if diag(i, j) else ids[2] for j in range(2)] for i in range(2)]}
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=grid, box_size=BOX, G=2.0, theta=1e-6, softening=eps, type_to_grav=T2G, wiring=w,
                          walk_mode=pkg.WALK_STRICT, yukawa_imass=MU)
    fns = [(A.USER_ACCEL, coloyuk), (A.USER_GREENS, pgcoloyuk), (A.USER_NORMED, normed_pgcoloyuk)] if user else None
    M = U.models(mu)
    model = {(0, 1): M["coloyuk"], (1, 0): M["coloyuk"], (1, 1): M["coloyuk"]}
    return cfg, fns, model, entries(pkg, lib, model)


@pytest.mark.gpu
@pytest.mark.parametrize("n", [65, 1037])
def test_treepm_short_range_mesh_and_total(pkg, mdl, n):
    pos, mass, typ, eps = U.particle_set(n, 400 + n, box=BOX)
    cfg, fns, model, pots = _treepm(pkg, mdl, eps, user=True)
    cfg_b = _treepm(pkg, mdl, eps, user=False)[0]
    eng = pkg.Engine(cfg, user_fns=fns, user_potentials=pots)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=True)
    before = eng.get_accel(want_pm=True)
    pot = eng.compute_potential()
    for a, b in zip(before, eng.get_accel(want_pm=True)):
        assert np.array_equal(a, b)                            # GravAccel, OldAcc, GravCost, GravPM: bit-equal
    force, ptab = pkg.shortrange_table_with_laws(cfg, fns)
    E = (np.asarray(force) + np.asarray(ptab)) * (3.0 / R.NTAB * (np.arange(R.NTAB) + 0.5))
    assert np.abs(E - R.e_table(pkg, cfg_b)).max() <= 1e-12 * np.abs(E).max()
    terms = U.pair_terms(cfg, model, pos, mass, typ, table=E)
    mesh = R.mesh_potential(cfg_b, pos, mass, typ)
    self_t = U.self_term(cfg, model, mass, typ)
    short = (pot - mesh) / cfg.G - self_t
    bound = _bound(1.0, terms, self_t)
    assert _ratio("n = %d: TreePM short-range walk against the cut pair sum" % n, short, terms.sum(1), bound) <= 1
    want = U.tail(cfg, model, None, pos, mass, typ, terms.sum(1), mesh)
    assert _ratio("n = %d: TreePM total against walk + mesh" % n, pot, want, cfg.G * bound + 1e-10 * np.abs(want).max()) <= 1
    # the mesh part alone: a clump in [0, 0.3 L]^3, probes around 0.65 L -- farther than 6 Asmth from every particle
    rng = np.random.default_rng(41)
    cpos = rng.uniform(0, 0.3 * BOX, (n, 3))
    _load(eng, cpos, mass, typ)
    eng.compute_potential()
    probes = 0.65 * BOX + rng.uniform(-0.02, 0.02, (65, 3)) * BOX
    ptyp = (np.arange(65) % 6).astype(np.int32)
    p, ni = eng.potential_targets(probes, ptyp, want_nint=True)
    wmesh = R.mesh_potential(cfg_b, cpos, mass, typ, probes, ptyp)
    assert np.all(ni == 0)
    err = np.abs(p - wmesh).max() / np.abs(wmesh).max()
    print("n = %d: mesh part max err %.2e of max|pot|" % (n, err))
    assert err <= 1e-10
    eng.close()


# ---- 5. split additivity ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_a_set_split_over_two_engines_adds_up(pkg, mdl):
    n = 1037
    pos, mass, typ, eps = U.particle_set(n, 51)
    cfg, model, pots = _case(pkg, mdl, "coloyuk", eps)
    total = np.zeros(n)
    for sel in (np.arange(n) < 500, np.arange(n) >= 500):
        e = pkg.Engine(cfg, user_potentials=pots)
        _load(e, pos[sel], mass[sel], typ[sel])
        total += e.potential_targets(pos, typ, mass=mass)
        e.close()
    eng = pkg.Engine(cfg, user_potentials=pots)
    _load(eng, pos, mass, typ)
    single = eng.potential_targets(pos, typ, mass=mass)
    terms = U.pair_terms(cfg, model, pos, mass, typ)
    bound = FIT * cfg.G * np.abs(terms).sum(1)
    assert _ratio("split 500 / 537 against the single engine", total, single, bound) <= 1
    assert _ratio("split 500 / 537 against the pair sum", total, cfg.G * terms.sum(1), bound) <= 1
    eng.close()


# ---- 6. tail ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_tail_takes_the_entries_lattice_zero(pkg, mdl):
    n = 65
    pos, mass, typ, eps = U.particle_set(n, 61, box=BOX)
    cfg, model, _ = _case(pkg, mdl, "coloyuk", eps, mu=MU / BOX, box=BOX, G=1.0)
    Y = U.models(MU / BOX, BOX)["yukawa"]
    model = {p: e._replace(psi=Y.psi, zero=1.2345 + 0.5 * p[0] * p[1], names=e.names[:2] + ("mdl_yuk_psi",)) for p, e in model.items()}
    eng = pkg.Engine(cfg, user_potentials=entries(pkg, mdl, model, with_psi=True))
    _load(eng, pos, mass, typ)
    par = pkg.abi.make_time_params(comoving=1, omega0=0.3, omega_lambda=0.7, hubble=0.1)
    walk = eng.potential_targets(pos, typ, mass=mass) / cfg.G
    pot, plain = eng.compute_potential(par), eng.compute_potential()
    want, want_plain = U.tail(cfg, model, par, pos, mass, typ, walk), U.tail(cfg, model, None, pos, mass, typ, walk)
    # what the comoving tail adds is the LatticeZero term alone: to 1e-12 of the column.  The column itself carries the self
    # term, a table read, which the restatement takes from the function: FIT of it on top
    scale = np.abs(want).max()
    err = np.abs((pot - plain) - (want - want_plain)).max() / scale
    err_col = (np.abs(pot - want) - FIT * cfg.G * np.abs(U.self_term(cfg, model, mass, typ))).max() / scale
    print("comoving periodic: LatticeZero term max err %.2e, column beyond the self term's fit %.2e; the tail moves the column by %.2e of it"
          % (err, err_col, np.abs(pot - plain).max() / scale))
    assert err <= 1e-12 and err_col <= 1e-12
    assert np.abs(pot - plain).max() > 1e-6 * scale
    with_builtin_zero = want_plain - (want_plain - want) * 2.8372975 / 1.2345
    assert np.abs(pot - with_builtin_zero).max() > 1e-6 * scale                 # the entry's value, not 2.8372975
    eng.close()


# ---- 7. softening change ---------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_set_softening_rebuilds_the_spline_tables(pkg, mdl):
    n = 65
    pos, mass, typ, eps = U.particle_set(n, 71)
    cfg, model, pots = _case(pkg, mdl, "coloyuk", eps)
    eng = pkg.Engine(cfg, user_potentials=pots)
    _load(eng, pos, mass, typ)
    first = eng.compute_potential()
    eng.set_softening(np.array(cfg.force_softening[:]) * np.array([1.5, 0.7, 1.2, 0.9, 1.4, 0.8]))
    assert eng.cfg is cfg                                      # (the truth below reads the new lengths)
    _load(eng, pos, mass, typ)
    pot = eng.compute_potential()
    terms = U.pair_terms(cfg, model, pos, mass, typ)
    want = U.tail(cfg, model, None, pos, mass, typ, terms.sum(1))
    bound = _bound(cfg.G, terms, U.self_term(cfg, model, mass, typ))
    assert _ratio("after set_softening: column against the pair sum with the new lengths", pot, want, bound) <= 1
    assert (np.abs(first - want) / bound).max() > 1e3          # the old lengths' column is somewhere else
    eng.close()


# ---- 8. Timeline -----------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_timeline_takes_the_device_potential_of_a_yukawa_wiring(pkg, mdl, tmp_path):
    import torch
    import test_time_integration as T
    n = 65
    pos, mass, typ, eps = U.particle_set(n, 81)
    typ = np.where(typ == 0, 1, typ).astype(np.int32)          # no gas
    vel = np.random.default_rng(82).normal(size=(n, 3)) * 0.05
    cfg, model, pots = _case(pkg, mdl, "coloyuk", eps, G=2.0 ** -27)       # every row takes max_size_timestep
    eng = pkg.Engine(cfg, user_potentials=pots)
    P = T.params(False, time_max=8.0, timebase_interval=8.0 / T.TB, max_size_timestep=0.25, min_size_timestep=0.0)
    host = dict(type=typ, pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    cols = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    ids = torch.arange(n, dtype=torch.int32, device="cuda")
    seen = []

    def on_station(name, tl):
        if name == "statistics":
            seen.append(tl.cols["pos"].cpu().numpy().copy())
    out = dict(dir=str(tmp_path) + os.sep, base="snap", snap_format=2, rule=pkg.abi.make_output_rule(time_of_first_snapshot=0.3, time_bet_snapshot=0.6),
               blocks_mask=pkg.abi.snap_mask("POT"), ids=lambda tl: ids)
    par = T.c_params(pkg, P)
    tl = pkg.timeline.Timeline(eng, cols, par, on_station=on_station, time_bet_statistics=0, potential="device", output=out)
    states = []
    for _ in range(2):
        tl.step()
        states.append(tl.sys_state.EnergyPot)
    assert len(seen) == 2
    for p_at, e_pot in zip(seen, states):
        terms = U.pair_terms(cfg, model, p_at, mass, typ)
        want = U.tail(cfg, model, par, p_at, mass, typ, terms.sum(1))
        # (the fit's share, and the rounding of the energy sum as test_potential.py bounds it, cosmological term included)
        bound = (0.5 * mass * _bound(cfg.G, terms, U.self_term(cfg, model, mass, typ))).sum() + 1e-12 * np.abs(0.5 * mass * want).sum()
        print("EnergyPot: deviation / bound = %.3e" % (abs(e_pot - (0.5 * mass * want).sum()) / bound))
        assert abs(e_pot - (0.5 * mass * want).sum()) <= bound
    path = tl.write_snapshot()
    _, blocks = pkg.snapshot.read_blocks(path)
    order = np.argsort(typ, kind="stable")
    got = np.asarray(blocks["POT"]).ravel()
    assert got.dtype == np.float32
    assert np.array_equal(got, tl.potential_column.cpu().numpy()[order].astype(np.float32))
    eng.close()


# ---- 9. still refused ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
def test_still_refused_with_entries(pkg, mdl):
    n = 65
    pos, mass, typ, eps = U.particle_set(n, 91)
    mdl.mdl_set(MU, 1.0)
    M = U.models(MU)
    full = entries(pkg, mdl, {(a, b): M["newton"] for a in range(2) for b in range(2)})

    def refused(eng, word, status="status -1"):
        out = np.full(n, -3.25)
        with pytest.raises(pkg.NgravsError, match=status) as e:
            eng.compute_potential(into=out)
        assert word in str(e.value), (word, str(e.value))
        with pytest.raises(pkg.NgravsError, match=status) as e:
            eng.potential_targets(pos[:5], typ[:5])
        assert word in str(e.value), (word, str(e.value))
        assert np.all(out == -3.25)

    for kw, word in ((dict(wiring="bam"), "BAM"), (dict(wiring="newton", world_size=2), "single task only")):
        cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.5, softening=eps, type_to_grav=T2G, walk_mode=pkg.WALK_STRICT, **kw)
        eng = pkg.Engine(cfg, user_potentials=full)
        eng.set_particles(pos, mass, typ)
        refused(eng, word)
        eng.close()
    cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.5, softening=eps, type_to_grav=T2G, walk_mode=pkg.WALK_STRICT)
    eng = pkg.Engine(cfg, user_potentials=full)
    _load(eng, pos, mass, typ)
    eng.set_gas_softening(np.where(typ == 0, 0.05, 0.0))
    refused(eng, "adaptive gas softening")
    eng.set_gas_softening(None)
    assert np.all(np.isfinite(eng.compute_potential()))
    eng.close()
    # a pair without a companion next to pairs with entries: the first such pair is named, as before
    cfg = pkg.make_config(n_gravs=2, G=1.0, theta=0.5, softening=eps, type_to_grav=T2G, walk_mode=pkg.WALK_STRICT, wiring="coloyuk")
    eng = pkg.Engine(cfg, user_potentials=[e for e in full if (e[0], e[1]) != (1, 1)])
    _load(eng, pos, mass, typ)
    refused(eng, "law_accel[1][1] has no wired potential companion")
    eng.close()
    # a periodic tree-only wiring whose entries lack lattice_pot does not get as far as a context
    cfg = pkg.make_config(n_gravs=2, softening=eps, type_to_grav=T2G, periodic=1, box_size=BOX)
    with pytest.raises(pkg.NgravsError, match="status -6") as e:
        pkg.Engine(cfg, user_potentials=full)
    assert "lattice_pot" in str(e.value)
