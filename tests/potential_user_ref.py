"""CPU truth for the potentials of a model's own functions (ngravs_create_with_potentials): tests/user_potential/model.c restated
in numpy, pair sums over these functions in the manner of potential_ref.pair_terms, the tail with the entries' self term and
LatticeZero, image sums for the periodic cases and the particle sets with their planted pairs.  potential_ref.py supplies what
does not depend on the law (separations, the trilinear lookup, the mesh, the built-in companions).

A `model` maps a species pair (target, source) to an Entry; a pair that is missing has the built-in companions of its wiring.
"""
import collections

import numpy as np

import potential_ref as R

Entry = collections.namedtuple("Entry", "pot spline psi zero names")   # names: the model.c symbols (pot, spline, psi or None)


# ---- tests/user_potential/model.c in numpy: f(source mass, h, r) ----------------------------------------------------------------
def newton_pot(s, h, r):
    with np.errstate(divide="ignore", invalid="ignore"):
        return s / r


def neg_newton_pot(s, h, r):
    return -newton_pot(s, h, r)


def plummer_pot(s, h, r):
    return R.plummer_pot(s, h, r)


def neg_plummer_pot(s, h, r):
    return -R.plummer_pot(s, h, r)


def yuk_pot(mu):
    def f(s, h, r):
        with np.errstate(divide="ignore", invalid="ignore"):
            return s * np.exp(-mu * r) / r
    return f


def yuk_spline(mu):
    def f(s, h, r):
        u = r / h
        return -s / h * (2.8 - 1.7 * u * u + 0.4 * u * u * u * u * u) * np.exp(-mu * r)
    return f


def coloyuk_pot(mu):
    return lambda s, h, r: newton_pot(s, h, r) + yuk_pot(mu)(s, h, r)


def coloyuk_spline(mu):
    return lambda s, h, r: plummer_pot(s, h, r) + yuk_spline(mu)(s, h, r)


def yuk_psi(x, mu_box, nmax=6):
    """exp(-mu |x|) / |x| - sum_{|n_i| <= nmax} exp(-mu |x - n|) / |x - n| at x[..., 3] in box units: minus the images n != 0"""
    x = np.asarray(x, dtype=np.float64)
    out = np.zeros(x.shape[:-1])
    g = np.arange(-nmax, nmax + 1, dtype=np.float64)
    for n0 in g:
        for n1 in g:
            d01 = (x[..., 0] - n0) ** 2 + (x[..., 1] - n1) ** 2
            for n2 in g:
                if n0 == 0 and n1 == 0 and n2 == 0:
                    continue                      # (the model adds and subtracts this term)
                r = np.sqrt(d01 + (x[..., 2] - n2) ** 2)
                out -= np.exp(-mu_box * r) / r
    return out


def yuk_zero(mu_box, nmax=6):
    """the value at the origin, LatticeZero of the Yukawa pairs: minus the sum over the images n != 0"""
    return float(yuk_psi(np.zeros(3), mu_box, nmax))


def models(mu, box=None):
    """the entries the tests wire, by name"""
    mb = mu * box if box else 0.0
    ypsi = (lambda x: yuk_psi(x, mb)) if box else None
    return {
        "newton": Entry(newton_pot, plummer_pot, R.ewald_psi if box else None, R.LATTICE_ZERO, ("mdl_newton_pot", "mdl_plummer_pot", "mdl_ewald_psi")),
        "neg_newton": Entry(neg_newton_pot, neg_plummer_pot, None, -R.LATTICE_ZERO, ("mdl_neg_newton_pot", "mdl_neg_plummer_pot", None)),
        "yukawa": Entry(yuk_pot(mu), yuk_spline(mu), ypsi, yuk_zero(mb) if box else 0.0, ("mdl_yuk_pot", "mdl_yuk_spline", "mdl_yuk_psi")),
        "coloyuk": Entry(coloyuk_pot(mu), coloyuk_spline(mu), None, 0.0, ("mdl_coloyuk_pot", "mdl_coloyuk_spline", None)),
    }


# ---- pair sums --------------------------------------------------------------------------------------------------------------------
def pair_terms(cfg, model, pos, mass, typ, tpos=None, ttyp=None, table=None):
    """terms[t, s] of the everything-opened walk, without G: potential_ref.pair_terms with the model's functions at unit masses,
    scaled by the source mass, on the pairs that have an entry"""
    out = R.pair_terms(cfg, pos, mass, typ, tpos, ttyp, table=None)
    tpos = pos if tpos is None else tpos
    ttyp = typ if ttyp is None else ttyp
    mass = np.asarray(mass, dtype=np.float64)
    fs = np.array([cfg.force_softening[t] for t in range(6)])
    h = np.maximum(fs[np.asarray(ttyp)][:, None], fs[np.asarray(typ)][None, :]) + 0.0 * mass[None, :]
    tg, sg = R.species(cfg, ttyp), R.species(cfg, typ)
    d, r = R.separations(cfg, tpos, pos)
    m = mass[None, :] + 0.0 * r
    for (a, b), e in model.items():
        sel = (tg[:, None] == a) & (sg[None, :] == b)
        far = sel & (r >= h)
        near = sel & (r < h)
        out[far] = -m[far] * e.pot(1.0, h[far], r[far])
        out[near] = m[near] * e.spline(1.0, h[near], r[near])
    if table is not None:
        asmth = float(cfg.asmth) if cfg.asmth > 0 else R.pm_reference.ASMTH * float(cfg.box_size) / int(cfg.pmgrid)
        asmthfac = 0.5 / asmth * (R.NTAB / 3.0)
        tab = (asmthfac * r).astype(np.int64)
        lr = m / (2 * np.pi * asmth) * table[tg[:, None], sg[None, :], np.minimum(tab, R.NTAB - 1)]
        out = np.where(tab < R.NTAB, out + lr, 0.0)
    return out


def self_term(cfg, model, mass, typ):
    """what the tail adds for the row itself: - m pot_spline[g][g](1, 1, h, 0, 1) with an entry, the built-in 2.8 m / h without"""
    mass = np.asarray(mass, dtype=np.float64)
    fs = np.array([cfg.force_softening[t] for t in range(6)])[np.asarray(typ)]
    g = R.species(cfg, typ)
    out = 2.8 * mass / fs
    for (a, b), e in model.items():
        if a == b:
            sel = g == a
            out[sel] = -mass[sel] * e.spline(1.0, fs[sel], np.zeros(sel.sum()))
    return out


def tail(cfg, model, par, pos, mass, typ, walk, mesh=None):
    """potential_ref.tail with the entries' self term and LatticeZero"""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    pot = walk + self_term(cfg, model, mass, typ)
    comoving = par is not None and par.comoving
    if comoving and cfg.periodic:
        g = R.species(cfg, typ)
        lz = np.array([model[k, k].zero if (k, k) in model else R.law_sign(cfg.law_accel[k][k]) * R.LATTICE_ZERO
                       for k in range(int(cfg.n_gravs))])[g]
        pot = pot - lz * mass ** (2.0 / 3) * (par.omega0 * 3 * par.hubble * par.hubble / (8 * np.pi * float(cfg.G))) ** (1.0 / 3)
    pot = pot * float(cfg.G)
    if mesh is not None:
        pot = pot + mesh
    r2 = (pos ** 2).sum(1)
    if comoving:
        if not cfg.periodic:
            pot = pot + (-0.5 * par.omega0 * par.hubble * par.hubble) * r2
    elif par is not None and par.omega_lambda * par.hubble != 0:
        pot = pot + (-0.5 * par.omega_lambda * par.hubble * par.hubble) * r2
    return pot


def lookup_terms(cfg, tables, pos, mass, typ):
    """look[t, s] = m_s x the trilinear lookup in the pair's octant table (tables[a, b]: [65, 65, 65])"""
    g = R.species(cfg, typ)
    d, _ = R.separations(cfg, pos, pos)
    look = np.zeros((len(pos), len(pos)))
    for (a, b), t in tables.items():
        sel = (g[:, None] == a) & (g[None, :] == b)
        look[sel] = (np.asarray(mass)[None, :] * R.lat_lookup(t, 2.0 * 64 / float(cfg.box_size), d))[sel]
    return look


def image_terms(cfg, model, pos, mass, typ, rows):
    """img[k, s] = m_s psi(d / L) / L for the targets rows[k] with psi evaluated at every pair instead of looked up, the row's own
    images (LatticeZero) included"""
    L = float(cfg.box_size)
    g = R.species(cfg, typ)
    d, r = R.separations(cfg, pos[rows], pos)
    out = np.zeros(r.shape)
    for (a, b), e in model.items():
        sel = (g[rows][:, None] == a) & (g[None, :] == b)
        if not sel.any():
            continue
        with np.errstate(divide="ignore", invalid="ignore"):
            psi = e.psi(d[sel] / L)
        psi[r[sel] == 0] = e.zero
        out[sel] = psi
    return out * np.asarray(mass)[None, :] / L


# ---- particle sets ----------------------------------------------------------------------------------------------------------------
PLANTED = ((20, 21, 0, 1, 0.3), (22, 23, 2, 4, 0.7), (24, 25, 3, 0, 0.7), (26, 27, 5, 1, 0.3))   # (row, row, type, type, r / h)
T2G = [0, 1, 0, 1, 0, 1]


def particle_set(n, seed, box=None):
    """potential_ref.particle_set (six distinct softening lengths, two species, close pairs, the coincident pair 0 / 1) with four
    planted pairs from 63 particles on: 0.3 h and 0.7 h of the pair's h = 2.8 max(eps), across species (types 0 / 1, 3 / 0) and
    within one (types 2 / 4 -> species 0, types 5 / 1 -> species 1): both halves of a spline table, several lengths"""
    pos, mass, typ, eps = R.particle_set(n, seed, box)
    if n >= 63:
        rng = np.random.default_rng(seed + 1000)
        for a, b, ta, tb, frac in PLANTED:
            typ[a], typ[b] = ta, tb
            v = rng.normal(size=3)
            pos[b] = pos[a] + v / np.linalg.norm(v) * frac * 2.8 * max(eps[ta], eps[tb])
    return pos, mass, typ, eps
