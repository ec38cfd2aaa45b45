"""CPU restatement of the potential path (csrc/kernels_potential.hip) in plain numpy fp64: what the reference's potential routines
MEAN (DESIGN.md §8 lists why they themselves cannot be the truth).  Built-in Newton / neg-Newton with Plummer / neg-Plummer.

  pair_terms      the walk's term of every (target, source) pair with everything opened: h = max(h_target, h_source);
                  r >= h: -Pfn(m, r), r < h: +Pspl(m, h, r) (ngravs.c:368-489); periodic: nearest image
  ewald_psi       ngravs.c:761-816, summed in its order; psi_brute is a plain image sum that knows nothing of Ewald's split
  lat_lookup      lattice_pot_corr (forcetree.c:3895-3941): the trilinear lookup in an octant table
  e_table         E[i] = (force_tab[i] + pot_tab[i]) u_i from the library's own short-range tables
  mesh_potential  the CIC read-back of the mesh potential, from tests/pm_reference.py's kspace_factor, _cells and _corners
  tail            potential.c:244-337
"""
import numpy as np
from scipy.special import erfc

import pm_reference

LATTICE_ZERO = 2.8372975
NTAB = 2048
LAW_NONE, LAW_NEWTON, LAW_NEG_NEWTON = 0, 1, 2
SPLINE_NONE, SPLINE_PLUMMER, SPLINE_NEG_PLUMMER = 0, 1, 2


def law_sign(law):
    return {LAW_NEWTON: 1.0, LAW_NEG_NEWTON: -1.0}.get(int(law), 0.0)


def _coeffs(cfg, tg, sg):
    """cN[t, s], cS[t, s] of target species tg[t] against source species sg[s]"""
    ng = int(cfg.n_gravs)
    cn = np.array([[law_sign(cfg.law_accel[a][b]) for b in range(ng)] for a in range(ng)])
    cs = np.array([[{SPLINE_PLUMMER: 1.0, SPLINE_NEG_PLUMMER: -1.0}.get(int(cfg.law_spline[a][b]), 0.0) for b in range(ng)] for a in range(ng)])
    return cn[tg[:, None], sg[None, :]], cs[tg[:, None], sg[None, :]]


def species(cfg, typ):
    return np.array([cfg.type_to_grav[t] for t in range(6)], dtype=np.int64)[np.asarray(typ, dtype=np.int64)]


def plummer_pot(m, h, r):
    """plummer_pot (ngravs.c:459-472), its literal constants"""
    h_inv = 1.0 / h
    u = r * h_inv
    lo = m * h_inv * (-2.8 + u * u * (5.333333333333 + u * u * (6.4 * u - 9.6)))
    with np.errstate(divide="ignore", invalid="ignore"):
        hi = m * h_inv * (-3.2 + 0.066666666667 / u + u * u * (10.666666666667 + u * (-16.0 + u * (9.6 - 2.133333333333 * u))))
    return np.where(u < 0.5, lo, hi)


def separations(cfg, tpos, pos):
    """d[t, s, 3] = source - target (nearest image when periodic), r[t, s]"""
    d = np.asarray(pos, dtype=np.float64)[None, :, :] - np.asarray(tpos, dtype=np.float64)[:, None, :]
    if cfg.periodic:
        L = float(cfg.box_size)
        d = np.where(d > 0.5 * L, d - L, np.where(d < -0.5 * L, d + L, d))      # NEAREST
    return d, np.sqrt((d ** 2).sum(2))


def pair_terms(cfg, pos, mass, typ, tpos=None, ttyp=None, table=None):
    """terms[t, s] of the everything-opened walk, without G.  table = e_table(...): the TreePM short-range terms, pairs with
    int(r asmthfac) >= NTAB dropped"""
    tpos = pos if tpos is None else tpos
    ttyp = typ if ttyp is None else ttyp
    mass = np.asarray(mass, dtype=np.float64)
    fs = np.array([cfg.force_softening[t] for t in range(6)])
    h = np.maximum(fs[np.asarray(ttyp)][:, None], fs[np.asarray(typ)][None, :])
    tg, sg = species(cfg, ttyp), species(cfg, typ)
    cn, cs = _coeffs(cfg, tg, sg)
    d, r = separations(cfg, tpos, pos)
    m = mass[None, :]
    with np.errstate(divide="ignore", invalid="ignore"):
        far = -cn * (m / r)
    near = cs * plummer_pot(m, h, r)
    out = np.where(r >= h, far, near)
    if table is not None:
        asmth = float(cfg.asmth) if cfg.asmth > 0 else pm_reference.ASMTH * float(cfg.box_size) / int(cfg.pmgrid)
        asmthfac = 0.5 / asmth * (NTAB / 3.0)
        tab = (asmthfac * r).astype(np.int64)
        lr = m / (2 * np.pi * asmth) * table[tg[:, None], sg[None, :], np.minimum(tab, NTAB - 1)]
        out = np.where(tab < NTAB, out + lr, 0.0)
    return out


def ewald_psi(x):
    """ewald_psi (ngravs.c:761-816) at x[..., 3] in box units: the loops of the reference in their order"""
    x = np.asarray(x, dtype=np.float64)
    alpha = 2.0
    sum1 = np.zeros(x.shape[:-1])
    sum2 = np.zeros(x.shape[:-1])
    rng = range(-4, 5)
    for n0 in rng:
        for n1 in rng:
            for n2 in rng:
                dx = x - np.array([n0, n1, n2], dtype=np.float64)
                r = np.sqrt(dx[..., 0] * dx[..., 0] + dx[..., 1] * dx[..., 1] + dx[..., 2] * dx[..., 2])
                with np.errstate(divide="ignore", invalid="ignore"):
                    sum1 = sum1 + erfc(alpha * r) / r
    for h0 in rng:
        for h1 in rng:
            for h2_ in rng:
                h2 = h0 * h0 + h1 * h1 + h2_ * h2_
                if h2 > 0:
                    hdotx = x[..., 0] * h0 + x[..., 1] * h1 + x[..., 2] * h2_
                    sum2 = sum2 + 1 / (np.pi * h2) * np.exp(-np.pi * np.pi * h2 / (alpha * alpha)) * np.cos(2 * np.pi * hdotx)
    r = np.sqrt((x ** 2).sum(-1))
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.pi / (alpha * alpha) - sum1 - sum2 + 1 / r


def psi_brute(x, nmax=100):
    """psi without Ewald's split, for |x| <= 0.5: the unit masses on the lattice points n != 0 inside the sphere |n| <= nmax with
    the uniform background of density -1 inside the same sphere, relative to the origin:
        psi(x) = 2.8372975 - sum_n [1 / |x - n| - 1 / |n|] - (2 pi / 3) |x|^2
    (the ball of background gives -(2 pi / 3) |x|^2 relative to its centre, the background outside a sphere nothing, and psi(0) is
    LatticeZero).  What is cut off: the multipoles of the points outside the sphere about the origin.  l = 1 and 3 vanish by
    inversion, l = 2 by cubic symmetry, so the first is l = 4: at most |x|^4 max|K4| sum_{|n| > R} 1 / |n|^5 <= (1/16) (35/8)
    2 pi / R^2 < 2 / R^2 -- the bound psi_brute_bound returns, 2e-4 at R = 100."""
    x = np.asarray(x, dtype=np.float64)
    g = np.arange(-nmax, nmax + 1, dtype=np.float64)
    s = 0.0
    for n0 in g:                                      # plane by plane: [2 nmax + 1]^2 points at a time
        n = np.stack(np.meshgrid(np.array([n0]), g, g, indexing="ij"), -1).reshape(-1, 3)
        n2 = (n ** 2).sum(1)
        n = n[(n2 <= nmax * nmax) & (n2 > 0)]
        s += (1.0 / np.sqrt(((x[None, :] - n) ** 2).sum(1)) - 1.0 / np.sqrt((n ** 2).sum(1))).sum()
    return LATTICE_ZERO - s - 2 * np.pi / 3 * (x ** 2).sum()


def psi_brute_bound(nmax=100):
    return 2.0 / nmax ** 2


def lat_lookup(table, fac_intp, d):
    """lattice_pot_corr (forcetree.c:3895-3941): table [65, 65, 65], d[..., 3]"""
    a = np.abs(d) * fac_intp
    i = np.minimum(a.astype(np.int64), 63)
    f = a - i
    u, v, w = f[..., 0], f[..., 1], f[..., 2]
    i0, j0, k0 = i[..., 0], i[..., 1], i[..., 2]
    return (table[i0, j0, k0] * ((1 - u) * (1 - v) * (1 - w)) + table[i0, j0, k0 + 1] * ((1 - u) * (1 - v) * w) +
            table[i0, j0 + 1, k0] * ((1 - u) * v * (1 - w)) + table[i0, j0 + 1, k0 + 1] * ((1 - u) * v * w) +
            table[i0 + 1, j0, k0] * (u * (1 - v) * (1 - w)) + table[i0 + 1, j0, k0 + 1] * (u * (1 - v) * w) +
            table[i0 + 1, j0 + 1, k0] * (u * v * (1 - w)) + table[i0 + 1, j0 + 1, k0 + 1] * (u * v * w))


def ewald_exact(cfg, pos, mass, typ):
    """the walk's column of a periodic tree-only configuration with ewald_psi evaluated at every pair instead of looked up:
    sum_j [term_ij + sign_ij m_j ewald_psi(d_ij / L) / L], the row's own images (LatticeZero) included"""
    L = float(cfg.box_size)
    g = species(cfg, typ)
    cn, _ = _coeffs(cfg, g, g)
    d, r = separations(cfg, pos, pos)
    psi = ewald_psi(d / L)
    psi[r == 0] = LATTICE_ZERO
    return (pair_terms(cfg, pos, mass, typ) + cn * np.asarray(mass)[None, :] * psi / L).sum(1)


def lattice_table(sign, box):
    """the octant table the device tabulates: sign ewald_psi(i / 128, j / 128, k / 128) / box, the origin sign 2.8372975 / box"""
    g = 0.5 * np.arange(65, dtype=np.float64) / 64
    x = np.stack(np.meshgrid(g, g, g, indexing="ij"), -1)
    t = ewald_psi(x)
    t[0, 0, 0] = LATTICE_ZERO
    return sign * t / box


def e_table(pkg, cfg):
    """E[tg][sg][NTAB] = (force_tab + pot_tab) u, u_i = 3 / NTAB (i + 0.5): the long-range potential tempI(u) / u"""
    force, pot = pkg.shortrange_table(cfg)
    u = 3.0 / NTAB * (np.arange(NTAB) + 0.5)
    return (np.asarray(force) + np.asarray(pot)) * u


def mesh_potential(cfg, pos, mass, typ, tpos=None, ttyp=None):
    """G / (pi L) x the CIC read-back of the mesh potential of the sources at the targets (the own rows by default)"""
    N, L, ng = int(cfg.pmgrid), float(cfg.box_size), int(cfg.n_gravs)
    tpos = pos if tpos is None else tpos
    ttyp = typ if ttyp is None else ttyp
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    tpos = np.ascontiguousarray(tpos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    grav, tgrav = species(cfg, typ), species(cfg, ttyp)
    forward, inverse = pm_reference.numpy_ffts(N)
    smth = pm_reference.kspace_factor(cfg)
    s, d = pm_reference._cells(cfg, pos)
    ts, td = pm_reference._cells(cfg, tpos)
    out = np.zeros(len(tpos))
    for a in range(ng):
        src = np.flatnonzero(grav == a)
        rho = np.zeros((N, N, N))
        for ix, iy, iz, w in pm_reference._corners(s[src], d[src], N):
            np.add.at(rho, (ix, iy, iz), mass[src] * w)
        rho_k = forward(rho)
        for b in range(ng):
            law = int(cfg.law_greens[a][b])
            tgt = np.flatnonzero(tgrav == b)
            if law == pm_reference.LAW_NONE or not len(tgt):
                continue
            phi = inverse(rho_k * smth[law])
            acc = np.zeros(len(tgt))
            for ix, iy, iz, w in pm_reference._corners(ts[tgt], td[tgt], N):
                acc += phi[ix, iy, iz] * w
            out[tgt] += acc
    return float(cfg.G) / (np.pi * L) * out


def tail(cfg, par, pos, mass, typ, walk, mesh=None):
    """potential.c:244-337 on the walk's column: self term, LatticeZero term, G, mesh part, cosmological term"""
    pos = np.asarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    fs = np.array([cfg.force_softening[t] for t in range(6)])[np.asarray(typ)]
    pot = walk + 2.8 * mass / fs
    comoving = par is not None and par.comoving
    if comoving and cfg.periodic:
        g = species(cfg, typ)
        lz = np.array([law_sign(cfg.law_accel[k][k]) * LATTICE_ZERO for k in range(int(cfg.n_gravs))])[g]
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


def particle_set(n, seed, box=None, eps=(0.002, 0.005, 0.003, 0.008, 0.004, 0.006)):
    """mixed types with unequal softenings, two species, several pairs inside h, one coincident pair; in [0, box]^3 when box is
    given (lengths scaled by box), else a clump of unit size"""
    rng = np.random.default_rng(seed)
    L = 1.0 if box is None else float(box)
    pos = rng.uniform(0.05, 0.95, (n, 3)) * L
    typ = rng.integers(0, 6, n).astype(np.int32)
    mass = rng.uniform(0.5, 2.0, n) / max(n, 1)
    for k in range(min(6, n // 8)):                 # close pairs: inside the smaller or the larger softening of the two
        a, b = 2 * k + 2, 2 * k + 3
        pos[b] = pos[a] + rng.normal(size=3) * 0.03 * (k + 1) / 6 * L
    if n >= 2:
        pos[1] = pos[0]                            # the coincident pair
    if box is not None:
        pos = np.clip(pos, 0.0, L * (1 - 1e-12))
    return pos, mass, typ, [e * L for e in eps]
