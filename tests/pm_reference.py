"""Truth for the periodic PM force at ANY mesh size: pmforce_periodic (pm_periodic.c:204-790) restated in plain numpy fp64.

The oracle's orc_pm_periodic carries its own radix-2 FFT and so only knows PMGRID = 2^k; this module states the same
arithmetic, step for step, with numpy's FFTs (any N, odd ones included): CIC deposit, forward transform, the k-space factor of
pm_periodic.c:436-520, unnormalised inverse transform, 4-point differences, CIC gather.  tests/test_pm_reference.py holds it to
the oracle where the oracle can go, and to explicit DFT matrices where it cannot, before any kernel is judged by it.
"""
import numpy as np

LAW_NONE, LAW_NEWTON, LAW_NEG_NEWTON, LAW_YUKAWA, LAW_COLOYUK = range(5)
LAW_USER0 = 64      # user-defined Green's functions live in the host: not restated here
ASMTH = 1.25


def _cells(cfg, pos):
    """cell index min(int(to_slab*x), N-1) and the fraction inside it (which reaches 1.0 at x == L), pm_periodic.c:297-307"""
    N = int(cfg.pmgrid)
    u = (N / float(cfg.box_size)) * np.asarray(pos, dtype=np.float64)
    s = np.minimum(u.astype(np.int64), N - 1)
    return s, u - s


def _corners(s, d, N):
    """the eight (ix, iy, iz, weight) of the CIC cloud in the reference's order (pm_periodic.c:316-331, 745-776)"""
    s1 = (s + 1) % N
    x, y, z, xx, yy, zz = s[:, 0], s[:, 1], s[:, 2], s1[:, 0], s1[:, 1], s1[:, 2]
    dx, dy, dz = d[:, 0], d[:, 1], d[:, 2]
    return [(x, y, z, (1.0 - dx) * (1.0 - dy) * (1.0 - dz)), (x, yy, z, (1.0 - dx) * dy * (1.0 - dz)),
            (x, y, zz, (1.0 - dx) * (1.0 - dy) * dz), (x, yy, zz, (1.0 - dx) * dy * dz),
            (xx, y, z, dx * (1.0 - dy) * (1.0 - dz)), (xx, yy, z, dx * dy * (1.0 - dz)),
            (xx, y, zz, dx * (1.0 - dy) * dz), (xx, yy, zz, dx * dy * dz)]


def _law_greens(cfg, asmth2, law, k2):
    """the Green's functions of ngravs.c (pgdelta :390, pgyukawa :869-878) on k2 > 0 (grid units)"""
    ym = float(cfg.yukawa_imass) / (2 * np.pi)
    if law == LAW_NEWTON:
        return 1.0 / k2
    if law == LAW_NEG_NEWTON:
        return -1.0 / k2
    if law in (LAW_YUKAWA, LAW_COLOYUK):
        g = np.exp(-ym * ym * asmth2) / (k2 + ym * ym)
        return g + 1.0 / k2 if law == LAW_COLOYUK else g
    raise ValueError("pm_reference knows the built-in Green's functions only, not law id %d" % law)


def kspace_factor(cfg):
    """{law id: smth[N][N][N/2+1]} for every law of cfg.law_greens: law * -exp(-k2*asmth2) / sinc^4, 0 at k = 0"""
    N, L = int(cfg.pmgrid), float(cfg.box_size)
    asmth = float(cfg.asmth) if cfg.asmth > 0 else ASMTH * L / N
    asmth2 = ((2 * np.pi) * asmth / L) ** 2
    k = np.arange(N, dtype=np.float64)
    k = np.where(k > N // 2, k - N, k)                       # kx, ky > N/2 -> k - N; kz only runs to N/2
    kz = k[: N // 2 + 1]

    def sinc(q):
        a = np.pi * q / N
        return np.where(q != 0, np.sin(a) / np.where(q != 0, a, 1.0), 1.0)

    k2 = k[:, None, None] ** 2 + k[None, :, None] ** 2 + kz[None, None, :] ** 2
    ff = 1.0 / (sinc(k)[:, None, None] * sinc(k)[None, :, None] * sinc(kz)[None, None, :])
    k2s = np.where(k2 > 0, k2, 1.0)
    out = {}
    ng = int(cfg.n_gravs)
    for law in sorted({int(cfg.law_greens[a][b]) for a in range(ng) for b in range(ng)}):
        if law == LAW_NONE:
            continue
        smth = _law_greens(cfg, asmth2, law, k2s) * (-np.exp(-k2s * asmth2) * ff * ff * ff * ff)
        smth[0, 0, 0] = 0.0
        out[law] = smth
    return out


def numpy_ffts(N):
    """(forward, inverse): real [N][N][N] -> half spectrum [N][N][N/2+1], sign -1; and back, sign +1, NOT normalised"""
    return (lambda rho: np.fft.rfftn(rho), lambda half: np.fft.irfftn(half, s=(N, N, N), axes=(0, 1, 2)) * float(N) ** 3)


def pm_periodic(cfg, pos, mass, typ, ffts=None):
    """GravPM[n][3] (G included) of pmforce_periodic on one task.  ffts: a (forward, inverse) pair as numpy_ffts() returns,
    for a test that wants to put the transforms themselves on trial."""
    N, L, ng = int(cfg.pmgrid), float(cfg.box_size), int(cfg.n_gravs)
    if N <= 0:
        raise ValueError("pm_periodic needs PMGRID > 0")
    pos = np.ascontiguousarray(pos, dtype=np.float64)
    mass = np.asarray(mass, dtype=np.float64)
    grav = np.array([cfg.type_to_grav[t] for t in range(6)], dtype=np.int64)[np.asarray(typ, dtype=np.int64)]
    forward, inverse = ffts if ffts is not None else numpy_ffts(N)
    smth = kspace_factor(cfg)
    fac = float(cfg.G) / (np.pi * L) / (2 * L / N)
    s, d = _cells(cfg, pos)
    out = np.zeros((len(pos), 3))
    for a in range(ng):                                      # sources
        src = np.flatnonzero(grav == a)
        if not any(int(cfg.law_greens[a][b]) != LAW_NONE for b in range(ng)):
            continue
        rho = np.zeros((N, N, N))
        for ix, iy, iz, w in _corners(s[src], d[src], N):
            np.add.at(rho, (ix, iy, iz), mass[src] * w)
        rho_k = forward(rho)
        for b in range(ng):                                  # receivers; law_greens is indexed [source][target]
            law = int(cfg.law_greens[a][b])
            tgt = np.flatnonzero(grav == b)
            if law == LAW_NONE or not len(tgt):
                continue
            phi = inverse(rho_k * smth[law])
            corners = _corners(s[tgt], d[tgt], N)
            for dim in range(3):
                fg = fac * ((4.0 / 3) * (np.roll(phi, 1, dim) - np.roll(phi, -1, dim)) -
                            (1.0 / 6) * (np.roll(phi, 2, dim) - np.roll(phi, -2, dim)))
                acc = np.zeros(len(tgt))
                for ix, iy, iz, w in corners:
                    acc += fg[ix, iy, iz] * w
                out[tgt, dim] += acc
    return out
