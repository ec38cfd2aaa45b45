"""CPU: tests/pm_reference.py, the any-mesh-size truth of the PM force, is pinned before it judges a kernel
(tests/test_gpu_pm_mesh.py): against the oracle's own pmforce_periodic where that can go (PMGRID = 2^k), against itself with the
FFTs replaced by explicit DFT matrices where it cannot, and by momentum conservation.  The refusals of a PMGRID the library's
mesh layout cannot hold are checked here too; none of this needs a GPU.

Bound 1e-12 of max |GravPM|: the two restatements differ by summation order and FFT rounding only (measured 1e-15 .. 4e-15);
1e-12 leaves room for another FFT backend and stays two decades under the 1e-10 the kernels are held to.
"""
import ctypes as C

import numpy as np
import pytest

import pm_reference

BOUND = 1e-12
CASES = [("newton", 1), ("c4", 2), ("coloyuk", 2), ("yukawa_offdiag", 2), ("c4", 3)]   # the wirings of test_strict_treepm_and_pm


def _config(pkg, wiring, ng, N, L, G=43007.1):
    return pkg.make_config(n_gravs=ng, periodic=1, pmgrid=N, box_size=L, G=G, theta=0.5, softening=[L / 2000] * 6,
                           type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring)


def _particles(pkg, n, L, ng, N, seed):
    """a clumped set; rows 0.. are particles at 0, at L, at L(1-2^-53) and exactly on cell boundaries k L/N"""
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=seed)
    pos[: n // 3] = 0.2 * L + 0.3 * (pos[: n // 3] - 0.2 * L)
    pos[0] = 0.0
    pos[1] = L
    pos[2] = L * (1 - 2.0 ** -53)
    pos[3] = (3 * L / N, 0.0, (N - 1) * L / N)
    for j, k in enumerate((1, N // 2, N - 1, N // 3)):
        pos[4 + j] = (k * L / N, (k + 1) % N * L / N, (N - k) * L / N)
        pos[8 + j, j % 3] = k * L / N                      # one coordinate on a boundary, the others anywhere
    mass = np.random.default_rng(seed).uniform(0.5, 1.5, n) / n
    return pos, mass, typ


@pytest.mark.parametrize("N", [16, 32, 64])
@pytest.mark.parametrize("wiring,ng", CASES)
def test_reference_equals_the_oracle(pkg, O, wiring, ng, N):
    n = 6000
    L = 1e4 if N != 32 else 1.0
    pos, mass, typ = _particles(pkg, n, L, ng, N, seed=5 + N)
    cfg = _config(pkg, wiring, ng, N, L)
    want = O.pm_periodic(cfg, pos, mass, typ)
    got = pm_reference.pm_periodic(cfg, pos, mass, typ)
    err = np.abs(got - want).max() / np.abs(want).max()
    print("pm_reference vs oracle [%s/%d N=%d]: %.2e" % (wiring, ng, N, err))
    assert np.isfinite(got).all() and np.abs(want).max() > 0
    assert err < BOUND


def _dft_ffts(N):
    """the transforms as explicit DFT matrices exp(-+2 pi i jk/N) applied along each axis: no FFT algorithm, no half-spectrum
    shortcut.  forward keeps z <= N/2 of the full spectrum; inverse rebuilds the other half as the conjugate of (-x, -y, -z),
    transforms with the + sign, not normalised, and must come out real."""
    j = np.arange(N)
    W = np.exp(-2j * np.pi * np.outer(j, j) / N)
    h = N // 2 + 1

    def forward(rho):
        f = np.einsum("xa,abc->xbc", W, rho.astype(complex))
        f = np.einsum("yb,xbc->xyc", W, f)
        f = np.einsum("zc,xyc->xyz", W, f)
        return f[:, :, :h]

    def inverse(half):
        full = np.empty((N, N, N), dtype=complex)
        full[:, :, :h] = half
        m = (-j) % N
        for z in range(h, N):
            full[:, :, z] = np.conj(half[m][:, m][:, :, N - z])
        Wc = np.conj(W)
        f = np.einsum("xa,abc->xbc", Wc, full)
        f = np.einsum("yb,xbc->xyc", Wc, f)
        f = np.einsum("zc,xyc->xyz", Wc, f)
        assert np.abs(f.imag).max() <= 1e-12 * np.abs(f.real).max()
        return f.real

    return forward, inverse


@pytest.mark.parametrize("N", [12, 20])
@pytest.mark.parametrize("wiring,ng", [("c4", 2), ("yukawa_offdiag", 2)])
def test_reference_equals_itself_without_an_fft(pkg, wiring, ng, N):
    """sign, normalisation and Hermitian-half conventions at sizes the oracle cannot reach"""
    n, L = 4000, 1e4 if N == 12 else 1.0
    pos, mass, typ = _particles(pkg, n, L, ng, N, seed=70 + N)
    cfg = _config(pkg, wiring, ng, N, L)
    got = pm_reference.pm_periodic(cfg, pos, mass, typ)
    want = pm_reference.pm_periodic(cfg, pos, mass, typ, ffts=_dft_ffts(N))
    err = np.abs(got - want).max() / np.abs(want).max()
    print("pm_reference, numpy FFT vs DFT matrices [%s/%d N=%d]: %.2e" % (wiring, ng, N, err))
    assert np.abs(want).max() > 0
    assert err < BOUND


@pytest.mark.parametrize("N", [20, 48, 33])
@pytest.mark.parametrize("wiring,ng", [("newton", 1), ("c4", 2)])
def test_reference_conserves_momentum(pkg, wiring, ng, N):
    """deposit and gather use the same cloud and the difference stencil is antisymmetric: the mesh force obeys Newton's
    third law to rounding at any N, odd ones included"""
    n, L = 20000, 1e4
    pos, mass, typ = _particles(pkg, n, L, ng, N, seed=90 + N)
    cfg = _config(pkg, wiring, ng, N, L)
    f = mass[:, None] * pm_reference.pm_periodic(cfg, pos, mass, typ)
    net, tot = np.linalg.norm(f.sum(axis=0)), np.linalg.norm(f, axis=1).sum()
    print("pm_reference momentum [%s/%d N=%d]: |sum m a| / sum |m a| = %.2e" % (wiring, ng, N, net / tot))
    assert tot > 0 and net <= 1e-13 * tot


def test_reference_refuses_user_laws(pkg):
    cfg = _config(pkg, "newton", 1, 16, 1.0)
    cfg.law_greens[0][0] = pm_reference.LAW_USER0
    pos, mass, typ = _particles(pkg, 100, 1.0, 1, 16, seed=1)
    with pytest.raises(ValueError):
        pm_reference.pm_periodic(cfg, pos, mass, typ)


def test_odd_or_negative_pmgrid_is_refused_without_a_gpu(pkg, have_lib):
    """the mesh is laid out [N][N][N+2] for the in-place real-to-complex transform, right only for even N: an odd PMGRID would
    give wrong forces with no error, so ngravs_create refuses it (and a negative one), and says why"""
    h = C.c_void_p()
    for bad in (33, 1, 95, -32, -1):
        cfg = _config(pkg, "c4", 2, bad, 1.0)
        assert have_lib.ngravs_create(C.byref(cfg), C.byref(h)) == -1          # NGRAVS_ERR_ARG
        assert not h.value
        assert b"PMGRID" in have_lib.ngravs_last_error(None)
