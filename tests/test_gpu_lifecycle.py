"""GPU: engines are created, used and destroyed over and over in one process.  Every device buffer, event and stream of an engine
belongs to an owner that frees it (csrc/devbuf.hpp), and ngravs_destroy is `delete` after a synchronisation: three cycles of two
small engines that between them make FFT plans, walk scratch, batch events, masked streams, SPH buffers and the temporaries of
the direct sum.  Every call must succeed in every cycle, and the strict walk -- one thread per target, the same inputs -- must
give the same bits in each.  Free device memory is not looked at: other processes move it."""
import numpy as np
import pytest

CYCLES = 3
NORM_COEFF = 4.188790204786   # allvars.h:109-115
DES, DEV = 32.0, 2.0


def tree_only_cycle(pkg, pos, mass, ptype, rows):
    """engine (a): tree-only, strict walk; accelerations, potentials, a direct sum"""
    cfg = pkg.make_config(n_gravs=2, softening=[0.5] * 6, type_to_grav=pkg.ic.default_type_to_grav(2), wiring="newton",
                          walk_mode=pkg.WALK_STRICT)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.compute_accelerations(pm_step=False)
    acc = eng.get_accel()[0]
    pot = eng.compute_potential()
    direct = eng.direct_sum(rows)
    eng.close()
    return acc, pot, direct


def treepm_gas_cycle(pkg, pos, mass, ptype, vel, hsml, box):
    """engine (b): periodic TreePM, group walk; two PM steps (the second may run PM beside the walk), then the SPH density"""
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=16, box_size=box, softening=[box / 400] * 6, type_to_grav=[0, 0, 1, 0, 0, 0],
                          wiring="newton", walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(cfg)
    eng.set_particles(pos, mass, ptype)
    eng.compute_accelerations(pm_step=True)
    eng.compute_accelerations(pm_step=True)
    acc, _, _, pm = eng.get_accel(want_pm=True)
    res = eng.sph_density(vel, hsml, DES, DEV)
    eng.close()
    return acc, pm, res


@pytest.mark.gpu
def test_three_create_use_destroy_cycles_of_two_engines(pkg):
    box = 1000.0
    pos_a, mass_a, type_a = pkg.ic.uniform_box(1000, box=box, n_gravs=2, seed=21)
    assert len(np.unique(np.asarray(pkg.ic.default_type_to_grav(2))[type_a])) == 2
    rows = np.arange(0, 1000, 63, dtype=np.int32)[:16]
    n, ngas = 2000, 500
    rng = np.random.default_rng(22)
    pos_b, mass_b, _ = pkg.ic.uniform_box(n, box=box, n_gravs=2, seed=22)
    type_b = np.where(rng.permutation(n) < ngas, 0, 1 + (np.arange(n) % 2)).astype(np.int32)
    gas = np.nonzero(type_b == 0)[0]
    vel = rng.normal(0.0, 1.0, (n, 3))
    hsml = np.zeros(n)
    hsml[gas] = (DES / (NORM_COEFF * ngas / box ** 3)) ** (1.0 / 3)   # DesNumNgb gas particles at the mean gas density
    first = None
    for cycle in range(CYCLES):
        acc, pot, direct = tree_only_cycle(pkg, pos_a, mass_a, type_a, rows)
        assert len(rows) == 16 and np.isfinite(acc).all() and np.isfinite(pot).all() and np.isfinite(direct).all()
        assert np.abs(acc).max() > 0 and np.abs(pot).min() > 0
        if first is None:
            first = (acc, pot)
        assert np.array_equal(acc, first[0]) and np.array_equal(pot, first[1]), "cycle %d differs from cycle 1" % (cycle + 1)
        acc_b, pm_b, res = treepm_gas_cycle(pkg, pos_b, mass_b, type_b, vel, hsml, box)
        assert np.isfinite(acc_b).all() and np.isfinite(pm_b).all() and np.abs(pm_b).max() > 0
        for k in ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor"):
            assert np.isfinite(res[k]).all(), (cycle, k)
        assert np.all(res["density"][gas] > 0) and np.all(res["hsml"][gas] > 0)
