"""PM beside the walk (ngravs_compute_accelerations): the two masked streams, their CUs, and the results of the overlapped step"""
import numpy as np
import pytest

N = 1 << 20


def _engine(pkg, pm_cus):
    L = 1.0
    pos, mass, typ = pkg.ic.uniform_box(N, box=L, n_gravs=2, seed=5)
    cfg = pkg.make_config(n_gravs=2, periodic=1, pmgrid=128, box_size=L, G=1.0, theta=0.5, err_tol_force_acc=0.005,
                          softening=[L / (40 * N ** (1 / 3))] * 6, type_to_grav=pkg.ic.default_type_to_grav(2), wiring="c4",
                          walk_mode=pkg.WALK_GROUP)
    eng = pkg.Engine(cfg)
    if pm_cus is not None:
        eng.set_tuning(pm_cus=pm_cus)
    eng.set_particles(pos, mass, typ)
    eng.compute_accelerations(pm_step=True)    # the angle criterion with OldAcc = 0, as the reference's first pass
    _, old, _ = eng.get_accel()
    eng.set_opening(0.0, 0.005)
    eng.set_old_acc(old)
    eng.compute_accelerations(pm_step=True)
    return eng


@pytest.mark.gpu
def test_masked_streams_split_the_device(pkg):
    eng = _engine(pkg, 32)
    assert eng.last_pm_cus() == 32
    dev = set(eng.cu_probe(0, 8192).tolist())
    pm = set(eng.cu_probe(1, 4096).tolist())
    walk = set(eng.cu_probe(2, 8192).tolist())
    assert len(pm) == 32 and len(walk) == len(dev) - 32
    assert not (pm & walk) and (pm | walk) == dev
    assert np.bincount(np.array(sorted(pm)) >> 8, minlength=8).tolist() == [4] * 8   # 4 CUs of every XCD
    eng.close()


@pytest.mark.gpu
def test_overlapped_step_computes_what_the_serial_step_does(pkg):
    res = {}
    for R in (0, 32):
        eng = _engine(pkg, R)
        acc, old, cost, gpm = eng.get_accel(want_pm=True)
        res[R] = (acc, old, cost, gpm, eng.stats().interactions, eng.last_pm_cus(), eng.last_walk_kernel())
        eng.close()
    a, b = res[0], res[32]
    assert a[5] == 0 and b[5] == 32
    assert np.array_equal(a[0], b[0])             # GravAccel
    assert np.array_equal(a[2], b[2])             # GravCost
    assert a[4] == b[4]                           # interactions
    assert np.abs(a[3] - b[3]).max() <= 1e-13 * np.abs(a[3]).max()   # GravPM (the deposit's atomics)
    assert np.abs(a[1] - b[1]).max() <= 1e-13 * np.abs(a[1]).max()   # OldAcc
    assert b[6] == a[6] == pkg.abi.KERNEL_GROUP


@pytest.mark.gpu
def test_pm_cus_knob_range(pkg):
    cfg = pkg.make_config(n_gravs=1, periodic=1, pmgrid=32, box_size=1.0, G=1.0, theta=0.5, softening=[0.01] * 6,
                          type_to_grav=pkg.ic.default_type_to_grav(1), wiring="newton")
    eng = pkg.Engine(cfg)
    for v in (-1, 0, 8, 16, 24, 32):
        eng.set_tuning(pm_cus=v)
    for v in (-2, 4, 40):
        with pytest.raises(pkg.NgravsError):
            eng.set_tuning(pm_cus=v)
    eng.close()
