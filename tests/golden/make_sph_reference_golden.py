#!/usr/bin/env python3
"""Generate tests/golden/sph_reference_{periodic,open}.npz: inputs and the REFERENCE's own density() -> hydro_force() outputs
(oracle/_ref/ref_sph_*, built from the reference tree by `make -C oracle ref`) for one periodic and one non-periodic mixed-type
set of 2 000 gas particles among 3 200: a coincident pair, a particle whose sphere crosses three faces of the box, MinGasHsml
set so that a third of the particles are clamped, and a timestep mix with a Timebase_interval at which the viscosity limiter
acts on both sides of its minimum.  CPU only; needs the executables; run from the repo root:
    python tests/golden/make_sph_reference_golden.py
tests/test_sph_reference.py holds the restatements (CPU) and the device (GPU) to these files, with or without the reference."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import __graft_entry__ as ge  # noqa: E402
import ref_sph as R  # noqa: E402
import test_sph_density as D  # noqa: E402
import test_sph_hydro as H  # noqa: E402

N, NGAS, SEED = 3200, 2000, 31
SETS = {"periodic": ("uniform", 1000.0), "open": ("plummer", 0.0)}
RECORDED = ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor", "pressure", "hydro_accel", "dt_entropy", "max_signal_vel")


def main():
    pkg = ge.load_package()
    for name, (kind, box) in SETS.items():
        pos, mass, ptype, vel, hsml0, gas = D.gas_mix(pkg, kind, n=N, ngas=NGAS, seed=SEED)
        vel = vel - (0.02 * (pos - 500.0) if kind == "uniform" else 2.0 * pos)
        pos[gas[1]] = pos[gas[0]]
        if box:
            pos[gas[2]] = [0.4, 999.7, 0.2]
        rng = np.random.default_rng(SEED + 100)
        timestep = (rng.choice([0, 1, 2, 4, 8], N) * 2 ** rng.integers(0, 4, N)).astype(np.int32)
        entropy = H.full(N, gas, 10.0 ** rng.uniform(-0.5, 0.5, NGAS), fill=0.0)
        tbi = H.KIND_TBI[kind] * ((12000 / NGAS) ** (1.0 / 3) if kind == "uniform" else 1.0)
        free = R.run(pos, mass, ptype, vel, hsml0, box=box)
        minh = float(np.quantile(free["hsml"][gas], 1.0 / 3))
        out = R.run(pos, mass, ptype, vel, hsml0, box=box, min_gas_hsml=minh, entropy=entropy, visc=H.VISC, timestep=timestep, tbi=tbi)
        z = dict(pos=pos, mass=mass, ptype=ptype, vel=vel, gas=gas.astype(np.int32), hsml0=hsml0[gas], entropy=entropy[gas], timestep=timestep,
                 box=np.float64(box), min_gas_hsml=np.float64(minh), tbi=np.float64(tbi), ref_passes=np.int32(out["passes"]))
        for k in RECORDED:
            z["ref_" + k] = out[k][gas]
        path = os.path.join(ROOT, "tests", "golden", "sph_reference_%s.npz" % name)
        np.savez_compressed(path, **z)
        print("%s: %d bytes, %d passes, %d of %d gas particles at MinGasHsml" % (path, os.path.getsize(path), out["passes"],
                                                                                 (out["hsml"][gas] == minh).sum(), NGAS))


if __name__ == "__main__":
    main()
