#!/usr/bin/env python3
"""Kernel time of the potential walk next to the strict force walk, same tree, same opening criterion (theta = 0.5): a uniform box
of 2^log2n particles, two species, as TreePM (the C4 layout with every pair Newtonian -- the C4 wiring's coloyuk pairs have no
potential companion) and tree-only without periodic boundaries.  After a warm-up of both, compute_potential() and gravity_tree()
alternate in one process, five repetitions each; the times are HIP-event times of the walk kernels alone
(ngravs_last_potential_ms, ngravs_stats_t.walk_kernel_ms).  DESIGN §8 "Potentials" records the numbers.
  python tools/potential_cost.py [log2n]"""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

REPS = 5


def main():
    log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    pkg = ge.load_package()
    n, L, ng = 1 << log2n, 1000.0, 2
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=7)
    pmgrid = 16
    while (pmgrid * 2) ** 3 <= 2 * n:
        pmgrid *= 2
    eps = L / (40 * n ** (1 / 3))
    out = {"particles": n, "pmgrid": pmgrid, "repetitions": REPS}
    for name, periodic, mesh in (("treepm", 1, pmgrid), ("tree_only", 0, 0)):
        cfg = pkg.make_config(n_gravs=ng, periodic=periodic, pmgrid=mesh, box_size=L if periodic else 0.0, G=1.0, theta=0.5,
                              softening=[eps] * 6, type_to_grav=pkg.ic.default_type_to_grav(ng), wiring="newton", walk_mode=pkg.WALK_STRICT)
        eng = pkg.Engine(cfg)
        eng.set_particles(pos, mass, typ)
        eng.compute_accelerations(pm_step=bool(mesh))      # decomposition, tree, first walk
        column = np.zeros(n)
        eng.compute_potential(into=column)                 # warm-up: tables, mesh plans
        eng.gravity_tree()
        pot_ms, force_ms = [], []
        for _ in range(REPS):
            _, nint = eng.compute_potential(into=column, want_nint=True)
            pot_ms.append(eng.last_potential_ms())
            eng.gravity_tree()
            force_ms.append(eng.stats().walk_kernel_ms)
        _, _, cost = eng.get_accel()
        out[name] = {"potential_walk_ms": pot_ms, "force_walk_ms": force_ms,
                     "potential_median": float(np.median(pot_ms)), "force_median": float(np.median(force_ms)),
                     "potential_spread": float(max(pot_ms) - min(pot_ms)), "force_spread": float(max(force_ms) - min(force_ms)),
                     "ia_per_particle_potential": float(nint.mean()), "ia_per_particle_force": float(cost.mean())}
        eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
