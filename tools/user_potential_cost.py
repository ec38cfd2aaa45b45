#!/usr/bin/env python3
"""Kernel time of the potential walk that evaluates a model's own potential tables (ngravs_create_with_potentials) next to the
built-in walk, tools/potential_cost.py's method: a uniform box of 2^log2n particles, two species, theta = 0.5, tree-only without
periodic boundaries and TreePM; three engines on the same particles --
  builtin   every pair Newtonian, the built-in companions                       (k_potential_walk<2, PM, 0, 0>)
  copies    the same wiring, user copies of newtonian_pot / plummer_pot on every pair  (k_potential_walk<2, PM, 0, 1>)
  c4        the C4 wiring: [g][g] Newton with its built-in companion, the coloyuk pairs with Newton + Yukawa entries
-- alternating in one process after a warm-up, five repetitions each; HIP-event times of the walk kernel alone
(ngravs_last_potential_ms).  The model is tests/user_potential/model.c, compiled here.  DESIGN §8 records the numbers.
  python tools/user_potential_cost.py [log2n]"""
import ctypes as C
import json
import os
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import __graft_entry__ as ge

REPS = 5


def main():
    log2n = int(sys.argv[1]) if len(sys.argv) > 1 else 20
    pkg = ge.load_package()
    A = pkg.abi
    tmp = tempfile.mkdtemp()
    so = os.path.join(tmp, "libmodel.so")
    subprocess.check_call(["gcc", "-O2", "-ffp-contract=off", "-shared", "-fPIC", os.path.join(ROOT, "tests", "user_potential", "model.c"),
                           "-o", so, "-lm"])
    mdl = C.CDLL(so)
    mdl.mdl_set.argtypes = [C.c_double, C.c_double]
    n, L, ng = 1 << log2n, 1000.0, 2
    mdl.mdl_set(60.0 / L, L)                                   # YUKAWA_IMASS = 60 of the C4 box
    fn = lambda name: A.GravityFn((name, mdl))                 # noqa: E731
    pos, mass, typ = pkg.ic.uniform_box(n, box=L, n_gravs=ng, seed=7)
    pmgrid = 16
    while (pmgrid * 2) ** 3 <= 2 * n:
        pmgrid *= 2
    eps = L / (40 * n ** (1 / 3))
    pairs = [(a, b) for a in range(ng) for b in range(ng)]
    variants = {"builtin": ("newton", None),
                "copies": ("newton", [(a, b, fn("mdl_newton_pot"), fn("mdl_plummer_pot"), None, 2.8372975) for a, b in pairs]),
                "c4": ("c4", [(a, b, fn("mdl_coloyuk_pot"), fn("mdl_coloyuk_spline"), None, 0.0) for a, b in pairs if a != b])}
    out = {"particles": n, "pmgrid": pmgrid, "repetitions": REPS}
    for name, periodic, mesh in (("treepm", 1, pmgrid), ("tree_only", 0, 0)):
        engines, column = {}, np.zeros(n)
        for v, (wiring, pots) in variants.items():
            cfg = pkg.make_config(n_gravs=ng, periodic=periodic, pmgrid=mesh, box_size=L if periodic else 0.0, G=1.0, theta=0.5,
                                  softening=[eps] * 6, type_to_grav=pkg.ic.default_type_to_grav(ng), wiring=wiring, walk_mode=pkg.WALK_STRICT)
            eng = engines[v] = pkg.Engine(cfg, user_potentials=pots)
            eng.set_particles(pos, mass, typ)
            eng.compute_accelerations(pm_step=bool(mesh))      # decomposition, tree, first walk
            eng.compute_potential(into=column)                 # warm-up: tables, mesh plans
        ms = {v: [] for v in variants}
        nint = {}
        for _ in range(REPS):
            for v, eng in engines.items():
                _, ni = eng.compute_potential(into=column, want_nint=True)
                ms[v].append(eng.last_potential_ms())
                nint[v] = float(ni.mean())
        res = {}
        for v in variants:
            res[v] = {"walk_ms": ms[v], "median": float(np.median(ms[v])), "spread": float(max(ms[v]) - min(ms[v])), "ia_per_particle": nint[v]}
        for v in ("copies", "c4"):
            res[v]["ratio_to_builtin"] = res[v]["median"] / res["builtin"]["median"]
        out[name] = res
        for eng in engines.values():
            eng.close()
    print(json.dumps(out, indent=1))


if __name__ == "__main__":
    main()
