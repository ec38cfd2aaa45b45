#!/usr/bin/env python3
"""Generate tests/golden/global_reference.npz: inputs and the REFERENCE's own compute_global_quantities_of_system() output, the
119 doubles of SysState, for three builds of its global.c, all without comoving integration:
    pmgrid    -DPMGRID        make_set(1037, 1137, P, True), pm_ti = (TI - 2^20, TI + 2^20), a seeded negative potential column
    nomesh    (no switch)     the same set
    isotherm  -DISOTHERM_EQS  a set of 257 rows with gamma = 1
    pmgrid_kick -DPMGRID      the first set with pm_ti = (TI - 2^20, TI + 2^18): the middle of the first variant's PM step is TI itself,
                              so its long-range prediction is over no time; here GravPM does enter
global.c and allvars.c of the reference tree are compiled unmodified and in place with the stand-ins of oracle/ref_stubs/ and
linked with the driver below -- this project's text: it fills P[], SphP[] and All from a file, calls the routine and dumps
SysState; the two kick-factor functions, which only the comoving branch calls, abort.  Build products go to a temporary directory;
nothing of the reference is copied into the tree, the npz holds inputs and recorded doubles only.  CPU only; needs the reference
tree (NGRAVS_REFERENCE, default /root/reference) and gcc; run from the repo root:
    python tests/golden/make_global_golden.py
tests/test_global_quantities.py holds its restatement to this file, with or without the reference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import test_global_quantities as Q  # noqa: E402
import test_time_integration as T  # noqa: E402

REFERENCE = os.environ.get("NGRAVS_REFERENCE", "/root/reference")
# (the flags of oracle/Makefile's REF_CFLAGS)
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DDOUBLEPRECISION", "-DN_GRAVS=2", "-DNGRAVS_EN=64", "-DNGRAVS_TIMESTEP_SCALE=1.0"]
VARIANTS = {"pmgrid": ("a", ["-DPMGRID=16"], Q.PM_TI), "nomesh": ("a", [], None), "isotherm": ("b", ["-DISOTHERM_EQS"], None),
            "pmgrid_kick": ("a", ["-DPMGRID=16"], Q.PM_TI_KICK)}
DOUBLES = ("pos", "vel", "mass", "grav_accel", "grav_pm", "hydro_accel", "entropy", "dt_entropy", "density", "potential")

DRIVER = r"""
/* driver of tests/golden/make_global_golden.py: in = n, Ti_Current, PM_Ti_begstep, PM_Ti_endstep (int), Timebase_interval
 * (double), then type, ti_begstep, ti_endstep (int [n]) and pos[3], vel[3], mass, grav_accel[3], grav_pm[3], hydro_accel[3],
 * entropy, dt_entropy, density, potential (double [n] each, component-major rows); out = SysState */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "allvars.h"
#include "proto.h"

double get_gravkick_factor(int time0, int time1) { fprintf(stderr, "get_gravkick_factor reached\n"); abort(); }
double get_hydrokick_factor(int time0, int time1) { fprintf(stderr, "get_hydrokick_factor reached\n"); abort(); }

static void rd(void *p, size_t size, size_t count, FILE *f)
{
  if(fread(p, size, count, f) != count) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
  FILE *f = fopen(argv[1], "rb");
  int head[4], n, i, j, *ty, *tb, *te;
  double tbi, *x;
  if(argc != 3 || !f) return 2;
  rd(head, sizeof(int), 4, f);
  rd(&tbi, sizeof(double), 1, f);
  n = head[0];
  memset(&All, 0, sizeof All);
  ThisTask = 0; NTask = 1; NumPart = n;
  All.ComovingIntegrationOn = 0; All.Time = 0; All.Ti_Current = head[1]; All.Timebase_interval = tbi;
#ifdef PMGRID
  All.PM_Ti_begstep = head[2]; All.PM_Ti_endstep = head[3];
#endif
  P = malloc(sizeof(struct particle_data) * n);
  SphP = malloc(sizeof(struct sph_particle_data) * n);   /* indexed like P[]: global.c reads SphP[i] where P[i].Type == 0 */
  memset(P, 0, sizeof(struct particle_data) * n);
  memset(SphP, 0, sizeof(struct sph_particle_data) * n);
  ty = malloc(sizeof(int) * n); tb = malloc(sizeof(int) * n); te = malloc(sizeof(int) * n);
  x = malloc(sizeof(double) * 3 * n);
  rd(ty, sizeof(int), n, f); rd(tb, sizeof(int), n, f); rd(te, sizeof(int), n, f);
  for(i = 0; i < n; i++) { P[i].Type = ty[i]; P[i].Ti_begstep = tb[i]; P[i].Ti_endstep = te[i]; }
#define VEC(field) rd(x, sizeof(double), 3 * n, f); for(i = 0; i < n; i++) for(j = 0; j < 3; j++) field[j] = x[3 * i + j];
#define SKIP3 rd(x, sizeof(double), 3 * n, f);
#define SCA(field) rd(x, sizeof(double), n, f); for(i = 0; i < n; i++) field = x[i];
  VEC(P[i].Pos) VEC(P[i].Vel) SCA(P[i].Mass) VEC(P[i].GravAccel)
#ifdef PMGRID
  VEC(P[i].GravPM)
#else
  SKIP3
#endif
  VEC(SphP[i].HydroAccel) SCA(SphP[i].Entropy) SCA(SphP[i].DtEntropy) SCA(SphP[i].Density) SCA(P[i].Potential)
  fclose(f);
  compute_global_quantities_of_system();
  f = fopen(argv[2], "wb");
  if(!f || fwrite(&SysState, sizeof SysState, 1, f) != 1) return 3;
  fclose(f);
  return 0;
}
"""


def build(tmp, name, flags):
    exe = os.path.join(tmp, "ref_global_" + name)
    stubs = os.path.join(ROOT, "oracle", "ref_stubs")
    cmd = ["gcc"] + CFLAGS + flags + ["-I" + stubs, "-I" + REFERENCE, "-o", exe, os.path.join(tmp, "driver.c"),
                                     os.path.join(stubs, "ref_stubs.c"), os.path.join(REFERENCE, "global.c"), os.path.join(REFERENCE, "allvars.c"), "-lm"]
    subprocess.check_call(cmd)
    return exe


def run(exe, tmp, c, ti, pm_ti, tbi):
    src, dst = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
    with open(src, "wb") as f:
        f.write(np.array([len(c["type"]), ti, pm_ti[0], pm_ti[1]], dtype=np.int32).tobytes())
        f.write(np.float64(tbi).tobytes())
        for k in ("type", "ti_begstep", "ti_endstep"):
            f.write(np.ascontiguousarray(c[k], dtype=np.int32).tobytes())
        for k in DOUBLES:
            f.write(np.ascontiguousarray(c[k], dtype=np.float64).tobytes())
    subprocess.check_call([exe, src, dst], timeout=60)
    out = np.fromfile(dst, dtype=np.float64)
    assert out.shape == (119,)
    return out


def sets():
    Pa, Pb = T.params(False), T.params(False, gamma=1.0)
    a, b = T.make_set(1037, 1137, Pa, True), T.make_set(257, 1257, Pb, False)
    a["potential"], b["potential"] = Q.potential_of(1037, 2137), Q.potential_of(257, 2257)
    return {"a": (Pa, a), "b": (Pb, b)}


def main():
    if not os.path.exists(os.path.join(REFERENCE, "global.c")):
        sys.exit("the reference tree is not at %s" % REFERENCE)
    S = sets()
    z = dict(variants=np.array(list(VARIANTS)))
    for s, (P, c) in S.items():
        for k in Q.READ + ("potential",):
            z["%s_%s" % (s, k)] = c[k]
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.c"), "w") as f:
            f.write(DRIVER)
        for name, (s, flags, pm_ti) in VARIANTS.items():
            P, c = S[s]
            state = run(build(tmp, name, flags), tmp, c, T.TI, pm_ti or [0, 0], P["timebase_interval"])
            assert np.isfinite(state).all()
            sums, A = Q.ref_global(c, P, T.TI, pm_ti, c["potential"])
            want, scale = Q.finish(sums), Q.state_scale(sums, A)
            ok = scale > 0
            print("%-9s the restatement deviates from the reference by at most %.3g of the scale" % (name, np.max(np.abs(state - want)[ok] / scale[ok])))
            z.update({name + "_set": np.array(s), name + "_gamma": np.float64(P["gamma"]), name + "_tbi": np.float64(P["timebase_interval"]),
                      name + "_ti": np.int32(T.TI), name + "_pm_ti": np.array(pm_ti or [0, 0], dtype=np.int32), name + "_state": state})
    path = os.path.join(ROOT, "tests", "golden", "global_reference.npz")
    np.savez_compressed(path, **z)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
