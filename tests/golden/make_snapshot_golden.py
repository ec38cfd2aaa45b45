#!/usr/bin/env python3
"""Generate tests/golden/snapshot_reference.npz: one input set of 600 rows and the bytes of the files that the REFERENCE's own
savepositions() writes for it, for five builds of its io.c (tests/snapshot_ref.py: VARIANTS):
    stock_f1       (no switch)  SnapFormat 1
    stock_f2       (no switch)  SnapFormat 2
    full           -DPERIODIC -DPMGRID=16 -DOUTPUTACCELERATION -DOUTPUTCHANGEOFENTROPY -DOUTPUTTIMESTEP -DOUTPUTPOTENTIAL, not comoving,
                   a PM step whose middle is not Ti_Current, SnapFormat 2
    full_comoving  the same switches, ComovingIntegrationOn, SnapFormat 1
    isotherm       -DISOTHERM_EQS
io.c and allvars.c of the reference tree are compiled unmodified and in place with the stand-ins of oracle/ref_stubs/ and linked with
the driver below -- this project's text: it fills P[], SphP[] and All from a file, defines what io.c does not find (the MPI send that
one task never reaches, distribute_file for one task, dmax, the timers, endrun, and the two kick-factor functions as look-ups in
tables that the input file carries: those of the Python restatement in tests/test_time_integration.py) and calls savepositions(0).
Where run.c links with aborting stand-ins, find_next_outputtime() is recorded too, for a few dozen (rule, ti_curr) pairs.
Build products go to a temporary directory; nothing of the reference is copied into the tree, the npz holds inputs and recorded
bytes only.  CPU only; needs the reference tree (NGRAVS_REFERENCE, default /root/reference) and gcc; run from the repo root:
    python tests/golden/make_snapshot_golden.py
tests/test_snapshot.py holds its restatement and the library to this file, with or without the reference."""
import os
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(ROOT, "tests"))
import snapshot_ref as S  # noqa: E402
import test_time_integration as T  # noqa: E402

REFERENCE = os.environ.get("NGRAVS_REFERENCE", "/root/reference")
# (the flags of oracle/Makefile's REF_CFLAGS)
CFLAGS = ["-O2", "-ffp-contract=off", "-w", "-DDOUBLEPRECISION", "-DN_GRAVS=2", "-DNGRAVS_EN=64", "-DNGRAVS_TIMESTEP_SCALE=1.0"]
DOUBLES = ("pos", "vel", "mass", "grav_accel", "grav_pm", "hydro_accel", "entropy", "dt_entropy", "density", "hsml", "potential")

DRIVER = r"""
/* driver of tests/golden/make_snapshot_golden.py: in = n, Ti_Current, PM_Ti_begstep, PM_Ti_endstep, ComovingIntegrationOn,
 * SnapFormat (int), then Timebase_interval, TimeBegin, TimeMax, BoxSize, Omega0, OmegaLambda, HubbleParam, MinEgySpec,
 * MassTable[6], the gravkick table and the hydrokick table [DRIFT_TABLE_LENGTH each] (double), then type, ti_begstep, ti_endstep,
 * id (int [n]) and pos[3], vel[3], mass, grav_accel[3], grav_pm[3], hydro_accel[3], entropy, dt_entropy, density, hsml, potential
 * (double [n] each); argv[2] is the output directory (with its slash): savepositions(0) writes <dir>snap_000 */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <math.h>
#include <mpi.h>
#include "allvars.h"
#include "proto.h"

static double GravKickTab[DRIFT_TABLE_LENGTH], HydroKickTab[DRIFT_TABLE_LENGTH], LogBegin, LogMax;

/* the look-up of a kick factor between two integer times, in the table of the input file */
static double lookup(const double *tab, int time0, int time1)
{
  double a1 = LogBegin + time0 * All.Timebase_interval, a2 = LogBegin + time1 * All.Timebase_interval, u1, u2, df1, df2;
  int i1, i2;
  u1 = (a1 - LogBegin) / (LogMax - LogBegin) * DRIFT_TABLE_LENGTH;
  i1 = (int) u1;
  if(i1 >= DRIFT_TABLE_LENGTH) i1 = DRIFT_TABLE_LENGTH - 1;
  df1 = i1 <= 1 ? u1 * tab[0] : tab[i1 - 1] + (tab[i1] - tab[i1 - 1]) * (u1 - i1);
  u2 = (a2 - LogBegin) / (LogMax - LogBegin) * DRIFT_TABLE_LENGTH;
  i2 = (int) u2;
  if(i2 >= DRIFT_TABLE_LENGTH) i2 = DRIFT_TABLE_LENGTH - 1;
  df2 = i2 <= 1 ? u2 * tab[0] : tab[i2 - 1] + (tab[i2] - tab[i2 - 1]) * (u2 - i2);
  return df2 - df1;
}
double get_gravkick_factor(int time0, int time1) { return lookup(GravKickTab, time0, time1); }
double get_hydrokick_factor(int time0, int time1) { return lookup(HydroKickTab, time0, time1); }
double dmax(double x, double y) { return x > y ? x : y; }
double second(void) { return 0; }
double timediff(double t0, double t1) { return t1 - t0; }
void endrun(int ierr) { fprintf(stderr, "endrun(%d)\n", ierr); exit(10); }
void distribute_file(int nfiles, int firstfile, int firsttask, int lasttask, int *filenr, int *master, int *last)
{
  *filenr = 0; *master = 0; *last = 0;   /* one task, one file */
}
int MPI_Send(const void *buf, int count, MPI_Datatype datatype, int dest, int tag, MPI_Comm comm)
{
  fprintf(stderr, "MPI_Send reached\n"); abort();
}

static void rd(void *p, size_t size, size_t count, FILE *f)
{
  if(fread(p, size, count, f) != count) { fprintf(stderr, "short input\n"); exit(2); }
}

int main(int argc, char **argv)
{
  FILE *f = fopen(argv[1], "rb");
  int head[6], n, i, j, *ty, *tb, *te, *id;
  double par[14], *x;
  if(argc != 3 || !f) return 2;
  rd(head, sizeof(int), 6, f);
  rd(par, sizeof(double), 14, f);
  rd(GravKickTab, sizeof(double), DRIFT_TABLE_LENGTH, f);
  rd(HydroKickTab, sizeof(double), DRIFT_TABLE_LENGTH, f);
  n = head[0];
  memset(&All, 0, sizeof All);
  ThisTask = 0; NTask = 1; NumPart = n;
  All.Ti_Current = head[1]; All.ComovingIntegrationOn = head[4]; All.SnapFormat = head[5];
#ifdef PMGRID
  All.PM_Ti_begstep = head[2]; All.PM_Ti_endstep = head[3];
#endif
  All.Timebase_interval = par[0]; All.TimeBegin = par[1]; All.TimeMax = par[2]; All.BoxSize = par[3]; All.Omega0 = par[4];
  All.OmegaLambda = par[5]; All.HubbleParam = par[6]; All.MinEgySpec = par[7];
  for(i = 0; i < 6; i++) All.MassTable[i] = par[8 + i];
  if(All.ComovingIntegrationOn)
    {
      LogBegin = log(All.TimeBegin); LogMax = log(All.TimeMax);
      All.Time = All.TimeBegin * exp(All.Ti_Current * All.Timebase_interval);
    }
  else
    All.Time = All.TimeBegin + All.Ti_Current * All.Timebase_interval;
  All.NumFilesPerSnapshot = 1; All.NumFilesWrittenInParallel = 1; All.BufferSize = 1;
  strcpy(All.OutputDir, argv[2]); strcpy(All.SnapshotFileBase, "snap");
  CommBuffer = malloc(1024 * 1024);
  P = malloc(sizeof(struct particle_data) * n);
  SphP = malloc(sizeof(struct sph_particle_data) * n);   /* the rows of type 0 come first: SphP[i] belongs to P[i] there */
  memset(P, 0, sizeof(struct particle_data) * n);
  memset(SphP, 0, sizeof(struct sph_particle_data) * n);
  ty = malloc(sizeof(int) * n); tb = malloc(sizeof(int) * n); te = malloc(sizeof(int) * n); id = malloc(sizeof(int) * n);
  x = malloc(sizeof(double) * 3 * n);
  rd(ty, sizeof(int), n, f); rd(tb, sizeof(int), n, f); rd(te, sizeof(int), n, f); rd(id, sizeof(int), n, f);
  for(i = 0; i < n; i++) { P[i].Type = ty[i]; P[i].Ti_begstep = tb[i]; P[i].Ti_endstep = te[i]; P[i].ID = id[i]; }
  for(i = 1; i < n; i++) if(ty[i] == 0 && ty[i - 1] != 0) { fprintf(stderr, "gas must come first\n"); return 2; }
#define VEC(field) rd(x, sizeof(double), 3 * n, f); for(i = 0; i < n; i++) for(j = 0; j < 3; j++) field[j] = x[3 * i + j];
#define SKIP3 rd(x, sizeof(double), 3 * n, f);
#define SCA(field) rd(x, sizeof(double), n, f); for(i = 0; i < n; i++) field = x[i];
  VEC(P[i].Pos) VEC(P[i].Vel) SCA(P[i].Mass) VEC(P[i].GravAccel)
#ifdef PMGRID
  VEC(P[i].GravPM)
#else
  SKIP3
#endif
  VEC(SphP[i].HydroAccel) SCA(SphP[i].Entropy) SCA(SphP[i].DtEntropy) SCA(SphP[i].Density) SCA(SphP[i].Hsml) SCA(P[i].Potential)
  fclose(f);
  savepositions(0);
  return 0;
}
"""

# find_next_outputtime of run.c: what run.c does not find when it is linked alone is never reached from that function
NEXT_DRIVER = r"""
/* driver of tests/golden/make_snapshot_golden.py: in = ncase, then per case ComovingIntegrationOn, OutputListOn, OutputListLength,
 * ti_curr (int), Timebase_interval, TimeBegin, TimeMax, TimeOfFirstSnapshot, TimeBetSnapshot (double), the list (double
 * [OutputListLength]); out = ti_next (int [ncase]) */
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include "allvars.h"
#include "proto.h"
int main(int argc, char **argv)
{
  FILE *f = fopen(argv[1], "rb"), *g = fopen(argv[2], "wb");
  int ncase, k, head[4], out;
  double par[5];
  if(argc != 3 || !f || !g || fread(&ncase, sizeof(int), 1, f) != 1) return 2;
  ThisTask = 1;   /* (not the task that prints) */
  for(k = 0; k < ncase; k++)
    {
      if(fread(head, sizeof(int), 4, f) != 4 || fread(par, sizeof(double), 5, f) != 5) return 2;
      memset(&All, 0, sizeof All);
      All.ComovingIntegrationOn = head[0]; All.OutputListOn = head[1]; All.OutputListLength = head[2];
      All.Timebase_interval = par[0]; All.TimeBegin = par[1]; All.TimeMax = par[2]; All.TimeOfFirstSnapshot = par[3]; All.TimeBetSnapshot = par[4];
      if(head[2] > 0 && fread(All.OutputListTimes, sizeof(double), head[2], f) != (size_t) head[2]) return 2;
      out = find_next_outputtime(head[3]);
      fwrite(&out, sizeof(int), 1, g);
    }
  fclose(g);
  return 0;
}
"""


def build(tmp, name, flags):
    exe = os.path.join(tmp, "ref_snapshot_" + name)
    stubs = os.path.join(ROOT, "oracle", "ref_stubs")
    # (the stand-ins hold aborting my_fwrite / my_fread for the units that do no I/O; io.c brings its own: theirs get other names)
    stub_o = os.path.join(tmp, "ref_stubs_" + name + ".o")
    subprocess.check_call(["gcc"] + CFLAGS + flags + ["-Dmy_fwrite=stub_my_fwrite", "-Dmy_fread=stub_my_fread", "-I" + stubs, "-I" + REFERENCE, "-c",
                                                      "-o", stub_o, os.path.join(stubs, "ref_stubs.c")])
    cmd = ["gcc"] + CFLAGS + flags + ["-I" + stubs, "-I" + REFERENCE, "-o", exe, os.path.join(tmp, "driver.c"), stub_o,
                                     os.path.join(REFERENCE, "io.c"), os.path.join(REFERENCE, "allvars.c"), "-lm"]
    subprocess.check_call(cmd)
    return exe


def run(exe, tmp, c, P, snap_format, pm_ti):
    src, out = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out") + os.sep
    os.makedirs(out, exist_ok=True)
    tabs = P["tables"] if P["comoving"] else (np.zeros(T.LEN),) * 3
    with open(src, "wb") as f:
        f.write(np.array([len(c["type"]), S.TI, pm_ti[0], pm_ti[1], P["comoving"], snap_format], dtype=np.int32).tobytes())
        f.write(np.array([P["timebase_interval"], P["time_begin"], P["time_max"], S.BOX, P["omega0"], P["omega_lambda"], S.HUBBLE_PARAM,
                          P["min_egy_spec"]] + list(S.MASS_TABLE), dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(tabs[1], dtype=np.float64).tobytes())
        f.write(np.ascontiguousarray(tabs[2], dtype=np.float64).tobytes())
        for k in ("type", "ti_begstep", "ti_endstep", "ids"):
            f.write(np.ascontiguousarray(c[k], dtype=np.int32).tobytes())
        for k in DOUBLES:
            f.write(np.nan_to_num(np.ascontiguousarray(c[k], dtype=np.float64)).tobytes())
    subprocess.check_call([exe, src, out], timeout=60, stdout=subprocess.DEVNULL)
    with open(os.path.join(out, "snap_000"), "rb") as f:
        return f.read()


def run_next(tmp):
    """the reference's find_next_outputtime for next_cases(), or None where run.c does not link alone"""
    stubs = os.path.join(ROOT, "oracle", "ref_stubs")
    with open(os.path.join(tmp, "next_driver.c"), "w") as f:
        f.write(NEXT_DRIVER)
    exe = os.path.join(tmp, "ref_next")
    # --unresolved-symbols: the stations of the main loop that run.c calls are not reached from find_next_outputtime
    cmd = ["gcc"] + CFLAGS + ["-I" + stubs, "-I" + REFERENCE, "-o", exe, os.path.join(tmp, "next_driver.c"), os.path.join(stubs, "ref_stubs.c"),
                              os.path.join(REFERENCE, "run.c"), os.path.join(REFERENCE, "allvars.c"), "-lm", "-Wl,--unresolved-symbols=ignore-all"]
    if subprocess.call(cmd, stderr=subprocess.DEVNULL) != 0:
        return None
    cases = S.next_cases()
    src, dst = os.path.join(tmp, "next_in.bin"), os.path.join(tmp, "next_out.bin")
    with open(src, "wb") as f:
        f.write(np.int32(len(cases)).tobytes())
        for P, ti, lst, first, bet in cases:
            f.write(np.array([P["comoving"], lst is not None, len(lst or []), ti], dtype=np.int32).tobytes())
            f.write(np.array([P["timebase_interval"], P["time_begin"], P["time_max"], first, bet], dtype=np.float64).tobytes())
            if lst:
                f.write(np.array(lst, dtype=np.float64).tobytes())
    if subprocess.call([exe, src, dst], timeout=60) != 0:
        return None
    return np.fromfile(dst, dtype=np.int32)


def main():
    if not os.path.exists(os.path.join(REFERENCE, "io.c")):
        sys.exit("the reference tree is not at %s" % REFERENCE)
    c = S.golden_set()
    z = dict(variants=np.array(list(S.VARIANTS)))
    for k in S.COLS + ("ids", "potential"):
        z["in_" + k] = c[k]
    npart = np.bincount(c["type"], minlength=6)
    with tempfile.TemporaryDirectory() as tmp:
        with open(os.path.join(tmp, "driver.c"), "w") as f:
            f.write(DRIVER)
        for name, (flags, fmt, comoving, mesh, periodic, mask, gamma) in S.VARIANTS.items():
            P = S.variant_params(name)
            raw = run(build(tmp, name, flags), tmp, c, P, fmt, S.PM_TI if mesh else (0, 0))
            want = S.file_bytes(c, P, S.TI, mask, fmt, mesh, S.PM_TI, periodic)
            hdr, ref = S.split_file(raw, mask, fmt, npart, S.MASS_TABLE)
            hdr2, mine = S.split_file(want, mask, fmt, npart, S.MASS_TABLE)
            bad = [b for b in ref if ref[b] != mine[b]]
            nu = S.assert_u_close(mine["U"], ref["U"], name) if "U" in bad else 0
            print("%-14s %6d bytes, blocks %s; the restatement differs in %s (U: %d values)" % (name, len(raw), " ".join(ref), bad or "none", nu))
            assert hdr == hdr2 and [b for b in bad if b != "U"] == [] and (raw == want or "U" in bad)
            z[name + "_file"] = np.frombuffer(raw, dtype=np.uint8)
        got = run_next(tmp)
    if got is None:
        print("find_next_outputtime: run.c does not link alone here; the numpy restatement is the only truth for that function")
    else:
        cases = S.next_cases()
        want = np.array([S.find_next_outputtime(P, ti, lst, first, bet) for P, ti, lst, first, bet in cases], dtype=np.int32)
        print("find_next_outputtime: %d cases, the restatement differs in %d" % (len(cases), (got != want).sum()))
        z["next_ti"] = got
    path = os.path.join(ROOT, "tests", "golden", "snapshot_reference.npz")
    np.savez_compressed(path, **z)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
