"""Front end of oracle/_ref/ref_sph_*: the reference's own density() / hydro_force(), single task (tests only).

The executables are built by `make -C oracle ref` from the reference tree (ref_sph_driver.c + ref_stubs/); this module
writes the driver's input file, runs the variant that matches the compile-time switches asked for in a temporary
directory under a time limit, and reads the result back into arrays over ALL rows (rows that are not gas hold 0).
"""
import os
import re
import struct
import subprocess
import tempfile

import numpy as np

REF_DIR = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_ref")
VARIANTS = ("open", "periodic", "periodic_isotherm", "periodic_nolimiter")
MAKE_TARGET = "make -C oracle ref"
# order of the arrays in the driver's output file
OUT_NAMES = ("hsml", "density", "num_ngb", "div_vel", "curl_vel", "dhsml_factor", "pressure", "hydro_accel_x", "hydro_accel_y",
             "hydro_accel_z", "dt_entropy", "max_signal_vel", "ti_begstep", "ti_endstep")
TI_CURRENT = 1 << 20          # any point of the integer timeline with room for the steps below it


class RefSphError(RuntimeError):
    pass


def exe(variant):
    return os.path.join(REF_DIR, "ref_sph_" + variant)


def available():
    return all(os.access(exe(v), os.X_OK) for v in VARIANTS)


def variant_for(box, gamma=5.0 / 3, limiter=True):
    """the executable whose compile-time switches are (PERIODIC, ISOTHERM_EQS, NOVISCOSITYLIMITER) as asked"""
    iso = gamma == 1.0
    if not iso and abs(gamma - 5.0 / 3) > 1e-15:
        raise RefSphError("the reference knows GAMMA = 5/3 and, with ISOTHERM_EQS, 1")
    if not box:
        if iso or not limiter:
            raise RefSphError("only the periodic build exists with ISOTHERM_EQS / NOVISCOSITYLIMITER")
        return "open"
    if iso and not limiter:
        raise RefSphError("no build with ISOTHERM_EQS and NOVISCOSITYLIMITER together")
    return "periodic_isotherm" if iso else ("periodic" if limiter else "periodic_nolimiter")


def run(pos, mass, ptype, vel, hsml, *, box=0.0, des=50.0, dev=1.0, min_gas_hsml=0.0, visc=0.8, timestep=None, tbi=0.0, active=None,
        entropy=None, columns=None, gamma=5.0 / 3, limiter=True, comoving=None, softening=0.01, timeout=60.0, buffer_mb=16,
        part_alloc_factor=1.5, tree_alloc_factor=1.5):
    """density() then hydro_force() (columns=None), or hydro_force() alone on the SphP `columns` (dict of density, pressure,
    dhsml_factor, div_vel, curl_vel over all rows; `hsml` is SphP.Hsml either way).  entropy: SphP.Entropy over all rows (the
    reference's pressure line is Entropy * Density^GAMMA; SphP.DtEntropy starts at 0).  timestep: Ti_endstep - Ti_begstep per row;
    active: rows with Ti_endstep == Ti_Current (default all).  comoving: (Time, Omega0, OmegaLambda, Hubble) or None.
    Returns a dict of arrays over all rows (OUT_NAMES, hydro_accel [n, 3]) plus "passes" (passes of density()'s outer loop,
    counted from the reference's own progress lines), "seconds" and "stdout"."""
    import time
    n = len(pos)
    variant = variant_for(box, gamma, limiter)
    if not os.access(exe(variant), os.X_OK):
        raise RefSphError("%s is missing: %s" % (exe(variant), MAKE_TARGET))
    f64 = lambda a, shape: np.ascontiguousarray(np.broadcast_to(np.asarray(a, dtype=np.float64), shape))   # noqa: E731
    gas = np.asarray(ptype) == 0
    clean = lambda a: np.where(gas, f64(a, (n,)), 0.0)                                                     # noqa: E731
    ts = np.zeros(n, dtype=np.int64) if timestep is None else np.asarray(timestep, dtype=np.int64)
    act = np.ones(n, dtype=bool) if active is None else np.asarray(active) != 0
    ts = np.where(gas, ts, 0)
    if ts.min() < 0 or ts.max() >= TI_CURRENT // 2:
        raise RefSphError("timestep outside the timeline")
    end = np.where(act, TI_CURRENT, TI_CURRENT + 16 + ts).astype(np.int32)      # inactive: any Ti_endstep != Ti_Current
    beg = (end - ts).astype(np.int32)
    time_, omega0, omega_lambda, hubble = comoving if comoving is not None else (1.0, 0.0, 0.0, 0.0)
    head = struct.pack("=8s5i13d", b"NGSPHIN1", 0 if columns is None else 1, n, int(comoving is not None), TI_CURRENT, int(buffer_mb),
                       float(box), float(des), float(dev), float(min_gas_hsml), float(visc), float(tbi), float(time_), float(omega0),
                       float(omega_lambda), float(hubble), float(part_alloc_factor), float(tree_alloc_factor), float(softening))
    parts = [f64(pos, (n, 3)), f64(mass, (n,)), np.ascontiguousarray(ptype, dtype=np.int32), np.where(gas[:, None], f64(vel, (n, 3)), 0.0),
             clean(hsml), clean(np.zeros(n) if entropy is None else entropy), beg, end]
    if columns is not None:
        parts += [clean(columns[k]) for k in ("density", "pressure", "dhsml_factor", "div_vel", "curl_vel")]
    with tempfile.TemporaryDirectory(prefix="ref_sph_") as tmp:
        fin, fout = os.path.join(tmp, "in.bin"), os.path.join(tmp, "out.bin")
        with open(fin, "wb") as f:
            f.write(head)
            for a in parts:
                f.write(np.ascontiguousarray(a).tobytes())
        t0 = time.time()
        try:
            p = subprocess.run([exe(variant), fin, fout], cwd=tmp, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, timeout=timeout)
        except subprocess.TimeoutExpired as e:
            raise RefSphError("ref_sph_%s ran into its time limit of %g s\n%s" % (variant, timeout, (e.stdout or b"").decode(errors="replace")[-4000:]))
        seconds = time.time() - t0
        text = p.stdout.decode(errors="replace")
        if p.returncode != 0:
            raise RefSphError("ref_sph_%s ended with status %d\n%s" % (variant, p.returncode, text[-4000:]))
        with open(fout, "rb") as f:
            raw = f.read()
    if raw[:8] != b"NGSPHOU1":
        raise RefSphError("not an output file of the driver")
    ngas = struct.unpack_from("=i", raw, 8)[0]
    if ngas != int(gas.sum()) or len(raw) != 12 + 4 * ngas + 8 * ngas * len(OUT_NAMES):
        raise RefSphError("output file of the wrong size")
    rows = np.frombuffer(raw, dtype=np.int32, count=ngas, offset=12)
    if not np.array_equal(np.sort(rows), np.nonzero(gas)[0]):
        raise RefSphError("the rows of the output are not the gas rows of the input")
    cols = np.frombuffer(raw, dtype=np.float64, count=ngas * len(OUT_NAMES), offset=12 + 4 * ngas).reshape(len(OUT_NAMES), ngas)
    out = {}
    for k, c in zip(OUT_NAMES, cols):
        out[k] = np.zeros(n)
        out[k][rows] = c
    out["hydro_accel"] = np.stack([out.pop("hydro_accel_x"), out.pop("hydro_accel_y"), out.pop("hydro_accel_z")], axis=1)
    if not (np.array_equal(out.pop("ti_begstep")[gas], beg[gas]) and np.array_equal(out.pop("ti_endstep")[gas], end[gas])):
        raise RefSphError("the reference did not restore the particles' timeline marks")
    # density() announces every further pass of its outer loop on stdout ("ngb iteration K: ..."): passes = 1 + the last K
    its = [int(m) for m in re.findall(r"^ngb iteration (\d+):", text, flags=re.M)]
    out["passes"] = (1 + max(its, default=0)) if columns is None else 0
    out["seconds"] = seconds
    out["stdout"] = text
    return out
