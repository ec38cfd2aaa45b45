"""The numpy restatement of the reference's output station: fill_write_buffer (io.c:129-357), the header (io.c:720-761), the framing
of write_file (io.c:796-844, 965-969) and find_next_outputtime (run.c:244-361); and the input set of the golden files.  Rounding
goes through np.float32 where the reference assigns to its float buffer.  Shared by tests/test_snapshot.py and
tests/golden/make_snapshot_golden.py."""
import math
import struct

import numpy as np

import test_time_integration as T

BLOCKS = ("POS", "VEL", "ID", "MASS", "U", "RHO", "HSML", "POT", "ACCE", "ENDT", "TSTP")
LABELS = ("POS ", "VEL ", "ID  ", "MASS", "U   ", "RHO ", "HSML", "POT ", "ACCE", "ENDT", "TSTP")
VECTOR = ("POS", "VEL", "ACCE")
GAS = ("U", "RHO", "HSML", "ENDT")
ALWAYS = 0x7F
ALL_BLOCKS = 0x7FF
BOX = T.BOX
TI = T.TI
PM_TI = (T.TI - (1 << 20), T.TI + (1 << 18))     # a PM step whose middle is not Ti_Current
MASS_TABLE = np.array([0.0, 1.25, 0.0, 0.0, 0.5, 0.0])
HUBBLE_PARAM = 0.7
COLS = ("type", "pos", "vel", "mass", "ti_begstep", "ti_endstep", "grav_accel", "grav_pm", "hydro_accel", "entropy", "dt_entropy", "density", "hsml")

f32 = np.float32


def make_set(n, seed, P, gas_frac=0.4, gas_first=True, types=None):
    """T.make_set's columns with the rows of type 0 in front (SphP[] is indexed like P[] only there), a seeded id and potential
    column, and in the first rows of type 1 the four positions on which the float wrap of io.c:198-201 turns"""
    c = T.make_set(n, seed, P, True)
    rng = np.random.default_rng(seed + 7)
    ty = c["type"].copy()
    if types is not None:
        ty = np.asarray(types, dtype=np.int32)
    elif gas_frac == 0:
        ty = np.where(ty == 0, 1 + (np.arange(n) % 5), ty).astype(np.int32)
    if gas_first:
        ty = np.concatenate([ty[ty == 0], ty[ty != 0]]).astype(np.int32)
    c["type"] = ty
    gas = ty == 0
    for k in T.GASF:   # the gas columns hold numbers where there is gas, NaN elsewhere
        col = c[k]
        fill = np.abs(rng.normal(1.0, 0.1, col.shape)) if k not in ("vel_pred", "hydro_accel", "dt_entropy", "div_vel") else rng.normal(0, 0.1, col.shape)
        col[gas & np.isnan(col.reshape(n, -1)[:, 0])] = fill[gas & np.isnan(col.reshape(n, -1)[:, 0])]
        col[~gas] = np.nan
    c["ids"] = rng.permutation(n).astype(np.int32) + 1
    c["potential"] = -np.abs(rng.normal(50.0, 20.0, n))
    edge = np.array([-1e-9, BOX * (1 - 1e-12), 1.5 * BOX, -0.25 * BOX])
    rows = np.flatnonzero(ty != 0)[:4] if (ty != 0).sum() >= 4 else np.arange(min(n, 4))
    for r, x in zip(rows, edge):
        c["pos"][r, 0] = x
        c["pos"][r, 2] = x
    return c


# ---- fill_write_buffer ---------------------------------------------------------------------------------------------------------------
def file_order(ptype):
    return np.argsort(ptype, kind="stable")


def block_rows(block, ptype, mass_table):
    """the rows of a block in the file order (get_particles_in_block, io.c:465-523)"""
    order = file_order(ptype)
    t = ptype[order]
    if block == "MASS":
        return order[np.asarray(mass_table)[t] == 0]
    if block in GAS:
        return order[t == 0]
    return order


def kick_factors(c, P, ti):
    """io.c:213-228: (dt_gravkick, dt_hydrokick) per row"""
    beg = c["ti_begstep"].astype(np.int64)
    mid = (beg + c["ti_endstep"].astype(np.int64)) // 2
    if P["comoving"]:
        g = T.ref_factor(P["tables"][1], P, beg, ti) - T.ref_factor(P["tables"][1], P, beg, mid)
        h = T.ref_factor(P["tables"][2], P, beg, ti) - T.ref_factor(P["tables"][2], P, beg, mid)
        return g, h
    dt = (ti - mid) * P["timebase_interval"]
    return dt, dt


def time_of(P, ti):
    if P["comoving"]:
        return P["time_begin"] * math.exp(ti * P["timebase_interval"])
    return P["time_begin"] + ti * P["timebase_interval"]


def fill_block(block, c, P, ti, mesh=False, pm_ti=None, periodic=False, box=BOX, mass_table=MASS_TABLE):
    """the block's elements as they lie on disk: float32 ([k, 3] for the vectors), int32 for ID"""
    rows = block_rows(block, c["type"], mass_table)
    if len(rows) == 0:   # (a block without elements is not written, and its columns need not exist)
        return np.zeros((0, 3) if block in VECTOR else 0, dtype=np.int32 if block == "ID" else f32)
    gas = (c["type"][rows] == 0)[:, None]
    a3inv = fac1 = fac2 = 1.0
    if P["comoving"]:
        a = time_of(P, ti)
        a3inv, fac1, fac2 = 1 / (a * a * a), 1 / (a * a), 1 / math.pow(a, 3 * P["gamma"] - 2)
    with np.errstate(invalid="ignore", over="ignore"):
        if block == "POS":
            fp = c["pos"][rows].astype(f32)
            if periodic:
                for _ in range(1100):   # io.c:198-201, on the float
                    lo = fp < 0
                    if not lo.any():
                        break
                    fp = np.where(lo, (fp.astype(np.float64) + box).astype(f32), fp)
                for _ in range(1100):
                    hi = fp >= box
                    if not hi.any():
                        break
                    fp = np.where(hi, (fp.astype(np.float64) - box).astype(f32), fp)
            return fp
        if block == "VEL":
            g, h = kick_factors(c, P, ti)
            g, h = np.broadcast_to(g, c["type"].shape)[rows][:, None], np.broadcast_to(h, c["type"].shape)[rows][:, None]
            fp = (c["vel"][rows] + c["grav_accel"][rows] * g).astype(f32)
            if gas.any():
                fp = np.where(gas, (fp.astype(np.float64) + np.nan_to_num(c["hydro_accel"][rows]) * h).astype(f32), fp)
            if mesh:
                mid = (pm_ti[0] + pm_ti[1]) // 2
                if P["comoving"]:
                    dt_pm = float(T.ref_factor(P["tables"][1], P, pm_ti[0], ti) - T.ref_factor(P["tables"][1], P, pm_ti[0], mid))
                else:
                    dt_pm = (ti - mid) * P["timebase_interval"]
                fp = (fp.astype(np.float64) + c["grav_pm"][rows] * dt_pm).astype(f32)
            return (fp.astype(np.float64) * math.sqrt(a3inv)).astype(f32)
        if block == "ID":
            return c["ids"][rows].astype(np.int32)
        if block == "MASS":
            return c["mass"][rows].astype(f32)
        if block == "U":
            if P["gamma"] == 1:
                return c["entropy"][rows].astype(f32)
            gm1 = P["gamma"] - 1
            u = c["entropy"][rows] / gm1 * np.power(c["density"][rows] * a3inv, gm1)
            return np.where(P["min_egy_spec"] > u, P["min_egy_spec"], u).astype(f32)
        if block in ("RHO", "HSML", "ENDT"):
            return c[dict(RHO="density", HSML="hsml", ENDT="dt_entropy")[block]][rows].astype(f32)
        if block == "POT":
            return c["potential"][rows].astype(f32)
        if block == "ACCE":
            fp = (fac1 * c["grav_accel"][rows]).astype(f32)
            if mesh:
                fp = (fp.astype(np.float64) + fac1 * c["grav_pm"][rows]).astype(f32)
            if not gas.any():
                return fp
            return np.where(gas, (fp.astype(np.float64) + fac2 * np.nan_to_num(c["hydro_accel"][rows])).astype(f32), fp)
        if block == "TSTP":
            return ((c["ti_endstep"][rows].astype(np.int64) - c["ti_begstep"][rows]) * P["timebase_interval"]).astype(f32)
    raise KeyError(block)


# ---- the header and the framing ------------------------------------------------------------------------------------------------------
def header(npart, mass_table, time, comoving, box, omega0, omega_lambda, hubble_param, npart_total=None, num_files=1):
    tot = np.asarray(npart if npart_total is None else npart_total, dtype=np.int64)
    h = struct.pack("<6i6d2d2i6I2i4d2i6Ii", *[int(x) for x in npart], *[float(x) for x in mass_table], time, 1.0 / time - 1 if comoving else 0.0,
                    0, 0, *[int(x) & 0xFFFFFFFF for x in tot], 0, num_files, box, omega0, omega_lambda, hubble_param, 0, 0,
                    *[int(x) >> 32 for x in tot], 0)
    return h + bytes(256 - len(h))


def _rec(body):
    return struct.pack("<i", len(body)) + body + struct.pack("<i", len(body))


def block_present(mask):
    return [b for i, b in enumerate(BLOCKS) if ((mask | ALWAYS) >> i) & 1]


def file_bytes(c, P, ti, mask=ALWAYS, snap_format=1, mesh=False, pm_ti=None, periodic=False, box=BOX, mass_table=MASS_TABLE,
               hubble_param=HUBBLE_PARAM, header_box=None, blocks=None):
    """the whole file of savepositions() for one task; blocks: ready {label: array} instead of the restatement's"""
    npart = np.bincount(c["type"], minlength=6)
    hb = header(npart, mass_table, time_of(P, ti), P["comoving"], box if header_box is None else header_box, P["omega0"], P["omega_lambda"],
                hubble_param)
    out = b""
    if snap_format == 2:
        out += _rec(b"HEAD" + struct.pack("<i", 256 + 8))
    out += _rec(hb)
    for b in block_present(mask):
        a = blocks[b] if blocks is not None else fill_block(b, c, P, ti, mesh, pm_ti, periodic, box, mass_table)
        if len(a) == 0:
            continue
        body = np.ascontiguousarray(a).tobytes()
        if snap_format == 2:
            out += _rec(LABELS[BLOCKS.index(b)].encode() + struct.pack("<i", len(body) + 8))
        out += _rec(body)
    return out


def split_file(raw, mask, snap_format, npart, mass_table):
    """(header bytes, {label: body bytes}) of a file by position"""
    recs, o = [], 0
    while o < len(raw):
        (k,) = struct.unpack_from("<i", raw, o)
        recs.append(raw[o + 4:o + 4 + k])
        assert struct.unpack_from("<i", raw, o + 4 + k)[0] == k
        o += k + 8
    if snap_format == 2:
        assert recs[0][:4] == b"HEAD"
        labels = [r[:4].decode() for r in recs[2::2]]
        recs = [recs[1]] + recs[3::2]
    else:
        labels = None
    npart, mt = np.asarray(npart), np.asarray(mass_table)
    present = []
    for b in block_present(mask):
        cnt = npart[mt == 0].sum() if b == "MASS" else (npart[0] if b in GAS else npart.sum())
        if cnt > 0:
            present.append(b)
    assert len(present) == len(recs) - 1, (present, len(recs))
    if labels is not None:
        assert labels == [LABELS[BLOCKS.index(b)] for b in present]
    return recs[0], dict(zip(present, recs[1:]))


def assert_u_close(got, want, what=""):
    """the U block: pow() may differ between libraries -- each value the reference's float or an adjacent one, at most 0.1 % of them
    different.  Returns the number of values that differ."""
    got, want = np.frombuffer(got, dtype=f32) if isinstance(got, bytes) else got, np.frombuffer(want, dtype=f32) if isinstance(want, bytes) else want
    assert got.shape == want.shape, what
    diff = got != want
    adjacent = (got == np.nextafter(want, f32(np.inf))) | (got == np.nextafter(want, f32(-np.inf)))
    assert (~diff | adjacent).all(), "%s: U values that are not the reference's float or an adjacent one" % what
    assert diff.sum() <= 0.001 * len(want), "%s: %d of %d U values differ" % (what, diff.sum(), len(want))
    return int(diff.sum())


# ---- find_next_outputtime (run.c:244-361) --------------------------------------------------------------------------------------------
class Fatal(Exception):
    pass


def find_next_outputtime(P, ti_curr, output_list=None, first=0.0, bet=0.0):
    TB = T.TB
    ti_next = -1

    def to_ti(time):
        x = math.log(time / P["time_begin"]) / P["timebase_interval"] if P["comoving"] else (time - P["time_begin"]) / P["timebase_interval"]
        return int(x)   # C truncation
    if output_list is not None:
        for time in output_list:
            if P["time_begin"] <= time <= P["time_max"]:
                ti = to_ti(time)
                if ti >= ti_curr:
                    if ti_next == -1 or ti_next > ti:
                        ti_next = ti
    else:
        if (P["comoving"] and bet <= 1.0) or (not P["comoving"] and bet <= 0.0):
            raise Fatal(13123)
        time, it = first, 0
        while time < P["time_begin"]:
            time = time * bet if P["comoving"] else time + bet
            it += 1
            if it > 1000000:
                raise Fatal(110)
        while time <= P["time_max"]:
            ti = to_ti(time)
            if ti >= ti_curr:
                ti_next = ti
                break
            time = time * bet if P["comoving"] else time + bet
            it += 1
            if it > 1000000:
                raise Fatal(111)
    return 2 * TB if ti_next == -1 else ti_next


def next_cases():
    """(P, ti_curr, list or None, first, bet) for both branches of find_next_outputtime, comoving and not"""
    cases = []
    TB = T.TB
    for comoving in (False, True):
        P = T.params(comoving)
        span = P["time_max"] / P["time_begin"] if comoving else P["time_max"] - P["time_begin"]
        lst = [P["time_begin"] * span ** q if comoving else P["time_begin"] + span * q for q in (0.9, 0.1, 0.5, 0.1000001, 1.0, 1.2, 0.0)]
        for ti in (0, 1, TB // 10, TB // 10 + 1, TB // 2, TB // 2 + 1, TB - 1, TB, TB + 1):
            cases.append((P, ti, lst, 0.0, 0.0))
        first = P["time_begin"] / 3.0 if comoving else P["time_begin"] - 0.33
        bet = span ** 0.07 if comoving else span * 0.07
        for ti in (0, 1, TB // 7, TB // 2, (TB // 100) * 93, TB - 5, TB + 1):
            cases.append((P, ti, None, first, bet))
        cases.append((P, 0, None, P["time_max"] * 2, bet))   # no time at all
    return cases


# ---- the golden variants -------------------------------------------------------------------------------------------------------------
GOLDEN_N = 600
GOLDEN_SEED = 4242
# name: (compile switches, snap_format, comoving, mesh, periodic, mask, gamma)
VARIANTS = {
    "stock_f1": ([], 1, False, False, False, ALWAYS, T.GAMMA),
    "stock_f2": ([], 2, False, False, False, ALWAYS, T.GAMMA),
    "full": (["-DPERIODIC", "-DPMGRID=16", "-DOUTPUTACCELERATION", "-DOUTPUTCHANGEOFENTROPY", "-DOUTPUTTIMESTEP", "-DOUTPUTPOTENTIAL"], 2,
             False, True, True, ALL_BLOCKS, T.GAMMA),
    "full_comoving": (["-DPERIODIC", "-DPMGRID=16", "-DOUTPUTACCELERATION", "-DOUTPUTCHANGEOFENTROPY", "-DOUTPUTTIMESTEP", "-DOUTPUTPOTENTIAL"], 1,
                      True, True, True, ALL_BLOCKS, T.GAMMA),
    "isotherm": (["-DISOTHERM_EQS"], 1, False, False, False, ALWAYS, 1.0),
}
MIN_EGY_SPEC = 0.9   # a floor that some rows of the set reach


def variant_params(name):
    _, _, comoving, _, _, _, gamma = VARIANTS[name]
    return T.params(comoving, gamma=gamma, min_egy_spec=MIN_EGY_SPEC)


def golden_set():
    """one input set for every variant (the columns do not depend on the variant's parameters: T.params(False) scales them)"""
    return make_set(GOLDEN_N, GOLDEN_SEED, T.params(False))
