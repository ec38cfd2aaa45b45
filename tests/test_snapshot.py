"""Snapshot files from the device: the reference's savepositions() (io.c:33-989) and find_next_outputtime() (run.c:244-361).

The truth is the reference's own io.c, byte for byte: tests/golden/snapshot_reference.npz holds one input set and the files that five
builds of io.c wrote for it (tests/golden/make_snapshot_golden.py).  tests/snapshot_ref.py restates fill_write_buffer, the header and
the framing in numpy; it reproduces every golden file, and is the truth at the other sizes and modes.  The U block is the one
exception: pow() may differ between libraries, so each value is the reference's float or an adjacent one and at most 0.1 % differ
(measured on gfx950: 0 of the 246 U values of the golden set differ from the reference's bytes in every variant and layout, and 0 of
105 088 from the restatement's at n = 262 401)."""
import ctypes as C
import functools
import os
import re

import numpy as np
import pytest

import snapshot_ref as S
import test_time_integration as T

HERE = os.path.dirname(os.path.abspath(__file__))
NEW = ["ngravs_snapshot_plan", "ngravs_snapshot_block_count", "ngravs_snapshot_block", "ngravs_snapshot_header", "ngravs_snapshot_write",
       "ngravs_find_next_outputtime"]


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(HERE, "golden", "snapshot_reference.npz"))
    c = {k[3:]: z[k] for k in z.files if k.startswith("in_")}
    files = {str(v): z[str(v) + "_file"].tobytes() for v in z["variants"]}
    return c, files, (z["next_ti"] if "next_ti" in z.files else None)


def npart_of(c):
    return np.bincount(c["type"], minlength=6)


# ---- CPU ------------------------------------------------------------------------------------------------------------------
def test_golden_file_is_small_and_the_set_is_what_the_issue_asks():
    c, files, _ = golden()
    assert os.path.getsize(os.path.join(HERE, "golden", "snapshot_reference.npz")) < 512 * 1024
    assert set(files) == set(S.VARIANTS) and len(c["type"]) == S.GOLDEN_N
    ty = c["type"]
    assert (npart_of(c) > 0).all() and (np.diff((ty != 0).astype(int)) >= 0).all()   # all six types, gas first
    assert (S.MASS_TABLE != 0).sum() == 2
    for x in (-1e-9, S.BOX * (1 - 1e-12), 1.5 * S.BOX, -0.25 * S.BOX):
        assert (c["pos"] == x).any()
    fresh = S.golden_set()   # the maker's set is reproducible
    for k in S.COLS + ("ids", "potential"):
        assert np.array_equal(fresh[k], c[k], equal_nan=True), k


@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_restatement_reproduces_the_reference_files(name):
    c, files, _ = golden()
    flags, fmt, comoving, mesh, periodic, mask, gamma = S.VARIANTS[name]
    P = S.variant_params(name)
    want, got = files[name], S.file_bytes(c, P, S.TI, mask, fmt, mesh, S.PM_TI, periodic)
    hdr_w, ref = S.split_file(want, mask, fmt, npart_of(c), S.MASS_TABLE)
    hdr_g, mine = S.split_file(got, mask, fmt, npart_of(c), S.MASS_TABLE)
    assert hdr_w == hdr_g and list(ref) == list(mine)
    assert list(ref) == [b for b in S.block_present(mask)]
    for b in ref:
        if b == "U":
            print("%s: U values of the restatement that differ from the reference: %d" % (name, S.assert_u_close(mine[b], ref[b], name)))
        else:
            assert mine[b] == ref[b], (name, b)
    if mine["U"] == ref["U"]:
        assert got == want   # framing and label records too


def test_float_wrap_in_the_reference_files():
    """-1e-9 becomes BoxSize in float and wraps to 0; a double just below BoxSize rounds up to it and wraps to 0 too"""
    c, files, _ = golden()
    for name in ("stock_f1", "full"):
        flags, fmt, comoving, mesh, periodic, mask, gamma = S.VARIANTS[name]
        _, ref = S.split_file(files[name], mask, fmt, npart_of(c), S.MASS_TABLE)
        pos = np.frombuffer(ref["POS"], dtype=np.float32).reshape(-1, 3)
        rows = S.block_rows("POS", c["type"], S.MASS_TABLE)
        for x, wrapped in ((-1e-9, 0.0), (S.BOX * (1 - 1e-12), 0.0), (1.5 * S.BOX, 0.5 * S.BOX), (-0.25 * S.BOX, 0.75 * S.BOX)):
            at = np.flatnonzero(c["pos"][rows, 0] == x)
            assert len(at) == 1
            assert pos[at[0], 0] == np.float32(wrapped if periodic else x), (name, x)


def test_header_of_the_library_is_the_reference_header(pkg, have_lib):
    c, files, _ = golden()
    for name, (flags, fmt, comoving, mesh, periodic, mask, gamma) in S.VARIANTS.items():
        P = S.variant_params(name)
        want, _ = S.split_file(files[name], mask, fmt, npart_of(c), S.MASS_TABLE)
        got = pkg.snapshot_header(T.c_params(pkg, P), npart_of(c), S.time_of(P, S.TI), mass_table=S.MASS_TABLE, hubble_param=S.HUBBLE_PARAM,
                                  box_size=S.BOX)
        assert len(got) == 256 and got == want, name
    # the high word of the totals
    P = S.variant_params("stock_f1")
    tot = np.array([5, (7 << 32) + 3, 0, 0, 1 << 33, 0], dtype=np.int64)
    got = pkg.snapshot_header(T.c_params(pkg, P), np.array([5, 3, 0, 0, 2, 0]), 0.25, npart_total=tot, num_files=4)
    assert got == S.header([5, 3, 0, 0, 2, 0], np.zeros(6), 0.25, False, 0.0, P["omega0"], P["omega_lambda"], 0.0, npart_total=tot, num_files=4)
    h = pkg.snapshot.parse_header(got)
    assert list(h["npart_total_high"]) == [0, 7, 0, 0, 2, 0] and h["num_files"] == 4 and h["time"] == 0.25


def lib_next(pkg, P, ti, lst, first, bet):
    rule = pkg.abi.make_output_rule(output_list=lst, time_of_first_snapshot=first, time_bet_snapshot=bet)
    return pkg.find_next_outputtime(T.c_params(pkg, P), rule, ti)


def test_find_next_outputtime(pkg, have_lib):
    cases = S.next_cases()
    want = [S.find_next_outputtime(*k) for k in cases]
    got = [lib_next(pkg, *k) for k in cases]
    assert got == want
    gold = golden()[2]
    assert gold is not None and list(gold) == want   # the reference's own run.c
    assert 2 * T.TB in want and len(set(want)) > 12
    # both branches, comoving and not
    assert {(bool(k[0]["comoving"]), k[2] is None) for k in cases} == {(False, False), (False, True), (True, False), (True, True)}


def test_find_next_outputtime_refuses_the_fatal_cases(pkg, have_lib):
    P, Pc = T.params(False), T.params(True)
    fatal = [(P, 0, None, 0.0, 0.0, 13123), (Pc, 0, None, 0.2, 1.0, 13123), (P, 0, None, -1e9, 1e-3, 110), (P, T.TB, None, 0.0, 1e-9, 111)]
    for Pk, ti, lst, first, bet, code in fatal:
        with pytest.raises(S.Fatal) as e:
            S.find_next_outputtime(Pk, ti, lst, first, bet)
        assert e.value.args == (code,)
        with pytest.raises(pkg.NgravsError) as e:
            lib_next(pkg, Pk, ti, lst, first, bet)
        assert "status -1" in str(e.value) and str(code) in str(e.value)


def test_exported_declared_and_laid_out_as_the_header_says(pkg, have_lib):
    for name in NEW:
        assert name in pkg.EXPORTS and hasattr(have_lib, name), name
    root = pkg.__file__.replace("gadget-2.0.7-ngravs_amd/__init__.py", "")
    hdr = open(root + "include/ngravs_hip.h").read()
    for name in NEW:
        assert "int %s(" % name in hdr
    for cname, cls in (("ngravs_snapshot_t", pkg.abi.Snapshot), ("ngravs_output_rule_t", pkg.abi.OutputRule)):
        body = hdr[:hdr.index("} %s;" % cname)]
        body = re.sub(r"/\*.*?\*/", "", body[body.rindex("typedef struct {") + len("typedef struct {"):], flags=re.S)
        names = [re.search(r"(\w+)(\[\d+\])?\s*$", piece).group(1) for decl in body.split(";") if decl.strip() for piece in decl.split(",")]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert C.sizeof(pkg.abi.Snapshot) == 112 and C.sizeof(pkg.abi.OutputRule) == 32
    capi = open(root + "gadget-2.0.7-ngravs_amd/csrc/capi.hip").read()
    assert "static_assert(sizeof(ngravs_snapshot_t) == 112 && sizeof(ngravs_output_rule_t) == 32" in capi
    enum = re.search(r"enum \{ (NGRAVS_SNAP_POS.*?) \};", hdr, flags=re.S).group(1)
    assert [x.strip() for x in enum.split(",")] == ["NGRAVS_SNAP_" + b for b in pkg.abi.SNAP_BLOCKS] + ["NGRAVS_SNAP_NBLOCKS"]
    assert pkg.abi.SNAP_BLOCKS == S.BLOCKS and pkg.abi.SNAP_LABELS == S.LABELS and pkg.abi.snap_mask("POT", "ACCE", "ENDT", "TSTP") == S.ALL_BLOCKS
    assert have_lib.ngravs_abi_version() == 3
    L = have_lib
    assert L.ngravs_snapshot_plan(None, None, None) == -1
    assert L.ngravs_snapshot_block_count(None, None, 0, None, None) == -1
    assert L.ngravs_snapshot_block(None, None, None, None, 0, 0, 0, None, 0) == -1
    assert L.ngravs_snapshot_header(None, None, None, None, 1, 0.0, None) == -1
    assert L.ngravs_snapshot_write(None, None, None, None, 0, 1, 0, None) == -1
    assert L.ngravs_find_next_outputtime(None, None, 0, None) == -1
    for m in ("snapshot_plan", "snapshot_block", "snapshot_block_count", "snapshot_header", "write_snapshot"):
        assert hasattr(pkg.Engine, m), m
    assert hasattr(pkg.timeline.Timeline, "write_snapshot") and hasattr(pkg.snapshot, "read_blocks")


def test_reader_reads_the_reference_files(pkg):
    """format 2 by label, format 1 by position given the mask"""
    import tempfile
    c, files, _ = golden()
    with tempfile.TemporaryDirectory() as tmp:
        for name, (flags, fmt, comoving, mesh, periodic, mask, gamma) in S.VARIANTS.items():
            path = os.path.join(tmp, name)
            with open(path, "wb") as f:
                f.write(files[name])
            hdr, blocks = pkg.snapshot.read_blocks(path, None if fmt == 2 else mask)
            _, ref = S.split_file(files[name], mask, fmt, npart_of(c), S.MASS_TABLE)
            assert list(blocks) == list(ref) and np.array_equal(hdr["npart"], npart_of(c)) and np.array_equal(hdr["mass"], S.MASS_TABLE)
            assert hdr["box_size"] == S.BOX and hdr["hubble_param"] == S.HUBBLE_PARAM
            for b in ref:
                assert blocks[b].tobytes() == ref[b], (name, b)
                assert blocks[b].shape == ((len(ref[b]) // 12, 3) if b in S.VECTOR else (len(ref[b]) // 4,))
            if fmt == 1 and mask != S.ALWAYS:
                with pytest.raises(ValueError):
                    pkg.snapshot.read_blocks(path)   # by position, the optional blocks must be announced


# ---- GPU ------------------------------------------------------------------------------------------------------------------
def engine(pkg, mesh, periodic):
    cfg = pkg.make_config(n_gravs=1, periodic=int(periodic), pmgrid=16 if mesh else 0, box_size=S.BOX, G=1.0, softening=list(T.SOFT))
    return pkg.Engine(cfg)


def to_device(c):
    import torch
    return {k: torch.from_numpy(np.ascontiguousarray(v)).cuda() for k, v in c.items()}


def time_cols(c):
    return {k: c[k] for k in S.COLS}


def interleaved(pkg, c):
    """P[] and SphP[] as one array of structs: (abi.TimeCols, ids, potential, the record array that keeps them alive)"""
    n = len(c["type"])
    keys = S.COLS + ("ids", "potential")
    fields = [(k, np.int32 if c[k].dtype == np.int32 else np.float64, (3,) if c[k].ndim == 2 else ()) for k in keys]
    rec = np.zeros(n, dtype=np.dtype([("pad0", np.float64)] + fields + [("pad1", np.int32, (3,))], align=True))
    for k in keys:
        rec[k] = c[k]
    tc = pkg.abi.TimeCols()
    for k in S.COLS:
        setattr(tc, k, rec.ctypes.data + rec.dtype.fields[k][1])
        setattr(tc, k + "_stride", rec.dtype.itemsize)
    tc.n = n
    assert rec.dtype.itemsize not in (4, 8, 24)
    at = lambda k: (rec.ctypes.data + rec.dtype.fields[k][1], rec.dtype.itemsize)   # noqa: E731
    return tc, at("ids"), at("potential"), rec


def write(pkg, eng, path, c, P, layout="host", mask=S.ALWAYS, fmt=1, mesh=False, mass_table=S.MASS_TABLE, potential=True, **kw):
    par = T.c_params(pkg, P)
    keep = None
    if layout == "interleaved":
        cols, ids, pot, keep = interleaved(pkg, c)
    else:
        d = to_device(c) if layout == "device" else c
        cols, ids, pot = time_cols(d), d["ids"], d["potential"]
    eng.write_snapshot(path, cols, par, S.TI, pm_ti=S.PM_TI if mesh else None, mass_table=mass_table, ids=ids,
                       potential=pot if potential else None, blocks_mask=mask, snap_format=fmt, hubble_param=S.HUBBLE_PARAM, **kw)
    del keep
    with open(path, "rb") as f:
        return f.read()


def assert_same_file(got, want, c, mask, fmt, mass_table, what):
    """every block's bytes; U by the condition of the module's docstring.  Returns the number of adjacent U values."""
    hdr_w, ref = S.split_file(want, mask, fmt, npart_of(c), mass_table)
    hdr_g, mine = S.split_file(got, mask, fmt, npart_of(c), mass_table)
    assert hdr_g == hdr_w, what
    assert list(mine) == list(ref), what
    nu = 0
    for b in ref:
        if b == "U":
            nu = S.assert_u_close(mine[b], ref[b], what)
            print("%s: U values that are adjacent to the reference's: %d of %d" % (what, nu, len(ref[b]) // 4))
        else:
            assert mine[b] == ref[b], (what, b)
    if nu == 0:
        assert got == want, what
    return nu


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["all_one", "two_missing", "alternating", "mixed"])
def test_plan_is_the_stable_partition(pkg, layout):
    import torch
    eng = engine(pkg, False, False)
    par = T.c_params(pkg, T.params(False))
    for n in (1, 63, 64, 65, 255, 257, 1037, 262401):
        rng = np.random.default_rng(n)
        if layout == "all_one":
            ty = np.full(n, 3)
        elif layout == "two_missing":
            ty = rng.choice([0, 1, 3, 5], n)
        elif layout == "alternating":
            ty = np.arange(n) % 6
        else:
            ty = rng.integers(0, 6, n)
        ty = ty.astype(np.int32)
        want = np.argsort(ty, kind="stable").astype(np.int32)
        for dev in (False, True):
            col = torch.from_numpy(ty).cuda() if dev else ty
            npart = eng.snapshot_plan(dict(type=col))
            assert np.array_equal(npart, np.bincount(ty, minlength=6)), (n, dev)
            # (the order is the context's: read through the ID block, with the row numbers as ids)
            ids = np.arange(n, dtype=np.int32)
            ids = torch.from_numpy(ids).cuda() if dev else ids
            for _ in range(2):   # the same permutation on a second call
                got = eng.snapshot_block(pkg.abi.SNAP_ID, dict(type=col), par, S.TI, ids=ids)
                assert np.array_equal(got.cpu().numpy() if dev else got, want), (n, dev, layout)
                assert np.array_equal(eng.snapshot_plan(dict(type=col)), npart)


@pytest.mark.gpu
@pytest.mark.parametrize("layout", ["host", "device", "interleaved"])
@pytest.mark.parametrize("name", list(S.VARIANTS))
def test_write_snapshot_gives_the_reference_files(pkg, tmp_path, name, layout):
    c, files, _ = golden()
    flags, fmt, comoving, mesh, periodic, mask, gamma = S.VARIANTS[name]
    P = S.variant_params(name)
    eng = engine(pkg, mesh, periodic)
    got = write(pkg, eng, str(tmp_path / "snap_000"), c, P, layout, mask, fmt, mesh)
    assert_same_file(got, files[name], c, mask, fmt, S.MASS_TABLE, "%s %s" % (name, layout))


@functools.lru_cache(maxsize=None)
def sized_set(n, gas):
    return S.make_set(n, 900 + n, T.params(False), gas_frac=0.4 if gas else 0.0)


MASS_TABLES = {"zero": np.zeros(6), "all": np.array([1.0, 2.0, 3.0, 4.0, 5.0, 6.0]), "mixed": S.MASS_TABLE}


@pytest.mark.gpu
@pytest.mark.parametrize("comoving,mesh", T.MODES)
@pytest.mark.parametrize("n", [1, 65, 1037, 262401])
def test_write_snapshot_against_the_restatement(pkg, tmp_path, n, comoving, mesh):
    """the four (comoving, mesh) modes at every size, with and without gas, the three kinds of mass table"""
    P = T.params(comoving, min_egy_spec=S.MIN_EGY_SPEC)
    eng = engine(pkg, mesh, True)
    k = 0
    for gas in (True, False):
        c = sized_set(n, gas)
        assert ((c["type"] == 0).sum() > 0) == (gas and n > 1) or n == 1
        for mt_name in (("zero", "all", "mixed") if n <= 1037 else ("mixed",)):
            mt = MASS_TABLES[mt_name]
            fmt = 1 + (k % 2)
            k += 1
            want = S.file_bytes(c, P, S.TI, S.ALL_BLOCKS, fmt, mesh, S.PM_TI, True, mass_table=mt)
            got = write(pkg, eng, str(tmp_path / "snap"), c, P, "device" if n > 1037 else "host", S.ALL_BLOCKS, fmt, mesh, mass_table=mt)
            assert_same_file(got, want, c, S.ALL_BLOCKS, fmt, mt, "n=%d comoving=%d mesh=%d gas=%d %s" % (n, comoving, mesh, gas, mt_name))
            _, blocks = S.split_file(got, S.ALL_BLOCKS, fmt, npart_of(c), mt)
            assert ("MASS" in blocks) == (npart_of(c)[mt == 0].sum() > 0) and ("U" in blocks) == (npart_of(c)[0] > 0)


@pytest.mark.gpu
def test_ranges_and_bounded_buffer(pkg, tmp_path):
    c, files, _ = golden()
    name = "full_comoving"
    flags, fmt, comoving, mesh, periodic, mask, gamma = S.VARIANTS[name]
    P = S.variant_params(name)
    par = T.c_params(pkg, P)
    eng = engine(pkg, mesh, periodic)
    _, ref = S.split_file(files[name], mask, fmt, npart_of(c), S.MASS_TABLE)
    off = np.concatenate([[0], np.cumsum(npart_of(c))])
    for dev in (False, True):
        d = to_device(c) if dev else c
        kw = dict(pm_ti=S.PM_TI, mass_table=S.MASS_TABLE, ids=d["ids"], potential=d["potential"])
        eng.snapshot_plan(time_cols(d))
        back = (lambda a: a.cpu().numpy()) if dev else (lambda a: a)
        for b, label in enumerate(S.BLOCKS):
            total, bpe = eng.snapshot_block_count(b, S.MASS_TABLE)
            assert total * bpe == len(ref[label]) and bpe == (12 if label in S.VECTOR else 4)
            whole = back(eng.snapshot_block(b, time_cols(d), par, S.TI, **kw))
            if label == "U":
                S.assert_u_close(whole, np.frombuffer(ref[label], dtype=np.float32), label)
            else:
                assert whole.tobytes() == ref[label], label
            # chunks of 100 elements (they end inside types, and away from multiples of four)
            parts = [back(eng.snapshot_block(b, time_cols(d), par, S.TI, first=f, count=min(100, total - f), **kw)) for f in range(0, total, 100)]
            assert np.concatenate(parts).tobytes() == whole.tobytes(), label
            # a range that straddles a type boundary, one element, no element
            edge = int(off[2]) if label not in S.GAS and label != "MASS" else total // 2
            for first, count in ((edge - 3, 7), (edge - 1, 1), (total - 1, 1), (5, 0), (total, 0)):
                got = back(eng.snapshot_block(b, time_cols(d), par, S.TI, first=first, count=count, **kw))
                assert got.tobytes() == whole[first:first + count].tobytes(), (label, first, count)
    # a file written through a buffer of 1200 bytes equals the one written with the default
    a = write(pkg, eng, str(tmp_path / "a"), c, P, "host", mask, fmt, mesh)
    b = write(pkg, eng, str(tmp_path / "b"), c, P, "host", mask, fmt, mesh, buffer_bytes=1200)
    assert a == b and len(a) == len(files[name])


@pytest.mark.gpu
def test_float_wrap(pkg):
    P = T.params(False)
    par = T.c_params(pkg, P)
    edge = np.array([-1e-9, S.BOX * (1 - 1e-12), 1.5 * S.BOX, -0.25 * S.BOX, 0.0, S.BOX, -S.BOX, 1023.5 * S.BOX, -1023.5 * S.BOX, 3.0])
    pos = np.stack([edge, edge[::-1], np.full(len(edge), 7.25)], axis=1)
    ty = np.ones(len(edge), dtype=np.int32)
    c = dict(type=ty, pos=pos)
    for periodic in (True, False):
        eng = engine(pkg, False, periodic)
        eng.snapshot_plan(c)
        got = eng.snapshot_block(pkg.abi.SNAP_POS, c, par, S.TI)
        want = S.fill_block("POS", c, P, S.TI, periodic=periodic)
        assert got.tobytes() == want.tobytes(), periodic
        if periodic:
            assert list(got[:4, 0]) == [0.0, 0.0, 50.0, 75.0] and (got >= 0).all() and (got < S.BOX).all()
        else:
            assert np.array_equal(got, pos.astype(np.float32))


@pytest.mark.gpu
def test_refusals_write_nothing(pkg, tmp_path):
    c, files, _ = golden()
    P = S.variant_params("full")
    par = T.c_params(pkg, P)
    eng = engine(pkg, True, True)
    seen = T.handler(pkg, eng)
    path = str(tmp_path / "snap_000")
    kw = dict(pm_ti=S.PM_TI, mass_table=S.MASS_TABLE, ids=c["ids"], potential=c["potential"])

    def refused(what, status, fn):
        with open(path, "wb") as f:
            f.write(b"untouched")
        with pytest.raises(pkg.NgravsError) as e:
            fn()
        assert "status %d" % status in str(e.value) and what in str(e.value), str(e.value)
        with open(path, "rb") as f:
            assert f.read() == b"untouched", what

    def wr(cols, **over):
        a = dict(kw, blocks_mask=S.ALL_BLOCKS, snap_format=2, hubble_param=S.HUBBLE_PARAM)
        a.update(over)
        eng.write_snapshot(path, cols, par, S.TI, **a)
    out = np.full((10, 3), 123.0, dtype=np.float32)
    # a block call without a plan (also: the plan does not survive a refused plan)
    refused("no plan", -4, lambda: eng.snapshot_block(pkg.abi.SNAP_POS, time_cols(c), par, S.TI, first=0, count=10, out=out, **kw))
    bad = dict(time_cols(c), type=c["type"].copy())
    bad["type"][317] = 6
    refused("type outside 0..5", -1, lambda: eng.snapshot_plan(bad))
    refused("type outside 0..5", -1, lambda: wr(bad))
    refused("no plan", -4, lambda: eng.snapshot_block(pkg.abi.SNAP_POS, time_cols(c), par, S.TI, first=0, count=10, out=out, **kw))
    # a gas column that is missing while there is gas
    nogas = {k: v for k, v in time_cols(c).items() if k != "density"}
    refused("density is missing", -1, lambda: wr(nogas))
    eng.snapshot_plan(time_cols(c))
    refused("density is missing", -1, lambda: eng.snapshot_block(pkg.abi.SNAP_RHO, nogas, par, S.TI, first=0, count=10, out=out[:, 0].copy(), **kw))
    # a range beyond the block, an n that is not the plan's, a mesh without pm_ti
    total = len(c["type"])
    refused("range is outside the block POS", -1, lambda: eng.snapshot_block(pkg.abi.SNAP_POS, time_cols(c), par, S.TI, first=total - 5, count=10, out=out, **kw))
    refused("range is outside the block U", -1, lambda: eng.snapshot_block(pkg.abi.SNAP_U, time_cols(c), par, S.TI, first=0, count=int(npart_of(c)[0]) + 1,
                                                                           out=np.zeros(total, dtype=np.float32), **kw))
    short = {k: v[:-1] for k, v in time_cols(c).items()}
    refused("n is not the plan's", -4, lambda: eng.snapshot_block(pkg.abi.SNAP_POS, short, par, S.TI, first=0, count=10, out=out,
                                                                  **dict(kw, ids=c["ids"][:-1], potential=c["potential"][:-1])))
    refused("pm_ti", -1, lambda: eng.snapshot_block(pkg.abi.SNAP_VEL, time_cols(c), par, S.TI, first=0, count=10, out=out, **dict(kw, pm_ti=None)))
    # a periodic position that is not finite, or 1024 box lengths away
    for x in (np.nan, np.inf, -1024.0 * S.BOX):
        far = dict(time_cols(c), pos=c["pos"].copy())
        far["pos"][411, 1] = x
        refused("block POS", -1, lambda: wr(far))
        row = int(np.flatnonzero(S.file_order(c["type"]) == 411)[0])
        refused("block POS", -1, lambda: eng.snapshot_block(pkg.abi.SNAP_POS, far, par, S.TI, first=row - 4, count=10, out=out, **kw))
        ok = eng.snapshot_block(pkg.abi.SNAP_POS, far, par, S.TI, first=row + 1, count=10, **kw)   # a range without that row is served
        assert np.isfinite(ok).all()
    refused("HDF5", -1, lambda: wr(time_cols(c), snap_format=3))
    refused("snap_format", -1, lambda: wr(time_cols(c), snap_format=0))
    refused("buffer_bytes", -1, lambda: wr(time_cols(c), buffer_bytes=8))
    assert np.all(out == 123.0)
    assert len(seen) >= 15 and all(code < 0 for code, _ in seen)
    # and the engine still writes
    wr(time_cols(c))
    with open(path, "rb") as f:
        assert_same_file(f.read(), files["full"], c, S.ALL_BLOCKS, 2, S.MASS_TABLE, "after the refusals")


@pytest.mark.gpu
def test_round_trip_through_the_readers(pkg, tmp_path):
    c, _, _ = golden()
    P = S.variant_params("full")
    eng = engine(pkg, True, True)
    order = S.file_order(c["type"])
    gas = order[c["type"][order] == 0]
    for fmt in (1, 2):
        path = str(tmp_path / ("snap_%d" % fmt))
        write(pkg, eng, path, c, P, "device", S.ALL_BLOCKS & ~(1 << 7), fmt, True, potential=False)
        mask = pkg.abi.snap_mask("ACCE", "ENDT", "TSTP")
        hdr, blocks = pkg.snapshot.read_blocks(path, mask if fmt == 1 else None)
        assert list(blocks) == ["POS", "VEL", "ID", "MASS", "U", "RHO", "HSML", "ACCE", "ENDT", "TSTP"]
        assert np.array_equal(blocks["RHO"], c["density"][gas].astype(np.float32))
        assert np.array_equal(blocks["HSML"], c["hsml"][gas].astype(np.float32))
        assert np.array_equal(blocks["ENDT"], c["dt_entropy"][gas].astype(np.float32))
        assert np.array_equal(blocks["TSTP"], ((c["ti_endstep"] - c["ti_begstep"])[order] * P["timebase_interval"]).astype(np.float32))
        assert np.array_equal(blocks["ACCE"], S.fill_block("ACCE", c, P, S.TI, True, S.PM_TI, True))
        assert np.array_equal(blocks["ID"], c["ids"][order])
        # ic.read_snapshot: the first five blocks -- the float32 of the inputs grouped by type, the masses expanded from the header
        snap = pkg.ic.read_snapshot(path)
        assert np.array_equal(snap["type"], c["type"][order]) and np.array_equal(snap["ids"], c["ids"][order].astype(np.uint32))
        assert np.array_equal(snap["pos"].astype(np.float32), S.fill_block("POS", c, P, S.TI, periodic=True))
        inside = np.all((c["pos"][order] >= 0) & (c["pos"][order] < S.BOX * (1 - 1e-7)), axis=1)
        assert inside.sum() > 500 and np.array_equal(snap["pos"][inside].astype(np.float32), c["pos"][order][inside].astype(np.float32))
        assert np.array_equal(snap["vel"].astype(np.float32), S.fill_block("VEL", c, P, S.TI, True, S.PM_TI, True))
        mass = np.where(S.MASS_TABLE[c["type"]] == 0, c["mass"].astype(np.float32).astype(np.float64), S.MASS_TABLE[c["type"]])
        assert np.array_equal(snap["mass"], mass[order])
        assert np.array_equal(snap["u"].astype(np.float32), blocks["U"])


# ---- the loop -------------------------------------------------------------------------------------------------------------
STEP = 1 << 23   # max_size_timestep on the integer time line of the run below


def loop_run(pkg, tmp_path, with_output, output_kw=True):
    import torch
    n = 64
    pos, mass, _ = pkg.ic.plummer_sphere(n, seed=21)
    rng = np.random.default_rng(22)
    ptype = np.where(np.arange(n) % 3 == 0, 2, 1).astype(np.int32)
    vel = rng.normal(size=(n, 3)) * 0.3
    soft = [0, 0.05, 0.05, 0, 0, 0.0]
    # gravity so weak that every row takes max_size_timestep: the sync points are the multiples of STEP
    cfg = pkg.make_config(n_gravs=1, G=1e-8, softening=soft, theta=0.0, err_tol_force_acc=0.005)
    eng = pkg.Engine(cfg)
    P = T.params(False, time_max=8.0, timebase_interval=8.0 / T.TB, max_size_timestep=0.25, min_size_timestep=0.0)
    assert 0.25 / P["timebase_interval"] == STEP
    host = dict(type=ptype, pos=pos, vel=vel, mass=mass, ti_begstep=np.zeros(n, np.int32), ti_endstep=np.zeros(n, np.int32),
                grav_accel=np.zeros((n, 3)), grav_pm=np.zeros((n, 3)), old_acc=np.zeros(n))
    cols = {k: torch.from_numpy(v).cuda() for k, v in host.items()}
    ids = torch.arange(1000, 1000 + n, dtype=torch.int32, device="cuda")
    mass_table = np.array([0, 0, float(mass[0]), 0, 0, 0.0])
    captured = []

    def on_station(name, tl):
        if name == "snapshot":
            captured.append((tl.ti_current, tl.time, {k: v.cpu().numpy().copy() for k, v in tl.cols.items()}))
    kw = {}
    if with_output:
        # output times at 2.5, 5, 7.5, ... steps: two strictly between sync points for every one on a sync point
        rule = pkg.abi.make_output_rule(time_of_first_snapshot=2.5 * 0.25, time_bet_snapshot=2.5 * 0.25)
        kw["output"] = dict(dir=str(tmp_path) + os.sep, base="snap", snap_format=2, rule=rule, blocks_mask=pkg.abi.snap_mask("ACCE", "TSTP"),
                            mass_table=mass_table, ids=lambda tl: ids, buffer_bytes=600, hubble_param=0.7)
    elif output_kw:
        kw["output"] = None
    tl = pkg.timeline.Timeline(eng, cols, T.c_params(pkg, P), on_station=on_station, **kw)
    sync = []
    for _ in range(16):
        sync.append(tl.step())
    return tl, P, {k: v.cpu().numpy() for k, v in cols.items()}, captured, sync, mass_table, ids.cpu().numpy()


@pytest.mark.gpu
def test_timeline_writes_the_snapshots_of_the_output_rule(pkg, tmp_path):
    tl, P, final, captured, sync, mass_table, ids = loop_run(pkg, tmp_path, True)
    assert sync == [k * STEP for k in range(16)]
    want_ti = [int(2.5 * k * STEP) for k in range(1, 7)]   # 2.5, 5, 7.5, 10, 12.5, 15 steps
    assert [ti for ti, _, _ in captured] == want_ti
    assert sum(ti % STEP != 0 for ti in want_ti) == 3 and sum(ti % STEP == 0 for ti in want_ti) == 3
    assert tl.snapshot_file_count == 6 and tl.ti_nextoutput == int(17.5 * STEP)
    assert sorted(os.listdir(tmp_path)) == ["snap_%03d" % k for k in range(6)]
    mask = pkg.abi.snap_mask("ACCE", "TSTP")
    for k, (ti, time, c) in enumerate(captured):
        with open(tmp_path / ("snap_%03d" % k), "rb") as f:
            got = f.read()
        assert time == P["time_begin"] + ti * P["timebase_interval"]
        c = dict(c, ids=ids)
        want = S.file_bytes(c, P, ti, mask, 2, False, None, False, box=0.0, mass_table=mass_table, hubble_param=0.7)
        assert got == want, k
        hdr, blocks = pkg.snapshot.read_blocks(str(tmp_path / ("snap_%03d" % k)))
        assert hdr["time"] == time and list(blocks) == ["POS", "VEL", "ID", "MASS", "ACCE", "TSTP"]
        assert np.all(blocks["TSTP"] == np.float32(0.25)) and len(blocks["MASS"]) == (c["type"] == 1).sum()
    # the last snapshot of run.c:136 is the caller's
    path = tl.write_snapshot()
    assert path.endswith("snap_006") and tl.snapshot_file_count == 7 and os.path.exists(path)


@pytest.mark.gpu
def test_timeline_without_output_is_the_loop_as_it_was(pkg, tmp_path):
    """output=None leaves the loop alone: the columns of a run without the argument, bit for bit"""
    _, _, a, cap_a, sync_a, _, _ = loop_run(pkg, tmp_path, False, output_kw=False)
    _, _, b, cap_b, sync_b, _, _ = loop_run(pkg, tmp_path, False, output_kw=True)
    assert sync_a == sync_b == [k * STEP for k in range(16)] and cap_a == cap_b == [] and os.listdir(tmp_path) == []
    for k in a:
        assert np.array_equal(a[k], b[k], equal_nan=True), k
