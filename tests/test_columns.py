"""The column hand-over of the C ABI (pointer, byte stride, on_device), through the raw library: ngravs_set_particles,
ngravs_set_old_acc, ngravs_set_gas_softening, ngravs_get_accel, ngravs_get_keys and ngravs_get_order take and give the same bits
whether a column is a contiguous host array, a field of an interleaved host record, a contiguous device tensor or a field of an
interleaved device record.  Sizes: one thread, a 256-thread block of the pack kernels -1 / full / +1, and several blocks.

Two species, tree only, Newtonian, strict walk (one thread per target, so equal inputs give equal bits) with the relative opening
criterion (ErrTolTheta = 0), so that the OldAcc column decides what a walk opens."""
import ctypes as C
import functools

import numpy as np
import pytest

NS = (1, 255, 256, 257, 1000)
LAYOUTS = ("host", "host_rec", "dev", "dev_rec")
ARG = -1
SENTINEL = -3.25
OUT_FIELDS = [("grav_accel", np.float64, (3,)), ("old_acc", np.float64), ("grav_cost", np.float32)]


def record(fields, n):
    """an array of structs around the fields: a leading float64 and a trailing int32[3] that no call may touch"""
    rec = np.zeros(n, dtype=np.dtype([("pad0", np.float64)] + fields + [("pad1", np.int32, (3,))], align=True))
    assert rec.dtype.itemsize not in (4, 8, 24)
    return rec


@functools.lru_cache(maxsize=None)
def particle_set(n):
    rng = np.random.default_rng(4100 + n)
    cols = {"pos": rng.random((n, 3)), "mass": 0.5 + rng.random(n), "type": rng.integers(0, 3, n).astype(np.int32),
            "old_acc": n * (0.2 + rng.random(n)), "active": (rng.random(n) < 0.5).astype(np.uint8),
            "grav_cost": (1 + 50 * rng.random(n)).astype(np.float32)}
    cols["type"][0], cols["active"][0] = 0, 1   # (a gas row and a walked row at every size)
    return cols


def config(pkg):
    return pkg.make_config(n_gravs=2, G=1.0, theta=0.0, err_tol_force_acc=0.005, softening=[0.01] * 6, type_to_grav=[0, 0, 1, 0, 0, 0],
                           wiring="newton", walk_mode=pkg.WALK_STRICT)


def columns(cols, layout):
    """{name: (address, stride)}, on_device, and what must stay alive while the addresses are used"""
    import torch
    names = list(cols)
    if layout in ("host", "dev"):
        arrs = {k: np.ascontiguousarray(cols[k]) for k in names}
        if layout == "dev":
            arrs = {k: torch.from_numpy(v).cuda() for k, v in arrs.items()}
            return {k: (v.data_ptr(), v.stride(0) * v.element_size()) for k, v in arrs.items()}, 1, arrs
        return {k: (v.ctypes.data, v.strides[0]) for k, v in arrs.items()}, 0, arrs
    n = len(cols[names[0]])
    rec = record([(k, cols[k].dtype, cols[k].shape[1:]) for k in names], n)
    for k in names:
        rec[k] = cols[k]
    off = {k: rec.dtype.fields[k][1] for k in names}
    if layout == "dev_rec":
        t = torch.from_numpy(rec.view(np.uint8).reshape(n, rec.dtype.itemsize)).cuda()
        return {k: (t.data_ptr() + off[k], rec.dtype.itemsize) for k in names}, 1, t
    return {k: (rec.ctypes.data + off[k], rec.dtype.itemsize) for k in names}, 0, rec


def set_particles(pkg, L, eng, cols, layout):
    addr, on_device, keep = columns(cols, layout)
    p = pkg.abi.Particles()
    p.n = len(cols["pos"])
    for k, (a, s) in addr.items():
        setattr(p, k, a)
        setattr(p, k + "_stride", s)
    p.on_device = on_device
    rc = L.ngravs_set_particles(eng._h, C.byref(p))
    del keep
    return rc


def walk(L, eng):
    assert L.ngravs_gravity_tree(eng._h) == 0, L.ngravs_last_error(eng._h)


def get_accel(L, eng, n, only_active=0, fill=0.0):
    acc, old, cost = np.full((n, 3), fill), np.full(n, fill), np.full(n, fill, dtype=np.float32)
    assert L.ngravs_get_accel(eng._h, acc.ctypes.data, 24, None, 0, old.ctypes.data, 8, cost.ctypes.data, 4, 0, only_active) == 0
    return {"grav_accel": acc, "old_acc": old, "grav_cost": cost}


def bits(a):
    return np.ascontiguousarray(a).view(np.uint8)


def same_bits(a, b):
    return a.shape == b.shape and a.dtype == b.dtype and np.array_equal(bits(a), bits(b))


_ENGINES = {}


def engine_with_tree(pkg, n, layout="host"):
    L = pkg.lib()
    eng = pkg.Engine(config(pkg))
    eng.n = n
    assert set_particles(pkg, L, eng, particle_set(n), layout) == 0, L.ngravs_last_error(eng._h)
    assert L.ngravs_domain_decomposition(eng._h) == 0
    assert L.ngravs_force_treebuild(eng._h) >= 0
    return eng


def walked(pkg, n, layout):
    """an engine after hand-over (by layout), decomposition, tree build and a strict walk, with its results; kept for the module
    and never changed by a test"""
    if (n, layout) not in _ENGINES:
        L = pkg.lib()
        eng = engine_with_tree(pkg, n, layout)
        walk(L, eng)
        res = get_accel(L, eng, n)
        order, keys = np.zeros(n, dtype=np.int32), np.zeros(n, dtype=np.int64)
        assert L.ngravs_get_order(eng._h, order.ctypes.data, 0) == 0 and L.ngravs_get_keys(eng._h, keys.ctypes.data, 0) == 0
        res["order"], res["keys"] = order, keys
        _ENGINES[(n, layout)] = (eng, res)
    return _ENGINES[(n, layout)]


@pytest.fixture(scope="module", autouse=True)
def _close_engines():
    yield
    for eng, _ in _ENGINES.values():
        eng.close()
    _ENGINES.clear()


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_four_layouts_of_the_hand_over_give_the_same_bits(pkg, n):
    ref = walked(pkg, n, "host")[1]
    assert sorted(ref["order"].tolist()) == list(range(n))
    assert n == 1 or (np.abs(ref["grav_accel"]).max() > 0 and ref["grav_cost"].max() > 0)
    for layout in LAYOUTS[1:]:
        got = walked(pkg, n, layout)[1]
        for k in ref:
            assert same_bits(ref[k], got[k]), (layout, k)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_get_order_and_keys_on_the_device_are_the_host_arrays(pkg, n):
    import torch
    eng, ref = walked(pkg, n, "host")
    L = pkg.lib()
    order, keys = torch.full((n,), -7, dtype=torch.int32).cuda(), torch.full((n,), -7, dtype=torch.int64).cuda()
    assert L.ngravs_get_order(eng._h, order.data_ptr(), 1) == 0 and L.ngravs_get_keys(eng._h, keys.data_ptr(), 1) == 0
    assert np.array_equal(order.cpu().numpy(), ref["order"]) and np.array_equal(keys.cpu().numpy(), ref["keys"])


def get_accel_into(L, eng, n, where, only_active):
    """the three result columns through `where`, every destination filled with the sentinel first -> (rc, columns, pads)"""
    import torch
    if where in ("host", "dev"):
        out = {"grav_accel": np.full((n, 3), SENTINEL), "old_acc": np.full(n, SENTINEL), "grav_cost": np.full(n, SENTINEL, dtype=np.float32)}
        if where == "dev":
            out = {k: torch.from_numpy(v).cuda() for k, v in out.items()}
        ptr = {k: (v.data_ptr() if where == "dev" else v.ctypes.data) for k, v in out.items()}
        rc = L.ngravs_get_accel(eng._h, ptr["grav_accel"], 24, None, 0, ptr["old_acc"], 8, ptr["grav_cost"], 4, int(where == "dev"),
                                only_active)
        return rc, {k: (v.cpu().numpy() if where == "dev" else v) for k, v in out.items()}, None
    rec = record(OUT_FIELDS, n)
    for f in OUT_FIELDS:
        rec[f[0]] = SENTINEL
    stride = rec.dtype.itemsize
    t = torch.from_numpy(rec.view(np.uint8).reshape(n, stride)).cuda() if where == "dev_rec" else None
    base = t.data_ptr() if where == "dev_rec" else rec.ctypes.data
    ptr = {f[0]: base + rec.dtype.fields[f[0]][1] for f in OUT_FIELDS}
    rc = L.ngravs_get_accel(eng._h, ptr["grav_accel"], stride, None, 0, ptr["old_acc"], stride, ptr["grav_cost"], stride,
                            int(where == "dev_rec"), only_active)
    if where == "dev_rec":
        rec = t.cpu().numpy().view(rec.dtype).reshape(n)
    return rc, {f[0]: rec[f[0]] for f in OUT_FIELDS}, (rec["pad0"], rec["pad1"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_download_into_a_strided_host_record(pkg, n):
    eng, ref = walked(pkg, n, "host")
    rc, got, pads = get_accel_into(pkg.lib(), eng, n, "host_rec", 0)
    assert rc == 0
    for k in got:
        assert same_bits(np.ascontiguousarray(got[k]), ref[k]), k
    assert np.all(pads[0] == 0) and np.all(pads[1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("where", ["host", "host_rec", "dev"])
def test_only_active_writes_the_flagged_rows_alone(pkg, n, where):
    eng, ref = walked(pkg, n, "host")
    act = particle_set(n)["active"] != 0
    rc, got, pads = get_accel_into(pkg.lib(), eng, n, where, 1)
    assert rc == 0
    for k in got:
        g = np.ascontiguousarray(got[k])
        assert same_bits(g[act], ref[k][act]), k
        assert same_bits(g[~act], np.full_like(g[~act], SENTINEL)), k
    assert pads is None or (np.all(pads[0] == 0) and np.all(pads[1] == 0))


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("only_active", [0, 1])
def test_a_strided_device_destination_is_refused(pkg, n, only_active):
    eng, _ = walked(pkg, n, "host")
    L = pkg.lib()
    rc, got, pads = get_accel_into(L, eng, n, "dev_rec", only_active)
    assert rc == ARG and "device outputs must be contiguous" in L.ngravs_last_error(eng._h).decode()
    for k in got:
        g = np.ascontiguousarray(got[k])
        assert same_bits(g, np.full_like(g, SENTINEL)), k
    assert np.all(pads[0] == 0) and np.all(pads[1] == 0)


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_a_type_outside_0_to_5_is_refused(pkg, n):
    L = pkg.lib()
    eng = pkg.Engine(config(pkg))
    for layout in LAYOUTS:
        for bad in (6, -1):
            cols = dict(particle_set(n))
            cols["type"] = cols["type"].copy()
            cols["type"][n - 1] = bad
            assert set_particles(pkg, L, eng, cols, layout) == ARG, (layout, bad)
            assert "particle Type outside 0..5" in L.ngravs_last_error(eng._h).decode()
            L.ngravs_set_old_acc(eng._h, cols["old_acc"].ctypes.data, 8, 0)   # (any call after it: the message above is of the refusal)
    eng.close()


def column_variants(col):
    """the column handed over every way: (address, stride, on_device, keep-alive) by layout"""
    out = {}
    for layout in LAYOUTS:
        addr, on_device, keep = columns({"pad_a": np.zeros(len(col), dtype=np.int32), "col": col}, layout)
        out[layout] = addr["col"] + (on_device, keep)
    assert out["host_rec"][1] != 8 and out["dev_rec"][1] != 8
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_set_old_acc_strided_and_on_the_device(pkg, n):
    eng = engine_with_tree(pkg, n)
    L = pkg.lib()
    rng = np.random.default_rng(4200 + n)
    old = n * (0.01 + 3 * rng.random(n))
    never_open = np.full(n, 1e30)
    res = {}
    for layout, (ptr, stride, on_device, keep) in column_variants(old).items():
        assert L.ngravs_set_old_acc(eng._h, never_open.ctypes.data, 8, 0) == 0   # (so that a call that did nothing shows)
        assert L.ngravs_set_old_acc(eng._h, ptr, stride, on_device) == 0, layout
        walk(L, eng)
        res[layout] = get_accel(L, eng, n)
    assert L.ngravs_set_old_acc(eng._h, never_open.ctypes.data, 8, 0) == 0
    walk(L, eng)
    other = get_accel(L, eng, n)   # another column, another result: the walks above did read theirs
    for layout in LAYOUTS[1:]:
        for k in res["host"]:
            assert same_bits(res["host"][k], res[layout][k]), (layout, k)
    eng.close()
    assert n < 255 or not np.array_equal(other["grav_cost"], res["host"]["grav_cost"])


@pytest.mark.gpu
@pytest.mark.parametrize("n", NS)
def test_set_gas_softening_strided_and_on_the_device(pkg, n):
    eng = engine_with_tree(pkg, n)
    L = pkg.lib()
    rng = np.random.default_rng(4300 + n)
    old = particle_set(n)["old_acc"]
    hsml = 0.05 + 0.2 * rng.random(n)
    res = {}
    for layout, (ptr, stride, on_device, keep) in list(column_variants(hsml).items()) + [("off", (None, 0, 0, None))]:
        assert L.ngravs_set_gas_softening(eng._h, None, 0, 0) == 0
        assert L.ngravs_set_gas_softening(eng._h, ptr, stride, on_device) == 0, (layout, L.ngravs_last_error(eng._h))
        assert L.ngravs_set_old_acc(eng._h, old.ctypes.data, 8, 0) == 0
        walk(L, eng)
        res[layout] = get_accel(L, eng, n)
    for layout in LAYOUTS[1:]:
        for k in res["host"]:
            assert same_bits(res["host"][k], res[layout][k]), (layout, k)
    eng.close()
    assert n < 255 or not np.array_equal(res["off"]["grav_accel"], res["host"]["grav_accel"])
