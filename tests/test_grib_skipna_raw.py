"""Raw GRIB fields under skipna, host side: the four _na ABI entries (smm_apply_grib_na, smm_apply_host_grib_na,
smm_group_apply_grib_na, smm_group_apply_host_grib_na) in the header, the exports and the ctypes table, every refusal of
theirs that needs no device, the `skipna=` keyword of the four Python methods and `Regridder(packed_skipna=)`.  The
library is loaded; no device is touched."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, OperatorGroup, Regridder, SparseOperator,
                           _lib)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_p, _i64, _int, _dbl, _uint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_uint
_grp, _gbp = ctypes.POINTER(_lib.GribRowStruct), ctypes.POINTER(_lib.GribBitmapStruct)
# each entry with its twin: the argument lists are the twin's
TWINS = {"smm_apply_grib_na": "smm_apply_grib_bm", "smm_apply_host_grib_na": "smm_apply_host_grib_bm",
         "smm_group_apply_grib_na": "smm_group_apply_grib", "smm_group_apply_host_grib_na": "smm_group_apply_host_grib"}
ENTRIES = tuple(TWINS)


def header_code():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def declared(name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header_code(), flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


@pytest.mark.parametrize("name", ENTRIES)
def test_header_export_and_ctypes_table_agree(name):
    assert declared(name) == declared(TWINS[name])
    assert _lib.SIGNATURES[name] == _lib.SIGNATURES[TWINS[name]]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
    assert getattr(_lib.load(), name).argtypes == _lib.SIGNATURES[TWINS[name]]


def _call(name, x, x_bytes, rows, bitmaps, y, y_code=_lib.SMM_F64, shape=(1, 2, 1), level_index=(0, 0), area_min=0.0,
          flags=0, handle=None):
    lib = _lib.load()
    rp = None if rows is None else ctypes.cast(rows.ctypes.data, _grp)
    bp = None if bitmaps is None else ctypes.cast(bitmaps.ctypes.data, _gbp)
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)     # noqa: E731
    lev = None if level_index is None else np.asarray(level_index, np.int32)
    n_rows = shape[0] * shape[1] * shape[2] if min(shape) >= 0 else -1
    fn = getattr(lib, name)
    name = {twin: na for na, twin in TWINS.items()}.get(name, name)      # a twin takes the arguments of its _na entry
    if name == "smm_apply_grib_na":
        rc = fn(handle, ptr(x), x_bytes, rp, bp, ptr(y), y_code, 4, n_rows, area_min, flags, None)
    elif name == "smm_apply_host_grib_na":
        rc = fn(handle, ptr(x), x_bytes, rp, bp, ptr(y), y_code, 4, n_rows, area_min, flags, 0)
    elif name == "smm_group_apply_host_grib_na":
        rc = fn(handle, ptr(x), x_bytes, rp, bp, ptr(y), y_code, *shape, 1, ptr(lev), None, area_min, flags, 0)
    else:
        rc = fn(handle, ptr(x), x_bytes, rp, bp, ptr(y), y_code, 4, 4, 4, *shape, ptr(lev), None, area_min, flags, None)
    return rc, (lib.smm_last_error() or b"").decode()


@pytest.mark.parametrize("with_bitmaps", [True, False])
@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_that_need_no_device(name, with_bitmaps):
    """The refusals of the twins with their codes and a message, on a NULL handle -- each comes back before the handle is
    looked at -- in the order flags, result type, pointers, rules; SMM_APPLY_SKIPNA is implied and may be passed."""
    x = np.zeros(64, np.uint8)
    y = np.zeros(8, np.float64)
    group = "group" in name
    null_handle = "null group" if group else "null operator"

    def good(n=2):
        rows = np.zeros(n, GRIB_ROW_DTYPE)
        rows["bscale"], rows["ddiv"], rows["nbits"] = 0.25, 10.0, 16
        rows["ref"] = -3.5
        return rows

    def bms(n=2):
        if not with_bitmaps:
            return None
        b = np.zeros(n, GRIB_BITMAP_DTYPE)
        b["bitmap_off"], b["n_values"] = (60, GRIB_NO_BITMAP, 0)[:n], (5, 17, 0)[:n]
        return b

    INV, UNS = _lib.SMM_ERR_INVALID, _lib.SMM_ERR_UNSUPPORTED
    NA = _lib.APPLY_SKIPNA

    def refused(code, word, rows=None, **kw):
        rows = good() if rows is None else rows
        args = dict(x=x, x_bytes=64, rows=rows, bitmaps=bms(rows.size), y=y)
        args.update(kw)
        rc, msg = _call(name, **args)
        assert rc == code and word in msg, (rc, msg, word)

    for field, bad, word in (("nbits", -1, "nbits"), ("nbits", 33, "nbits"), ("reserved", 1, "reserved"),
                             ("bscale", 3.0, "bscale"), ("bscale", 0.0, "bscale"), ("bscale", np.nan, "bscale"),
                             ("ddiv", 0.0, "ddiv"), ("ddiv", np.inf, "ddiv"), ("ref", np.inf, "ref"), ("ref", np.nan, "ref")):
        rows = good()
        rows[field][1] = bad
        refused(INV, "rows[1]." + word, rows=rows)
    refused(INV, "null", x=None)
    refused(INV, "null", y=None)
    rc, msg = _call(name, x, 64, None, bms(), y)
    assert rc == INV and "null" in msg
    for shape in ((-1, 2, 1), (1, -2, 1), (1, 2, -1)):
        refused(INV, "negative batch", shape=shape)
    refused(INV, "x_bytes", x_bytes=-4)
    refused(INV, "remap_area_min", area_min=1.5)
    if "host" not in name:
        refused(INV, "aligned", x=x.ctypes.data + 1, x_bytes=60)
    refused(INV, "aligned", y=y.ctypes.data + 4)
    # 1. flag bits outside the ABI's set
    refused(INV, "unknown apply flag", flags=1 << 20)
    refused(INV, "unknown apply flag", flags=NA | 1 << 20)
    # 2. SMM_APPLY_NO_FILL, by the SKIPNA rule of the header -- the bit is implied, so without it too
    refused(INV, "SMM_APPLY_NO_FILL", flags=_lib.APPLY_NO_FILL)
    refused(INV, "SMM_APPLY_NO_FILL", flags=_lib.APPLY_NO_FILL | NA)
    # 3. the kernels not built for GRIB fields; the message no longer names SMM_APPLY_SKIPNA among them
    for flag in (_lib.APPLY_KERNEL_TILE, _lib.APPLY_SB_PACKED, _lib.APPLY_HOST_NO_PACK, _lib.APPLY_SB_Y_SB):
        for extra in (0, NA):
            refused(UNS, "not built", flags=flag | extra)
            rc, msg = _call(name, x, 64, good(), bms(), y, flags=flag | extra)
            assert "SMM_APPLY_SKIPNA" not in msg, msg
    # 4. the result type
    for y_code in (_lib.SMM_F32, _lib.SMM_I16, _lib.SMM_F16):
        refused(UNS, "SMM_F64", y_code=y_code)
    # the order: unknown bits < NO_FILL < unbuilt kernels < result type < pointers < rules < handle
    bad = good()
    bad["nbits"][0] = 40
    worst = dict(y_code=_lib.SMM_F32, y=None, rows=bad)
    refused(INV, "unknown apply flag", flags=1 << 20 | _lib.APPLY_NO_FILL | _lib.APPLY_KERNEL_TILE, **worst)
    refused(INV, "SMM_APPLY_NO_FILL", flags=_lib.APPLY_NO_FILL | _lib.APPLY_KERNEL_TILE, **worst)
    refused(UNS, "not built", flags=_lib.APPLY_KERNEL_TILE, **worst)
    refused(UNS, "SMM_F64", **worst)
    refused(INV, "null", y=None, rows=bad)
    refused(INV, "rows[0].nbits", rows=bad)
    # nothing to refuse without the handle: a well-formed call reaches it with SMM_APPLY_SKIPNA set and unset, whatever
    # the levels and ranges say
    rows = good(3)
    rows["nbits"], rows["bscale"], rows["ddiv"] = (0, 32, 1), (2.0 ** -1022, 2.0 ** 1023, 1.0), (1.0, 0.1, 1e-300)
    b = bms(3)
    if b is not None:
        b["n_values"][0] = 2 ** 40
    for extra in (0, NA):
        rc, msg = _call(name, x, 64, rows, b, y, shape=(1, 3, 1), level_index=(7, -1, 0),
                        flags=_lib.APPLY_MASKED | _lib.APPLY_KERNEL_SELL | extra, area_min=0.5)
        assert rc == INV and null_handle in msg, (rc, msg)
    # an empty call is refused for its handle too, not accepted
    rc, msg = _call(name, x, 64, good(0), None, y, shape=(0, 2, 1))
    assert rc == INV and null_handle in msg, (rc, msg)
    # the ABI version stays, and the twin, which shares the check, still refuses the bit and still names it
    assert _lib.load().smm_abi_version() == 6
    rc, msg = _call(TWINS[name], x, 64, good(), bms(), y, flags=NA)
    assert rc == UNS and "SMM_APPLY_SKIPNA" in msg and "not built" in msg, (rc, msg)


def fake_operator(n_src=40, n_dst=6):
    op = SparseOperator.__new__(SparseOperator)
    op.handle, op.n_src, op.n_dst = None, n_src, n_dst
    return op


def fake_group(n_ops=3, n_src=40, n_dst=6):
    grp = OperatorGroup.__new__(OperatorGroup)
    grp.operators = [fake_operator(n_src, n_dst) for _ in range(n_ops)]
    grp.handle, grp.n_src, grp.n_dst = None, n_src, n_dst
    return grp


def test_skipna_defaults_to_false_in_the_four_methods():
    for method in (SparseOperator.apply_grib, SparseOperator.apply_host_grib, OperatorGroup.apply_grib,
                   OperatorGroup.apply_host_grib):
        assert inspect.signature(method).parameters["skipna"].default is False


def test_apply_host_grib_skipna_picks_the_na_entry(monkeypatch):
    """skipna=True calls the _na entry with the twin's arguments (bitmaps or NULL); skipna=False calls what it called
    before, and a caller's APPLY_SKIPNA in flags= travels to that entry as it is, to be refused there."""
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    buf = np.zeros(16, np.uint8)
    rows = np.zeros(4, GRIB_ROW_DTYPE)
    bm = np.zeros(4, GRIB_BITMAP_DTYPE)
    bm["n_values"] = 100 + np.arange(4)
    op = fake_operator()
    out = op.apply_host_grib(buf, rows, bitmaps=bm, masked=True, remap_area_min=0.5, chunk_rows=3, skipna=True)
    assert out.shape == (4, 6) and out.dtype == np.float64
    op.apply_host_grib(buf, rows, skipna=True)
    op.apply_host_grib(buf, rows, bitmaps=bm)
    op.apply_host_grib(buf, rows)
    op.apply_host_grib(buf, rows, flags=_lib.APPLY_SKIPNA)
    assert [name for name, _ in calls] == ["smm_apply_host_grib_na", "smm_apply_host_grib_na", "smm_apply_host_grib_bm",
                                           "smm_apply_host_grib", "smm_apply_host_grib"]
    a = calls[0][1]
    assert len(a) == len(_lib.SIGNATURES["smm_apply_host_grib_na"])
    assert a[2] == 16 and a[6:] == (_lib.SMM_F64, 6, 4, 0.5, _lib.APPLY_MASKED, 3)
    got_bm = np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_uint64)), shape=(8,))
    assert got_bm[1::2].tolist() == [100, 101, 102, 103]
    assert calls[1][1][4] is None and calls[1][1][6:] == (_lib.SMM_F64, 6, 4, 0.0, 0, 0)
    assert calls[4][1][-2] == _lib.APPLY_SKIPNA
    # the group
    del calls[:]
    grp = fake_group()
    rows = np.zeros(12, GRIB_ROW_DTYPE)
    out = grp.apply_host_grib(buf, rows, [2, 0, 1], masked_levels=[1, 0, 1], masked=True, remap_area_min=0.5,
                              transpose=False, chunk_outer=4, n_inner=2, skipna=True)
    grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2)
    assert [name for name, _ in calls] == ["smm_group_apply_host_grib_na", "smm_group_apply_host_grib"]
    a = calls[0][1]
    assert out.shape == (3, 2, 2, 6) and len(a) == len(_lib.SIGNATURES["smm_group_apply_host_grib_na"])
    assert a[4] is None and a[7:11] == (2, 3, 2, 0) and a[13:] == (0.5, _lib.APPLY_MASKED, 4)


def test_regridder_packed_skipna_needs_packed_and_skipna():
    """In the wording of the packed_levels refusal; the Regridder refuses before it looks at its weights."""
    assert inspect.signature(Regridder.__init__).parameters["packed_skipna"].default is False
    for kw in (dict(), dict(packed=True), dict(skipna=True), dict(packed=True, packed_levels=True)):
        with pytest.raises(ValueError, match=r"packed_skipna=True needs packed=True and skipna=True"):
            Regridder(weights=object(), packed_skipna=True, **kw)
    with pytest.raises(ValueError, match=r"packed_levels=True needs packed=True"):
        Regridder(weights=object(), packed_levels=True, packed_skipna=True, skipna=True)


def grib_reason(dims, levels=False, out_dtype=np.float64, codec=None, mask_dim="isobaricInhPa", **switches):
    """why `road.decide` sends a `GribField` with these dims to the host decoder, or None: it stays raw"""
    from smmregrid_amd import road
    horizontal = [d for d in dims if d in ("lat", "lon", "latitude", "longitude")]
    way = road.decide(road.Switches.of(out_dtype=out_dtype, **switches),
                      road.Facts("t", road.GRIB, np.float32, dims, horizontal, mask_dim if levels else None, codec=codec))
    assert (way.source == road.RAW_GRIB) == (way.why is None) and way.source in (road.RAW_GRIB, road.DECODED)
    return way.why


def test_regridder_decides_the_raw_road_in_one_place():
    """`road.decide`, which `regrid_array` and direct calls of `apply_weights` and `regrid3d` share: skipna decodes on
    the host unless packed_skipna is on; the other fallbacks keep their reason either way."""
    def reason(levels=False, out_dtype=np.float64, by_level=True, **kw):
        dims = ("time", "lat", "lon") if not levels else ("time", "lev", "lat", "lon") if by_level else ("time", "lat", "lev", "lon")
        return grib_reason(dims, levels, out_dtype, mask_dim="lev", **kw)

    assert reason(packed=True) is None
    assert reason() is not None
    assert reason(packed=True, skipna=True) == "skipna"
    assert reason(packed=True, skipna=True, packed_skipna=True) is None
    assert reason(packed=True, skipna=True, packed_skipna=True, out_dtype=np.float32) == "out_dtype float32"
    assert reason(packed=True, skipna=True, packed_skipna=True, levels=True) == "masked levels"
    assert reason(packed=True, skipna=True, packed_skipna=True, packed_levels=True, levels=True) is None
    assert reason(packed=True, skipna=True, packed_levels=True, levels=True) == "skipna"
    assert reason(packed=True, skipna=True, packed_skipna=True, packed_levels=True, levels=True,
                  by_level=False).startswith("masked levels: its fields are not ordered")
