"""Raw GRIB fields on masked-level weights, host side: the two group ABI entries (smm_group_apply_grib,
smm_group_apply_host_grib) in the header, the exports and the ctypes table, every refusal of theirs that needs no device,
and the argument shaping of `OperatorGroup.apply_host_grib`.  The library is loaded; no device is touched."""
import ctypes
import os
import re

import numpy as np
import pytest

from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, OperatorGroup, SparseOperator, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("smm_group_apply_grib", "smm_group_apply_host_grib")
_p, _i64, _int, _dbl, _uint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_double, ctypes.c_uint
_grp, _gbp = ctypes.POINTER(_lib.GribRowStruct), ctypes.POINTER(_lib.GribBitmapStruct)
# parameter by parameter: (C declaration, ctypes type)
DEVICE = [("smm_group_t g", _p), ("const void* x", _p), ("int64_t x_bytes", _i64), ("const smm_grib_row_t* rows", _grp),
          ("const smm_grib_bitmap_t* bitmaps", _gbp), ("void* y", _p), ("int y_dtype", _int), ("int64_t ys_outer", _i64),
          ("int64_t ys_lev", _i64), ("int64_t ys_inner", _i64), ("int64_t n_outer", _i64), ("int64_t n_lev", _i64),
          ("int64_t n_inner", _i64), ("const int32_t* level_index", _p), ("const uint8_t* masked_levels", _p),
          ("double remap_area_min", _dbl), ("unsigned flags", _uint), ("void* stream", _p)]
HOST = [("smm_group_t g", _p), ("const void* x_host", _p), ("int64_t x_bytes", _i64), ("const smm_grib_row_t* rows", _grp),
        ("const smm_grib_bitmap_t* bitmaps", _gbp), ("void* y_host", _p), ("int y_dtype", _int), ("int64_t n_outer", _i64),
        ("int64_t n_lev", _i64), ("int64_t n_inner", _i64), ("int transpose", _int), ("const int32_t* level_index", _p),
        ("const uint8_t* masked_levels", _p), ("double remap_area_min", _dbl), ("unsigned flags", _uint),
        ("int64_t chunk_outer", _i64)]


def header_code():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


@pytest.mark.parametrize("name,want", list(zip(ENTRIES, (DEVICE, HOST))))
def test_header_export_and_ctypes_table_agree(name, want):
    code = header_code()
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared"
    params = [" ".join(p.split()) for p in m.group(1).split(",")]
    assert params == [decl for decl, _ in want]
    assert _lib.SIGNATURES[name] == [t for _, t in want]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name), f"{name} is not exported"
    assert getattr(_lib.load(), name).argtypes == [t for _, t in want]


def test_the_abi_version_stays_6():
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", header_code()) and _lib.load().smm_abi_version() == 6


def _call(name, x, x_bytes, rows, bitmaps, y, y_code=_lib.SMM_F64, shape=(1, 2, 1), level_index=(0, 0), area_min=0.0,
          flags=0, group=None):
    lib = _lib.load()
    rp = None if rows is None else ctypes.cast(rows.ctypes.data, _grp)
    bp = None if bitmaps is None else ctypes.cast(bitmaps.ctypes.data, _gbp)
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)     # noqa: E731
    lev = None if level_index is None else np.asarray(level_index, np.int32)
    if "host" in name:
        rc = getattr(lib, name)(group, ptr(x), x_bytes, rp, bp, ptr(y), y_code, *shape, 1, ptr(lev), None, area_min, flags, 0)
    else:
        rc = getattr(lib, name)(group, ptr(x), x_bytes, rp, bp, ptr(y), y_code, 4, 4, 4, *shape, ptr(lev), None, area_min,
                                flags, None)
    return rc, (lib.smm_last_error() or b"").decode()


@pytest.mark.parametrize("with_bitmaps", [True, False])
@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_that_need_no_device(name, with_bitmaps):
    """The refusals of smm_apply_grib_bm, with their codes and a message, on a NULL group handle -- each comes back
    before the group is looked at -- and a call with nothing to refuse, which gets as far as the handle."""
    x = np.zeros(64, np.uint8)
    y = np.zeros(8, np.float64)

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

    def refused(code, word, rows=None, **kw):
        rows = good() if rows is None else rows
        args = dict(x=x, x_bytes=64, rows=rows, bitmaps=bms(rows.size), y=y)
        args.update(kw)
        rc, msg = _call(name, **args)
        assert rc == code and word in msg, (rc, msg, word)

    for field, bad, word in (("nbits", -1, "nbits"), ("nbits", 33, "nbits"), ("reserved", 1, "reserved"),
                             ("bscale", 3.0, "bscale"), ("bscale", 0.0, "bscale"), ("bscale", -2.0, "bscale"),
                             ("bscale", np.inf, "bscale"), ("bscale", np.nan, "bscale"), ("bscale", 2.0 ** -1030, "bscale"),
                             ("ddiv", 0.0, "ddiv"), ("ddiv", -10.0, "ddiv"), ("ddiv", np.inf, "ddiv"), ("ddiv", np.nan, "ddiv"),
                             ("ref", np.inf, "ref"), ("ref", -np.inf, "ref"), ("ref", np.nan, "ref")):
        rows = good()
        rows[field][1] = bad
        refused(INV, "rows[1]." + word, rows=rows)
    refused(INV, "null", x=None)
    refused(INV, "null", y=None)
    rc, msg = _call(name, x, 64, None, bms(), y)
    assert rc == INV and "null" in msg
    for shape in ((-1, 2, 1), (1, -2, 1), (1, 2, -1), (-1, -2, 1)):
        refused(INV, "negative batch", shape=shape)
    refused(INV, "x_bytes", x_bytes=-4)
    refused(INV, "remap_area_min", area_min=1.5)
    refused(INV, "unknown apply flag", flags=1 << 20)
    if "host" not in name:
        refused(INV, "aligned", x=x.ctypes.data + 1, x_bytes=60)
    refused(INV, "aligned", y=y.ctypes.data + 4)
    for y_code in (_lib.SMM_F32, _lib.SMM_I16, _lib.SMM_F16):
        refused(UNS, "SMM_F64", y_code=y_code)
    for flag in (_lib.APPLY_SKIPNA, _lib.APPLY_KERNEL_TILE, _lib.APPLY_SB_PACKED, _lib.APPLY_HOST_NO_PACK, _lib.APPLY_SB_Y_SB):
        refused(UNS, "not built", flags=flag)
    # the order of check_grib_call: flags before the result type before the pointers before the rules
    bad = good()
    bad["nbits"][0] = 40
    refused(INV, "unknown apply flag", flags=1 << 20, y_code=_lib.SMM_F32, y=None, rows=bad)
    refused(UNS, "not built", flags=_lib.APPLY_SKIPNA, y_code=_lib.SMM_F32, y=None, rows=bad)
    refused(UNS, "SMM_F64", y_code=_lib.SMM_F32, y=None, rows=bad)
    refused(INV, "null", y=None, rows=bad)
    refused(INV, "rows[0].nbits", rows=bad)
    # nothing to refuse without the group: the call reaches the handle, whatever the levels and ranges say
    rows = good(3)
    rows["nbits"], rows["bscale"], rows["ddiv"] = (0, 32, 1), (2.0 ** -1022, 2.0 ** 1023, 1.0), (1.0, 0.1, 1e-300)
    b = bms(3)
    if b is not None:
        b["n_values"][0] = 2 ** 40
    rc, msg = _call(name, x, 64, rows, b, y, shape=(1, 3, 1), level_index=(7, -1, 0),
                    flags=_lib.APPLY_MASKED | _lib.APPLY_NO_FILL | _lib.APPLY_KERNEL_SELL)
    assert rc == INV and "null group" in msg, (rc, msg)
    # an empty call is refused for its handle too, not accepted
    rc, msg = _call(name, x, 64, good(0), None, y, shape=(0, 2, 1))
    assert rc == INV and "null group" in msg, (rc, msg)


def fake_group(n_ops=3, n_src=40, n_dst=6):
    """An OperatorGroup object without a handle: what `_grib_args` and `apply_host_grib` read from it."""
    grp = OperatorGroup.__new__(OperatorGroup)
    grp.operators = [SparseOperator.__new__(SparseOperator) for _ in range(n_ops)]
    grp.handle, grp.n_src, grp.n_dst = None, n_src, n_dst
    return grp


def test_apply_host_grib_shapes_its_arguments(monkeypatch):
    """rows and bitmaps flat (n_lev from level_index, n_inner from the keyword) or (n_outer, n_lev, n_inner); the result
    array follows `transpose`; what reaches the entry is counted out parameter by parameter."""
    grp = fake_group()
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    rows = np.zeros(2 * 3 * 2, GRIB_ROW_DTYPE)
    rows["byte_off"] = np.arange(12)
    bm = np.zeros(12, GRIB_BITMAP_DTYPE)
    bm["n_values"] = 100 + np.arange(12)
    buf = np.zeros(16, np.uint8)
    for shaped in (False, True):
        for transpose in (True, False):
            del calls[:]
            r = rows.reshape(2, 3, 2) if shaped else rows
            b = bm.reshape(2, 3, 2) if shaped else bm
            out = grp.apply_host_grib(buf, r, [2, 0, 1], masked_levels=[1, 0, 1], bitmaps=b, masked=True, remap_area_min=0.5,
                                      transpose=transpose, chunk_outer=4, n_inner=2)
            assert out.shape == ((2, 2, 3, 6) if transpose else (3, 2, 2, 6)) and out.dtype == np.float64
            (name, a), = calls
            assert name == "smm_group_apply_host_grib" and len(a) == len(HOST)
            assert a[2] == 16 and a[6] == _lib.SMM_F64 and a[7:11] == (2, 3, 2, int(transpose))
            assert a[13:] == (0.5, _lib.APPLY_MASKED, 4)
            got_rows = np.ctypeslib.as_array(ctypes.cast(a[3], ctypes.POINTER(ctypes.c_uint64)), shape=(12 * 5,))
            assert got_rows[::5].tolist() == list(range(12))              # C order of (o, l, i)
            got_bm = np.ctypeslib.as_array(ctypes.cast(a[4], ctypes.POINTER(ctypes.c_uint64)), shape=(12 * 2,))
            assert got_bm[1::2].tolist() == list(range(100, 112))
            lev = np.ctypeslib.as_array(ctypes.cast(a[11], ctypes.POINTER(ctypes.c_int32)), shape=(3,))
            ml = np.ctypeslib.as_array(ctypes.cast(a[12], ctypes.POINTER(ctypes.c_uint8)), shape=(3,))
            assert lev.tolist() == [2, 0, 1] and ml.tolist() == [1, 0, 1]
    # no bitmaps, no masked_levels: NULL in their places; n_inner defaults to 1
    del calls[:]
    out = grp.apply_host_grib(buf, rows, [0, 1])
    (name, a), = calls
    assert a[4] is None and a[12] is None and a[7:11] == (6, 2, 1, 1) and out.shape == (6, 1, 2, 6) and a[13:] == (0.0, 0, 0)
    # what does not fit
    with pytest.raises(ValueError, match="whole number"):
        grp.apply_host_grib(buf, rows[:11], [0, 1])
    with pytest.raises(ValueError, match="one entry per data level"):
        grp.apply_host_grib(buf, rows.reshape(2, 3, 2), [0, 1])
    with pytest.raises(ValueError, match="flat or"):
        grp.apply_host_grib(buf, rows.reshape(6, 2), [0, 1])
    with pytest.raises(ValueError, match="bitmaps must be flat or"):
        grp.apply_host_grib(buf, rows.reshape(2, 3, 2), [0, 1, 2], bitmaps=bm.reshape(3, 2, 2))
    with pytest.raises(ValueError, match="bitmap records"):
        grp.apply_host_grib(buf, rows, [0, 1], bitmaps=bm[:5])
    with pytest.raises(ValueError, match="one entry per group member"):
        grp.apply_host_grib(buf, rows, [0, 1], masked_levels=[1, 1])
    with pytest.raises(TypeError, match="uint8"):
        grp.apply_host_grib(buf.astype(np.int8), rows, [0, 1])
    with pytest.raises(ValueError, match="out must be"):
        grp.apply_host_grib(buf, rows, [0, 1], out=np.zeros((6, 2, 6)))
    assert len(calls) == 1
