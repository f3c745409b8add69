"""smm_group_apply_host_grib_pk, host side: the entry in the header, the exports and the ctypes table, the refusals of its
result side that need no group -- they come first, whatever the handle -- the switches of `Regridder(grib_out_levels=)`
and the argument shaping of `OperatorGroup.apply_host_grib(grib_out=)`.  The library is loaded; no device is touched.
out_bytes below the layout and a level_index outside the group need the group's sizes, and a group exists only on a
device: those two are refused in tests/test_gpu_grib_out_levels.py, in the same order."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ENCODE_DTYPE, GRIB_ROW_DTYPE, GribEncode, GribField, Regridder, _lib
from tests.test_grib_levels_raw import fake_group, header_code

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "smm_group_apply_host_grib_pk"
_p, _i64, _dbl, _uint = ctypes.c_void_p, ctypes.c_int64, ctypes.c_double, ctypes.c_uint
_grp, _gbp, _gep = (ctypes.POINTER(_lib.GribRowStruct), ctypes.POINTER(_lib.GribBitmapStruct),
                    ctypes.POINTER(_lib.GribEncodeStruct))
# parameter by parameter: (C declaration, ctypes type)
PARAMS = [("smm_group_t g", _p), ("const void* x_host", _p), ("int64_t x_bytes", _i64), ("const smm_grib_row_t* rows", _grp),
          ("const smm_grib_bitmap_t* bitmaps", _gbp), ("const smm_grib_encode_t* enc", _gep), ("void* out_host", _p),
          ("int64_t out_bytes", _i64), ("smm_grib_row_t* rows_out", _grp), ("smm_grib_bitmap_t* bitmaps_out", _gbp),
          ("int64_t n_outer", _i64), ("int64_t n_lev", _i64), ("int64_t n_inner", _i64), ("const int32_t* level_index", _p),
          ("const uint8_t* masked_levels", _p), ("double remap_area_min", _dbl), ("unsigned flags", _uint),
          ("int64_t chunk_outer", _i64)]


def test_header_export_and_ctypes_table_agree():
    m = re.search(r"\bint\s+" + NAME + r"\s*\(([^;]*?)\)\s*;", header_code(), flags=re.S)
    assert m, f"{NAME} is not declared"
    assert [" ".join(p.split()) for p in m.group(1).split(",")] == [decl for decl, _ in PARAMS]
    assert _lib.SIGNATURES[NAME] == [t for _, t in PARAMS]
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), NAME), f"{NAME} is not exported"
    assert getattr(_lib.load(), NAME).argtypes == [t for _, t in PARAMS]


def test_the_abi_version_stays_6():
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", header_code()) and _lib.load().smm_abi_version() == 6


def _enc(nbits=16, ddiv=1.0, reserved=0, n=2):
    rec = np.zeros(n, dtype=GRIB_ENCODE_DTYPE)
    rec["ddiv"], rec["nbits"], rec["reserved"] = ddiv, nbits, reserved
    return rec


def call_entry(group=None, enc="good", out="good", out_bytes=None, rows_out="good", bitmaps_out="good", rows="good",
               shape=(1, 2, 1), level_index=(0, 0), flags=0, area_min=0.0, x_bytes=64):
    """The entry with host arrays that are never followed without a group.  Returns (status, message)."""
    n = max(int(np.prod(shape)), 1)
    x = np.zeros(64, np.uint8)
    if isinstance(rows, str):
        rows = np.zeros(n, GRIB_ROW_DTYPE)
        rows["bscale"], rows["ddiv"], rows["nbits"] = 0.25, 10.0, 16
    enc = _enc(n=n) if isinstance(enc, str) else enc
    out = np.zeros(1 << 12, np.uint8) if isinstance(out, str) else out
    rows_out = np.zeros(n, GRIB_ROW_DTYPE) if isinstance(rows_out, str) else rows_out
    bitmaps_out = np.zeros(n, GRIB_BITMAP_DTYPE) if isinstance(bitmaps_out, str) else bitmaps_out
    lev = np.asarray(level_index, np.int32)
    cast = lambda a, t: None if a is None else ctypes.cast(a.ctypes.data, t)      # noqa: E731
    lib = _lib.load()
    rc = getattr(lib, NAME)(group, x.ctypes.data, x_bytes, cast(rows, _grp), None, cast(enc, _gep),
                            None if out is None else out.ctypes.data,
                            (0 if out is None else out.size) if out_bytes is None else out_bytes,
                            cast(rows_out, _grp), cast(bitmaps_out, _gbp), *shape, lev.ctypes.data, None, area_min, flags, 0)
    return rc, (lib.smm_last_error() or b"").decode()


def test_the_result_side_is_refused_first_and_without_a_device():
    """On a NULL group: every refusal of the encode records and of the record pointers answers before the handle, the
    row rules or the flags are looked at; then the refusals of smm_group_apply_host_grib follow in their order, the NULL
    group among them."""
    INV, UNS = _lib.SMM_ERR_INVALID, _lib.SMM_ERR_UNSUPPORTED
    bad_rows = np.zeros(2, GRIB_ROW_DTYPE)                            # bscale 0: a refusal of the group entry, which comes later
    bad_flags = 1 << 20

    def refused(word, **kw):
        for more in (dict(), dict(rows=bad_rows), dict(flags=bad_flags), dict(flags=_lib.APPLY_KERNEL_TILE)):
            rc, msg = call_entry(**kw, **more)
            assert rc == INV and word in msg, (kw, more, rc, msg)

    refused("null encode, row or bitmap record pointer", enc=None)
    refused("null encode, row or bitmap record pointer", rows_out=None)
    refused("null encode, row or bitmap record pointer", bitmaps_out=None)
    for nbits in (0, 33):
        refused("enc[0].nbits", enc=_enc(nbits=nbits))
    for ddiv in (0.0, np.inf, np.nan, -10.0):
        refused("enc[0].ddiv", enc=_enc(ddiv=ddiv))
    refused("enc[0].reserved", enc=_enc(reserved=1))
    second = _enc()
    second["nbits"][1] = 40
    refused("enc[1].nbits", enc=second)
    refused("negative out_bytes", out_bytes=-1)
    for shape in ((-1, 2, 1), (1, -2, 1), (1, 2, -1)):
        refused("negative batch", shape=shape)
    # a null out_host: the layout needs the group's n_dst, so without a group the handle is what is refused
    rc, msg = call_entry(out=None)
    assert rc == INV and "null group" in msg, (rc, msg)
    # ... then the group entry's own, in its order: flags, what is not built, pointers, rules, the handle
    rc, msg = call_entry(flags=bad_flags, rows=bad_rows)
    assert rc == INV and "unknown apply flag" in msg, (rc, msg)
    rc, msg = call_entry(flags=_lib.APPLY_KERNEL_TILE, rows=bad_rows)
    assert rc == UNS and "not built" in msg, (rc, msg)
    rc, msg = call_entry(flags=_lib.APPLY_SKIPNA | _lib.APPLY_NO_FILL)    # the flag road is the _na entry
    assert rc == INV, (rc, msg)
    rc, msg = call_entry(rows=None)
    assert rc == INV and "null" in msg, (rc, msg)
    rc, msg = call_entry(rows=bad_rows)
    assert rc == INV and "rows[0].bscale" in msg, (rc, msg)
    rc, msg = call_entry(area_min=1.5)
    assert rc == INV and "remap_area_min" in msg, (rc, msg)
    for flags in (0, _lib.APPLY_SKIPNA, _lib.APPLY_MASKED | _lib.APPLY_KERNEL_SELL):
        rc, msg = call_entry(flags=flags, level_index=(7, -1))
        assert rc == INV and "null group" in msg, (rc, msg)
    rc, msg = call_entry(shape=(0, 2, 1), enc=None, rows_out=None, bitmaps_out=None)     # an empty call gets to the handle
    assert rc == INV and "null group" in msg, (rc, msg)


def test_regridder_grib_out_levels_needs_grib_out_and_packed_levels():
    """In the wording of the packed_out_levels refusal; the Regridder refuses before it looks at its weights."""
    assert inspect.signature(Regridder.__init__).parameters["grib_out_levels"].default is False
    for kw in (dict(packed=True, packed_levels=True), dict(packed=True, grib_out=True)):
        with pytest.raises(ValueError, match="grib_out_levels=True needs grib_out=True and packed_levels=True"):
            Regridder(weights=object(), grib_out_levels=True, **kw)
    for kw in (dict(), dict(grib_out=True, packed_levels=True),
               dict(packed=True, packed_levels=True, grib_out=True, lazy=True)):
        with pytest.raises(ValueError):              # what grib_out and packed_levels need themselves comes first
            Regridder(weights=object(), grib_out_levels=True, **kw)


def test_apply_host_grib_grib_out_shapes_its_arguments(monkeypatch):
    """What reaches the entry, parameter by parameter; the GribField over `out` or a fresh buffer; transpose=False and a
    short or mistyped `out` are ValueErrors before any call."""
    grp = fake_group()                                                # 3 members, n_src 40, n_dst 6
    calls = []
    monkeypatch.setattr(_lib, "call", lambda name, *a: calls.append((name, a)))
    rows = np.zeros(2 * 3 * 2, GRIB_ROW_DTYPE)
    rows["byte_off"] = np.arange(12)
    bm = np.zeros(12, GRIB_BITMAP_DTYPE)
    buf = np.zeros(16, np.uint8)
    enc = GribEncode([16, 12, 7] * 4, [0, 1, 2] * 4)
    _, total = enc.layout(6, 12)
    for skipna in (False, True):
        for out in (None, np.zeros(total + 5, np.uint8)):
            del calls[:]
            got = grp.apply_host_grib(buf, rows.reshape(2, 3, 2), [2, 0, 1], masked_levels=[1, 0, 1], bitmaps=bm, out=out,
                                      masked=True, remap_area_min=0.5, chunk_outer=4, skipna=skipna, grib_out=enc)
            assert isinstance(got, GribField) and got.shape == (2, 3, 2, 6) and got.n_points == 6
            assert got.bitmaps is not None and got.rows.size == 12 and (out is None or got.buf is out)
            assert got.buf.dtype == np.uint8 and got.buf.size >= total
            (name, a), = calls
            assert name == NAME and len(a) == len(PARAMS)
            assert a[2] == 16 and a[7] == got.buf.size and a[10:13] == (2, 3, 2)
            assert a[15:] == (0.5, _lib.APPLY_MASKED | (_lib.APPLY_SKIPNA if skipna else 0), 4)
            rec = np.ctypeslib.as_array(ctypes.cast(a[5], ctypes.POINTER(ctypes.c_uint8)), shape=(12 * 16,))
            assert rec.tobytes() == enc.records(12).tobytes()
            lev = np.ctypeslib.as_array(ctypes.cast(a[13], ctypes.POINTER(ctypes.c_int32)), shape=(3,))
            assert lev.tolist() == [2, 0, 1]
    del calls[:]
    with pytest.raises(ValueError, match="transpose=False"):
        grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2, transpose=False, grib_out=enc)
    with pytest.raises(ValueError, match="at least"):
        grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2, out=np.zeros(total - 1, np.uint8), grib_out=enc)
    with pytest.raises(ValueError, match="at least"):
        grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2, out=np.zeros((total,), np.int8), grib_out=enc)
    with pytest.raises(ValueError, match="12 fields"):
        grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2, grib_out=GribEncode([16, 12]))
    assert not calls
    # without grib_out nothing changed: the float entry, its result array
    out = grp.apply_host_grib(buf, rows, [2, 0, 1], n_inner=2)
    assert calls[0][0] == "smm_group_apply_host_grib" and out.shape == (2, 2, 3, 6) and out.dtype == np.float64
