"""Bitmapped GRIB fields kept raw, on the host side: `open_dataset(grb, decode=False, bitmaps=True)` and the `bitmaps` of
its `GribField`, the `GRIB_BITMAP_DTYPE` record, the two `_bm` ABI entries and every refusal of theirs that needs no
device."""
import ctypes
import os
import re

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribField, _lib
from smmregrid_amd.io import open_dataset
from tests.test_grib_raw import grib1_file, grib2_file, same_bits
from tests.test_griblite import encode2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("smm_apply_grib_bm", "smm_apply_host_grib_bm")


def header_code():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as fh:
        return re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)


def test_bitmap_dtype_is_the_struct_field_for_field():
    assert smmregrid_amd.GRIB_BITMAP_DTYPE is GRIB_BITMAP_DTYPE and smmregrid_amd.GRIB_NO_BITMAP == GRIB_NO_BITMAP == 2 ** 64 - 1
    assert {"GRIB_BITMAP_DTYPE", "GRIB_NO_BITMAP"} <= set(smmregrid_amd.__all__)
    assert GRIB_BITMAP_DTYPE.itemsize == 16 == ctypes.sizeof(_lib.GribBitmapStruct)
    names = ("bitmap_off", "n_values")
    assert GRIB_BITMAP_DTYPE.names == names == tuple(n for n, _ in _lib.GribBitmapStruct._fields_)
    assert [GRIB_BITMAP_DTYPE.fields[n][1] for n in names] == [0, 8] == [getattr(_lib.GribBitmapStruct, n).offset for n in names]
    assert [GRIB_BITMAP_DTYPE.fields[n][0] for n in names] == [np.dtype("u8")] * 2
    assert all(t is ctypes.c_uint64 for _, t in _lib.GribBitmapStruct._fields_)
    code = header_code()
    m = re.search(r"typedef\s+struct\s+smm_grib_bitmap_t\s*\{(.*?)\}\s*smm_grib_bitmap_t\s*;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "uint64_t bitmap_off; uint64_t n_values;"
    assert re.search(r"#define\s+SMM_GRIB_NO_BITMAP\s+UINT64_MAX\b", code)
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", code)


def test_header_exports_and_ctypes_table_hold_the_two_bm_entries():
    code = header_code()
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, tail in zip(ENTRIES, ("void* stream", "int64_t chunk_rows")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(params) == 12 == len(_lib.SIGNATURES[name]) and params[-1] == tail
        assert params[3] == "const smm_grib_row_t* rows" and params[4] == "const smm_grib_bitmap_t* bitmaps"
        assert _lib.SIGNATURES[name][3] is ctypes.POINTER(_lib.GribRowStruct)
        assert _lib.SIGNATURES[name][4] is ctypes.POINTER(_lib.GribBitmapStruct)
        # the entry without bitmaps, with `bitmaps` put in behind `rows`
        old = _lib.SIGNATURES[name[:-3]]
        assert _lib.SIGNATURES[name] == old[:4] + [_lib.SIGNATURES[name][4]] + old[4:]
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.load().smm_abi_version() == 6


def _call(name, x, x_bytes, rows, bitmaps, y, y_code=_lib.SMM_F64, ldy=4, n_batch=None, area_min=0.0, flags=0, op=None):
    lib = _lib.load()
    rp = None if rows is None else ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))
    bp = None if bitmaps is None else ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct))
    n = (0 if rows is None else rows.size) if n_batch is None else n_batch
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)     # noqa: E731
    rc = getattr(lib, name)(op, ptr(x), x_bytes, rp, bp, ptr(y), y_code, ldy, n, area_min, flags,
                            0 if "host" in name else None)
    return rc, (lib.smm_last_error() or b"").decode()


@pytest.mark.parametrize("with_bitmaps", [True, False])
@pytest.mark.parametrize("name", ENTRIES)
def test_bm_refusals_that_need_no_device(name, with_bitmaps):
    """The refusals of the entries without bitmaps, with a bitmap table and with NULL in its place: each comes back with a
    NULL operator handle, before any device is touched; a call with nothing to refuse -- and one whose n_values exceeds
    any grid, which only an operator's n_src can tell -- gets as far as the handle."""
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
    rc, msg = _call(name, x, 64, None, bms(), y, n_batch=2)
    assert rc == INV and "null" in msg
    refused(INV, "negative batch", n_batch=-1)
    refused(INV, "x_bytes", x_bytes=-4)
    refused(INV, "remap_area_min", area_min=1.5)
    refused(INV, "unknown apply flag", flags=1 << 20)
    if name == "smm_apply_grib_bm":
        refused(INV, "aligned", x=x.ctypes.data + 1, x_bytes=60)
    refused(INV, "aligned", y=y.ctypes.data + 4)
    for y_code in (_lib.SMM_F32, _lib.SMM_I16, _lib.SMM_F16):
        refused(UNS, "SMM_F64", y_code=y_code)
    for flag in (_lib.APPLY_SKIPNA, _lib.APPLY_KERNEL_TILE, _lib.APPLY_SB_PACKED, _lib.APPLY_HOST_NO_PACK, _lib.APPLY_SB_Y_SB):
        refused(UNS, "not built", flags=flag)
    rows = good(3)
    rows["nbits"], rows["bscale"], rows["ddiv"] = (0, 32, 1), (2.0 ** -1022, 2.0 ** 1023, 1.0), (1.0, 0.1, 1e-300)
    b = bms(3)
    if b is not None:
        b["n_values"][0] = 2 ** 40                         # beyond any grid: refused once the operator says how many cells
    rc, msg = _call(name, x, 64, rows, b, y, flags=_lib.APPLY_MASKED | _lib.APPLY_NO_FILL | _lib.APPLY_KERNEL_SELL)
    assert rc == INV and "null operator" in msg, (rc, msg)


@pytest.mark.parametrize("make", [grib1_file, grib2_file])
def test_open_dataset_keeps_a_bitmapped_variable_raw(tmp_path, rng, make, monkeypatch):
    from smmregrid_amd import griblite
    path = make(tmp_path, rng)
    dec = open_dataset(path)
    file_bytes = np.fromfile(path, dtype=np.uint8)
    calls = []
    real = griblite._unpack_bits
    monkeypatch.setattr(griblite, "_unpack_bits", lambda raw, nbits, count: calls.append(nbits) or real(raw, nbits, count))
    raw = open_dataset(path, decode=False, bitmaps=True)
    assert calls == []                                                   # nothing is unpacked at open
    assert list(raw.data_vars) == list(dec.data_vars) and raw.attrs == dec.attrs
    f, want = raw["sst"].data, dec["sst"].data
    assert isinstance(f, GribField) and f.bitmaps is not None and f.bitmaps.dtype == GRIB_BITMAP_DTYPE
    assert f.bitmaps.size == f.rows.size == 1 and f.shape == want.shape
    assert raw["sst"].dims == dec["sst"].dims and raw["sst"].attrs == dec["sst"].attrs
    assert same_bits(f.decode(), want) and same_bits(np.asarray(f), want) and same_bits(raw["sst"].values, want)
    assert np.isnan(want).any() and len(calls) == 3
    # the offsets point at the bitmap's bytes: the test's own unpackbits on the file
    off, n = int(f.bitmaps["bitmap_off"][0]), int(f.bitmaps["n_values"][0])
    bits = np.unpackbits(file_bytes[off:off + (f.n_points + 7) // 8])[:f.n_points].astype(bool)
    assert np.array_equal(bits, ~np.isnan(want).ravel()) and n == int(bits.sum()) and 0 < n < f.n_points
    assert np.array_equal(f.buf, file_bytes)
    # variables without a bitmap carry no records, and everything is one buffer
    for name in raw.data_vars:
        g = raw[name].data
        assert isinstance(g, GribField) and g.buf is f.buf and same_bits(np.asarray(g), dec[name].data)
        assert (g.bitmaps is None) == (name != "sst")
    # the defaults are what they were: the bitmapped variable decoded at open, with its one unpack
    del calls[:]
    plain = open_dataset(path, decode=False)
    assert len(calls) == 1 and isinstance(plain["sst"].data, np.ndarray) and same_bits(plain["sst"].data, want)
    del calls[:]
    again = open_dataset(path, decode=False, bitmaps=False)
    assert len(calls) == 1 and isinstance(again["sst"].data, np.ndarray)
    assert all(getattr(again[n].data, "bitmaps", None) is None for n in again.data_vars)
    # bitmaps=True without decode=False is the decoded open
    assert isinstance(open_dataset(path, bitmaps=True)["sst"].data, np.ndarray)


def reuse_previous_bitmap(msg, n_points):
    """The GRIB-2 message `msg` of two fields on one bitmap, its second bitmap section replaced by "the bitmap of the
    field before" (indicator 254, six octets)."""
    n_bm = (n_points + 7) // 8
    sec6 = (6 + n_bm).to_bytes(4, "big") + bytes([6, 0])
    first = msg.index(sec6)
    second = msg.index(sec6, first + 1)
    assert msg[first + 6:first + 6 + n_bm] == msg[second + 6:second + 6 + n_bm]
    out = msg[:second] + (6).to_bytes(4, "big") + bytes([6, 254]) + msg[second + 6 + n_bm:]
    return out[:8] + len(out).to_bytes(8, "big") + out[16:]


def test_a_field_that_reuses_the_previous_bitmap_shares_its_offset(tmp_path, rng):
    ni, nj = 24, 13
    grid = dict(template=0, ni=ni, nj=nj, la1=90.0, lo1=0.0, la2=-90.0, lo2=345.0, n_or_dj=15000000)
    sea = rng.random((nj, ni)) > 0.4
    msg = encode2([dict(values=290.0 + rng.standard_normal((nj, ni)), category=3, number=0, bitmap=sea, nbits=14,
                        surface=(160, lev)) for lev in (0, 10)], discipline=10, **grid)
    # a plain level beside them: one variable mixing messages with and without a bitmap
    msg3 = encode2([dict(values=285.0 + rng.standard_normal((nj, ni)), category=3, number=0, nbits=11, surface=(160, 20))],
                   discipline=10, **grid)
    path = tmp_path / "reuse.grib2"
    path.write_bytes(reuse_previous_bitmap(msg, ni * nj) + msg3)
    dec = open_dataset(str(path))["sst"].data
    assert dec.shape == (3, nj, ni) and np.array_equal(np.isnan(dec[0]), ~sea) and np.array_equal(np.isnan(dec[1]), ~sea)
    f = open_dataset(str(path), decode=False, bitmaps=True)["sst"].data
    assert isinstance(f, GribField) and f.rows.size == 3 and f.bitmaps.size == 3
    assert f.bitmaps["bitmap_off"][0] == f.bitmaps["bitmap_off"][1] != GRIB_NO_BITMAP
    assert f.bitmaps["bitmap_off"][2] == GRIB_NO_BITMAP and f.bitmaps["n_values"].tolist() == [int(sea.sum())] * 2 + [ni * nj]
    assert f.rows["byte_off"][0] != f.rows["byte_off"][1] and same_bits(f.decode(), dec)
    # without bitmaps=True the whole variable is decoded at open
    assert isinstance(open_dataset(str(path), decode=False)["sst"].data, np.ndarray)


def test_a_missing_slot_still_forces_the_eager_decode(tmp_path, rng):
    ni, nj = 24, 13
    grid = dict(template=0, ni=ni, nj=nj, la1=90.0, lo1=0.0, la2=-90.0, lo2=345.0, n_or_dj=15000000)
    sea = rng.random((nj, ni)) > 0.4
    field = lambda lev, step: dict(values=290.0 + rng.standard_normal((nj, ni)), category=3, number=0, bitmap=sea,   # noqa: E731
                                   nbits=14, surface=(160, lev), step=step)
    path = tmp_path / "hole.grib2"
    path.write_bytes(encode2([field(0, 0), field(10, 0)], discipline=10, **grid) + encode2([field(0, 6)], discipline=10, **grid))
    raw = open_dataset(str(path), decode=False, bitmaps=True)["sst"].data
    dec = open_dataset(str(path))["sst"].data
    assert isinstance(raw, np.ndarray) and raw.shape == (2, 2, nj, ni) and np.isnan(raw[1, 1]).all() and same_bits(raw, dec)


def test_gribfield_checks_its_bitmap_records():
    rows = np.zeros(2, GRIB_ROW_DTYPE)
    with pytest.raises(ValueError, match="bitmap records"):
        GribField(np.zeros(8, np.uint8), rows, (2, 4), 4, bitmaps=np.zeros(3, GRIB_BITMAP_DTYPE))
    assert GribField(np.zeros(8, np.uint8), rows, (2, 4), 4).bitmaps is None
