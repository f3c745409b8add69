"""GRIB simple-packed fields kept raw, on the host side: `open_dataset(grb, decode=False)` and its `GribField`, the
`GRIB_ROW_DTYPE` record, the two ABI entries and every refusal of theirs that needs no device."""
import ctypes
import os
import re

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import GRIB_ROW_DTYPE, GribField, _lib
from smmregrid_amd.io import open_dataset
from tests import grib_cases
from tests.test_griblite import encode, encode2

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("smm_apply_grib", "smm_apply_host_grib")


def same_bits(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return a.shape == b.shape and a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))


def grib1_file(tmp_path, rng):
    """Edition 1: two times x three levels of temperature at 24 bits, a 12-bit surface field with D = 1, a 7-bit one with
    D = -1, and a bitmapped sea-surface temperature."""
    ni, nj = 36, 19
    grid = (0, ni, nj, 90, 0, -90, 350, 10000)
    msgs = []
    for day in (1, 2):
        for k, lev in enumerate((850, 500, 250)):
            f = 250.0 + rng.standard_normal((nj, ni)) * 20 - 10.0 * k + day
            msgs.append(encode(f, *grid, param=130, level_type=100, level=lev, date=(2021, 3, day, 12), nbits=24))
    msgs.append(encode(280.0 + rng.standard_normal((nj, ni)), *grid, param=167, nbits=12, decimal=1))
    msgs.append(encode(1.0e5 + 3000 * rng.standard_normal((nj, ni)), *grid, param=151, nbits=7, decimal=-1))
    msgs.append(encode(290.0 + rng.standard_normal((nj, ni)), *grid, param=34, bitmap=rng.random((nj, ni)) > 0.3, nbits=12))
    path = tmp_path / "raw1.grib"
    path.write_bytes(b"".join(msgs))
    return str(path)


def grib2_file(tmp_path, rng):
    """Edition 2: two levels x two times of temperature at 12 bits with D = 1 (several fields per message), a 17-bit
    2 m temperature, a constant (0-bit) pressure field and a bitmapped field."""
    ni, nj = 24, 13
    grid = dict(template=0, ni=ni, nj=nj, la1=90.0, lo1=0.0, la2=-90.0, lo2=345.0, n_or_dj=15000000)
    msgs = []
    for step in (0, 6):
        msgs.append(encode2([dict(values=220.0 + 30 * rng.random((nj, ni)) + lev / 1e4, category=0, number=0,
                                  surface=(100, lev), nbits=12, decimal=1, step=step) for lev in (85000, 50000)], **grid))
    msgs.append(encode2([dict(values=280.0 + rng.standard_normal((nj, ni)), category=0, number=0, surface=(103, 2), nbits=17),
                         dict(values=np.full((nj, ni), 101325.0), category=3, number=0, nbits=0)], **grid))
    msgs.append(encode2([dict(values=290.0 + rng.standard_normal((nj, ni)), category=3, number=0,
                              bitmap=rng.random((nj, ni)) > 0.4, nbits=14)], discipline=10, **grid))
    path = tmp_path / "raw2.grib2"
    path.write_bytes(b"".join(msgs))
    return str(path)


@pytest.mark.parametrize("make,bitmapped,expect", [
    (grib1_file, "sst", {"t": (6, {24}), "t2m": (1, {12}), "msl": (1, {7})}),
    (grib2_file, "sst", {"t": (4, {12}), "t2m": (1, {17}), "sp": (1, {0})})])
def test_open_dataset_decode_false_keeps_the_bits_and_decodes_to_the_same_field(tmp_path, rng, make, bitmapped, expect):
    path = make(tmp_path, rng)
    dec, raw = open_dataset(path), open_dataset(path, decode=False)
    assert list(raw.data_vars) == list(dec.data_vars) and raw.attrs == dec.attrs
    file_bytes = np.fromfile(path, dtype=np.uint8)
    ddivs = set()
    for name, (n_rows, widths) in expect.items():
        f, want = raw[name].data, dec[name].data
        assert isinstance(f, GribField) and isinstance(want, np.ndarray)
        assert f.shape == want.shape and f.dtype == np.float32 and f.ndim == want.ndim
        assert raw[name].dims == dec[name].dims and raw[name].attrs == dec[name].attrs
        assert list(raw[name].coords) == list(dec[name].coords)
        assert f.rows.dtype == GRIB_ROW_DTYPE and f.rows.size == n_rows and set(f.rows["nbits"].tolist()) == widths
        assert (f.rows["reserved"] == 0).all()
        assert f.buf.dtype == np.uint8 and np.array_equal(f.buf, file_bytes)
        assert same_bits(f.decode(), want) and same_bits(np.asarray(f), want) and same_bits(raw[name].values, want)
        # the test's own decoder on the row table: Python-integer extraction + the numpy statement
        mine = grib_cases.decode_rows(f.buf, f.rows, f.n_points).reshape(want.shape)
        assert same_bits(mine, want)
        ddivs |= set(f.rows["ddiv"].tolist())
    assert len({id(raw[n].data.buf) for n in expect}) == 1          # one buffer shared by the file's variables
    assert ddivs >= {1.0, 10.0}
    # a bitmapped variable comes back decoded, NaN where the bitmap says so
    b = raw[bitmapped].data
    assert isinstance(b, np.ndarray) and same_bits(b, dec[bitmapped].data) and np.isnan(b).any()


def test_a_missing_time_level_slot_is_decoded_eagerly(tmp_path, rng):
    ni, nj = 36, 19
    grid = (0, ni, nj, 90, 0, -90, 350, 10000)
    f = lambda: 250.0 + rng.standard_normal((nj, ni))     # noqa: E731
    msgs = [encode(f(), *grid, param=130, level_type=100, level=850, date=(2021, 3, 1, 12)),
            encode(f(), *grid, param=130, level_type=100, level=500, date=(2021, 3, 1, 12)),
            encode(f(), *grid, param=130, level_type=100, level=850, date=(2021, 3, 2, 12))]
    path = tmp_path / "hole.grib"
    path.write_bytes(b"".join(msgs))
    raw = open_dataset(str(path), decode=False)["t"].data
    assert isinstance(raw, np.ndarray) and raw.shape == (2, 2, nj, ni) and np.isnan(raw[1, 0]).all()


def test_row_dtype_is_the_struct_field_for_field():
    assert smmregrid_amd.GRIB_ROW_DTYPE is GRIB_ROW_DTYPE and "GRIB_ROW_DTYPE" in smmregrid_amd.__all__
    assert GRIB_ROW_DTYPE.itemsize == 40 == ctypes.sizeof(_lib.GribRowStruct)
    names = ("byte_off", "ref", "bscale", "ddiv", "nbits", "reserved")
    assert GRIB_ROW_DTYPE.names == names == tuple(n for n, _ in _lib.GribRowStruct._fields_)
    assert [GRIB_ROW_DTYPE.fields[n][1] for n in names] == [0, 8, 16, 24, 32, 36]
    assert [getattr(_lib.GribRowStruct, n).offset for n in names] == [0, 8, 16, 24, 32, 36]
    assert [GRIB_ROW_DTYPE.fields[n][0] for n in names] == [np.dtype(t) for t in ("u8", "f8", "f8", "f8", "i4", "i4")]
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as fh:
        code = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    m = re.search(r"typedef\s+struct\s+smm_grib_row_t\s*\{(.*?)\}\s*smm_grib_row_t\s*;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == \
        "uint64_t byte_off; double ref; double bscale; double ddiv; int32_t nbits; int32_t reserved;"
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", code)


def test_header_exports_and_ctypes_table_hold_the_two_entries():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as fh:
        code = re.sub(r"/\*.*?\*/", "", fh.read(), flags=re.S)
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, tail in zip(ENTRIES, ("void* stream", "int64_t chunk_rows")):
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared"
        params = [" ".join(p.split()) for p in m.group(1).split(",")]
        assert len(params) == 11 == len(_lib.SIGNATURES[name]) and params[-1] == tail
        assert params[3] == "const smm_grib_row_t* rows" and _lib.SIGNATURES[name][3] is ctypes.POINTER(_lib.GribRowStruct)
        assert hasattr(lib, name), f"{name} is not exported"
    assert _lib.load().smm_abi_version() == 6


def _call(name, x, x_bytes, rows, y, y_code=_lib.SMM_F64, ldy=4, n_batch=None, area_min=0.0, flags=0, op=None):
    lib = _lib.load()
    rp = None if rows is None else ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))
    n = (0 if rows is None else rows.size) if n_batch is None else n_batch
    ptr = lambda a: None if a is None else (a if isinstance(a, int) else a.ctypes.data)     # noqa: E731
    rc = getattr(lib, name)(op, ptr(x), x_bytes, rp, ptr(y), y_code, ldy, n, area_min, flags,
                            0 if name.endswith("host_grib") else None)
    return rc, (lib.smm_last_error() or b"").decode()


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_that_need_no_device(name):
    """Every refusal of the row rules and of the call's own arguments comes back with a NULL operator handle, before any
    device is touched, with a message; a call with nothing to refuse gets as far as the handle."""
    x = np.zeros(64, np.uint8)
    y = np.zeros(8, np.float64)

    def good(n=2):
        rows = np.zeros(n, GRIB_ROW_DTYPE)
        rows["bscale"], rows["ddiv"], rows["nbits"] = 0.25, 10.0, 16
        rows["ref"] = -3.5
        return rows

    INV, UNS = _lib.SMM_ERR_INVALID, _lib.SMM_ERR_UNSUPPORTED

    def refused(code, word, rows=None, **kw):
        args = dict(x=x, x_bytes=64, rows=good() if rows is None else rows, y=y)
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
    rc, msg = _call(name, x, 64, None, y, n_batch=2)
    assert rc == INV and "null" in msg
    refused(INV, "negative batch", n_batch=-1)
    refused(INV, "x_bytes", x_bytes=-4)
    refused(INV, "remap_area_min", area_min=1.5)
    refused(INV, "unknown apply flag", flags=1 << 20)
    if name == "smm_apply_grib":                      # device bytes are read as 32-bit words
        refused(INV, "aligned", x=x.ctypes.data + 1, x_bytes=60)
    refused(INV, "aligned", y=y.ctypes.data + 4)
    for y_code in (_lib.SMM_F32, _lib.SMM_I16, _lib.SMM_F16):
        refused(UNS, "SMM_F64", y_code=y_code)
    for flag in (_lib.APPLY_SKIPNA, _lib.APPLY_KERNEL_TILE, _lib.APPLY_SB_PACKED, _lib.APPLY_HOST_NO_PACK, _lib.APPLY_SB_Y_SB):
        refused(UNS, "not built", flags=flag)
    # nothing to refuse: the widest and the narrowest rule, every accepted flag -- the call reaches the handle, which no
    # GPU-less host can have created (the byte-range and ldy refusals, which need an operator's sizes, are tested in
    # tests/cpp/grib_harness.cpp and on the GPU)
    rows = good(3)
    rows["nbits"], rows["bscale"], rows["ddiv"] = (0, 32, 1), (2.0 ** -1022, 2.0 ** 1023, 1.0), (1.0, 0.1, 1e-300)
    rc, msg = _call(name, x, 64, rows, y, flags=_lib.APPLY_MASKED | _lib.APPLY_NO_FILL | _lib.APPLY_KERNEL_SELL)
    assert rc == INV and "null operator" in msg, (rc, msg)


@pytest.mark.parametrize("make", [grib1_file, grib2_file])
def test_decode_false_unpacks_nothing_of_a_raw_kept_variable(tmp_path, rng, make, monkeypatch):
    """Opening with decode=False runs the numpy unpack only for what cannot stay raw (the bitmapped message); the
    raw-kept variables are unpacked when, and only when, somebody asks for their values."""
    from smmregrid_amd import griblite
    path = make(tmp_path, rng)
    n_msgs = len(griblite.read_messages(path))
    calls = []
    real = griblite._unpack_bits
    monkeypatch.setattr(griblite, "_unpack_bits", lambda raw, nbits, count: calls.append(nbits) or real(raw, nbits, count))
    raw = open_dataset(path, decode=False)
    assert len(calls) == 1 and isinstance(raw["sst"].data, np.ndarray)          # the one bitmapped message
    kept = [n for n in raw.data_vars if isinstance(raw[n].data, GribField)]
    assert sum(raw[n].data.rows.size for n in kept) == n_msgs - 1
    del calls[:]
    t = raw["t"].data
    t.decode()
    assert len(calls) == t.rows.size                                            # its own messages, nobody else's
    del calls[:]
    open_dataset(path)
    assert len(calls) == n_msgs
