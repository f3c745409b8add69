"""CF-packed 16-bit RESULTS on the host side: the header's `_pk` entries and their ctypes twins, every refusal that needs
no device, the `cf_out` / `packed_out` keywords, and the `CFEncode` rule on hand-computed cases (no device needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import CFDecode, Regridder, SparseOperator, _lib, gridgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("smm_apply_pk", "smm_apply_sb_pk", "smm_apply_host_pk")


def _code():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        return re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)


def _params(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(p.split()) for p in m.group(1).split(",")]


def test_header_declares_the_pk_entries_as_cf_plus_enc():
    code = _code()
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", code)
    m = re.search(r"typedef\s+struct\s+smm_cf_encode_t\s*\{(.*?)\}\s*smm_cf_encode_t\s*;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "double scale, offset; int32_t fill; int32_t reserved;"
    for name in ENTRIES:
        cf_name = name[:-3] + "_cf"
        assert _params(code, name) == _params(code, cf_name) + ["const smm_cf_encode_t* enc"]


def test_library_exports_and_ctypes_table_lists_the_pk_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][-1] is ctypes.POINTER(_lib.CfEncodeStruct)
        assert _lib.SIGNATURES[name][:-1] == _lib.SIGNATURES[name[:-3] + "_cf"]
    assert ctypes.sizeof(_lib.CfEncodeStruct) == 24
    assert (_lib.CfEncodeStruct.fill.offset, _lib.CfEncodeStruct.reserved.offset) == (16, 20)
    assert _lib.load().smm_abi_version() == 6


def _args(name, x, x_code, y, y_code, flags=0):
    tail = 0 if name == "smm_apply_host_pk" else None          # chunk_rows / stream
    return (None, x.ctypes.data_as(ctypes.c_void_p), x_code, 4, y.ctypes.data_as(ctypes.c_void_p), y_code, 4, 1, 0.0,
            flags, tail)


@pytest.mark.parametrize("name", ENTRIES)
def test_refusals_that_need_no_device(name):
    """Every refusal of the encode rule comes back with a NULL operator handle: nothing has touched a device."""
    lib = _lib.load()
    fn = getattr(lib, name)
    xf, xi = np.zeros(4, np.float64), np.zeros(4, np.int16)
    yf, yi, yu = np.zeros(4, np.float64), np.zeros(4, np.int16), np.zeros(4, np.uint16)
    good = lambda: _lib.CfEncodeStruct(0.01, 250.0, -32768, 0)       # noqa: E731

    def refused(args, cf, enc, code, word):
        rc = fn(*args, None if cf is None else ctypes.byref(cf), None if enc is None else ctypes.byref(enc))
        assert rc == code, (rc, lib.smm_last_error())
        assert word in lib.smm_last_error(), lib.smm_last_error()

    INV, UNS = _lib.SMM_ERR_INVALID, _lib.SMM_ERR_UNSUPPORTED
    refused(_args(name, xf, _lib.SMM_F64, yf, _lib.SMM_F64), None, good(), INV, b"float y_dtype")
    refused(_args(name, xf, _lib.SMM_F64, yf, _lib.SMM_F32), None, good(), INV, b"float y_dtype")
    refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16), None, None, INV, b"encode rule")
    refused(_args(name, xf, _lib.SMM_F64, yu, _lib.SMM_U16), None, None, INV, b"encode rule")
    for y, code, fill in ((yi, _lib.SMM_I16, 40000), (yi, _lib.SMM_I16, -32769), (yu, _lib.SMM_U16, -1),
                          (yu, _lib.SMM_U16, 65536)):
        enc = good()
        enc.fill = fill
        refused(_args(name, xf, _lib.SMM_F64, y, code), None, enc, INV, b"representable")
    for scale in (0.0, -0.0, np.inf, -np.inf, np.nan):
        enc = good()
        enc.scale = scale
        refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16), None, enc, INV, b"scale")
    for offset in (np.inf, -np.inf, np.nan):
        enc = good()
        enc.offset = offset
        refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16), None, enc, INV, b"offset")
    enc = good()
    enc.reserved = 1
    refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16), None, enc, INV, b"reserved")
    # the LDS tile kernel is not built for packed results
    refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16, _lib.APPLY_KERNEL_TILE), None, good(), UNS, b"tile kernel")
    # the refusals of the _cf entry stay in front of the operator too: an integer field without a decode rule
    refused(_args(name, xi, _lib.SMM_I16, yi, _lib.SMM_I16), None, good(), INV, b"decode rule")
    # a valid rule gets as far as the operator check
    refused(_args(name, xf, _lib.SMM_F64, yi, _lib.SMM_I16), None, good(), INV, b"null operator")
    # enc == NULL is the _cf entry unchanged
    refused(_args(name, xf, _lib.SMM_F64, yf, _lib.SMM_F64), None, None, INV, b"null operator")


def test_keywords_exist_with_their_defaults():
    for name in ("apply", "apply_sb", "apply_host"):
        p = inspect.signature(getattr(SparseOperator, name)).parameters
        assert "cf_out" in p and p["cf_out"].default is None, name
    p = inspect.signature(Regridder.__init__).parameters
    assert "packed_out" in p and p["packed_out"].default is False
    assert smmregrid_amd.CFEncode is smmregrid_amd.device.CFEncode and "CFEncode" in smmregrid_amd.__all__


def test_value_errors_of_the_keywords():
    CFEncode = smmregrid_amd.CFEncode
    w = gridgen.bilinear_weights("r24x12", "r12x6")
    with pytest.raises(ValueError, match="packed=True"):
        Regridder(weights=w, packed_out=True)
    with pytest.raises(ValueError, match="float64"):
        Regridder(weights=w, packed=True, packed_out=True, out_dtype=np.float32)
    enc = CFEncode(0.01, 250.0, -32768, np.int16)
    with pytest.raises(ValueError, match="float64"):
        smmregrid_amd.device.result_dtype(np.float32, enc)
    assert smmregrid_amd.device.result_dtype(np.float64, enc) == (np.dtype(np.int16), _lib.SMM_I16)
    assert smmregrid_amd.device.result_dtype(np.float32, None) == (np.dtype(np.float32), _lib.SMM_F32)
    # the check sits in front of everything else in the three methods (no operator, no device needed)
    op = SparseOperator.__new__(SparseOperator)
    op.n_src, op.n_dst, op.n_used_src, op.handle = 4, 4, 4, None
    with pytest.raises(ValueError, match="float64"):
        op.apply_host(np.zeros((2, 4)), out_dtype=np.float32, cf_out=enc)
    for bad in (0.0, np.inf, np.nan):
        with pytest.raises(ValueError):
            CFEncode(bad, 0.0, 0, np.int16)
    for bad in (np.inf, -np.inf, np.nan):
        with pytest.raises(ValueError):
            CFEncode(1.0, bad, 0, np.int16)
    for fill, dt in ((40000, np.int16), (-1, np.uint16), (65536, np.uint16), (1.5, np.int16), (np.nan, np.int16),
                     (None, np.int16)):
        with pytest.raises(ValueError):
            CFEncode(1.0, 0.0, fill, dt)
    with pytest.raises(TypeError):
        CFEncode(1.0, 0.0, 0, np.int32)
    with pytest.raises(ValueError, match="_FillValue"):
        CFEncode.from_attrs({"scale_factor": 0.5}, np.int16)
    assert CFEncode.from_attrs({"missing_value": np.int16(-5)}, np.int16).fill_value == -5
    assert CFEncode.from_attrs({"missing_value": 3, "_FillValue": np.uint16(65535)}, np.uint16).fill_value == 65535
    e = CFEncode.from_attrs({"scale_factor": np.float32(0.5), "add_offset": 2.0, "_FillValue": -32768}, np.int16)
    a = e.attrs()
    assert a == {"scale_factor": 0.5, "add_offset": 2.0, "_FillValue": -32768} and a["_FillValue"].dtype == np.int16
    assert set(CFEncode(None, None, 7, np.uint16).attrs()) == {"_FillValue"}
    st = e._struct()
    assert (st.scale, st.offset, st.fill, st.reserved) == (0.5, 2.0, -32768, 0)
    st = CFEncode(None, None, 7, np.uint16)._struct()
    assert (st.scale, st.offset, st.fill, st.reserved) == (1.0, 0.0, 7, 0)


def test_encode_hand_computed_cases():
    CFEncode = smmregrid_amd.CFEncode
    # scale 0.5, offset 10: y = 10 + t / 2 exactly, so t is what the comments say
    e = CFEncode(0.5, 10.0, -999, np.int16)
    y = np.array([10.25, 10.75, 11.25, 9.75, 9.25,          # t = 0.5, 1.5, 2.5, -0.5, -1.5: ties to even
                  10.0 + (-32768 - 0.5) / 2,                # t = min - 0.5 -> rounds to min (even): kept
                  10.0 + (32767 + 0.5) / 2,                 # t = max + 0.5 -> rounds to 32768: fill
                  10.0 + 32767 / 2, 10.0 - 32768 / 2,       # the ends themselves
                  10.0 + (-32768 - 1.5) / 2,                # t = min - 1.5 -> min - 2: fill
                  np.inf, -np.inf, np.nan, 1e300, -1e300,
                  10.0 - 999 / 2])                          # a valid value that lands on the fill: stored as is
    want = np.array([0, 2, 2, 0, -2, -32768, -999, 32767, -32768, -999, -999, -999, -999, -999, -999, -999], np.int16)
    got = e.encode(y)
    assert got.dtype == np.int16 and np.array_equal(got, want)
    # -0.0 and the smallest magnitudes
    z = CFEncode(None, None, -1, np.int16).encode(np.array([-0.0, 0.0, -0.4, 0.5, -0.5, 5e-324]))
    assert np.array_equal(z, np.zeros(6, np.int16))
    # uint16: t = -0.5 -> -0 -> 0, t = -0.51 -> -1 -> fill; the top end
    u = CFEncode(None, None, 65535, np.uint16)
    got = u.encode(np.array([-0.5, -0.51, 65534.5, 65535.49, 65535.5, 65536.0, 0.5, 1.5, 2.5]))
    assert got.dtype == np.uint16
    assert np.array_equal(got, np.array([0, 65535, 65534, 65535, 65535, 65535, 0, 2, 2], np.uint16))
    # absent scale / offset are 1 / 0, each on its own
    assert np.array_equal(CFEncode(None, 3.0, 0, np.int16).encode([5.5, 6.5]), [2, 4])
    assert np.array_equal(CFEncode(-0.25, None, 0, np.int16).encode([1.0, -0.125, -0.375]), [-4, 0, 2])
    # float32 input is widened first: the arithmetic is float64
    y32 = np.float32([273.15, 250.004])
    assert np.array_equal(CFEncode(0.01, 250.0, -1, np.int16).encode(y32),
                          np.rint((y32.astype(np.float64) - 250.0) / 0.01).astype(np.int16))
    # shape is kept
    assert CFEncode(1.0, 0.0, 0, np.int16).encode(np.zeros((2, 3))).shape == (2, 3)


@pytest.mark.parametrize("raw", [np.int16, np.uint16])
@pytest.mark.parametrize("scale,offset", [(1.0e-3, 2.7e2), (-0.25, 0.0), (0.0019, 254.3), (1.0, -7.0), (3.7e5, 1.0e9)])
def test_round_trip_within_half_a_step(rng, raw, scale, offset):
    """|decode(encode(y)) - y| <= 0.5 |scale| + 4 eps max(|y|, |offset|) for finite in-range y: half a quantisation step
    plus the rounding of the two operations each way."""
    CFEncode = smmregrid_amd.CFEncode
    info = np.iinfo(raw)
    t = rng.uniform(info.min - 0.49, info.max + 0.49, size=20000)
    t[:4] = [info.min, info.max, info.min - 0.49, info.max + 0.49]
    y = t * scale + offset
    fill = int(info.min) if raw == np.int16 else int(info.max)
    enc = CFEncode(scale, offset, fill, raw)
    q = enc.encode(y)
    r = np.rint((y - offset) / scale)
    inr = (r >= info.min) & (r <= info.max)
    assert inr.mean() > 0.999                                   # the bound is checked on (nearly) everything
    back = CFDecode(scale, offset, (), np.float64).decode(q)    # no fill: a value landing on it reads as itself
    eps = np.finfo(np.float64).eps
    bound = 0.5 * abs(scale) + 4 * eps * np.maximum(np.abs(y), abs(offset))
    assert (np.abs(back - y)[inr] <= bound[inr]).all()
    assert (q[~inr] == fill).all()
    # the attributes read back through CFDecode.from_attrs
    cf = CFDecode.from_attrs(enc.attrs(), dtype=np.float64, raw_dtype=raw)
    assert cf.fill_values == (fill,) and (cf.scale_factor, cf.add_offset) == (scale, offset)
