"""CF-packed 16-bit RESULTS on masked-level (3-D) weights, host side: the three `smm_group_apply*_pk` entries in the
header, the built library and the ctypes table, the refusals that need no device, and the Python keywords."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from smmregrid_amd import OperatorGroup, Regridder, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"smm_group_apply_pk": "smm_group_apply_cf", "smm_group_apply_sb_pk": "smm_group_apply_sb_cf",
           "smm_group_apply_host_pk": "smm_group_apply_host_cf"}


def _header():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        return f.read()


def _declaration(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_group_pk_entries():
    text = _header()
    assert "Level groups have no _pk entries" not in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, twin in ENTRIES.items():
        args = _declaration(code, name)
        assert args[-1] == "const smm_cf_encode_t* enc", name
        assert args[:-1] == _declaration(code, twin), f"{name} is {twin} plus the encode rule"
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", text)       # entries are only added


def test_library_exports_and_ctypes_table_lists_the_group_pk_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, twin in ENTRIES.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][-1] is ctypes.POINTER(_lib.CfEncodeStruct)
        assert _lib.SIGNATURES[name][:-1] == _lib.SIGNATURES[twin]
    assert _lib.load().smm_abi_version() == 6
    assert len(_lib.HOST_STATS) == 12            # D2H_BYTES simply counts 2 B per cell: no new slot


def test_encode_rule_is_validated_before_anything_touches_a_device():
    """With a null group handle every refusal of the rule comes back SMM_ERR_INVALID: make_enc runs first."""
    lib = _lib.load()
    x = np.zeros(4, np.float64)
    yi = np.zeros(4, np.int16)
    yf = np.zeros(4, np.float64)
    lev = np.zeros(1, np.int32)
    xp, lp = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, lev))
    native = lambda y, dt, enc: lib.smm_group_apply_pk(None, xp, _lib.SMM_F64, 4, 4, 4, y.ctypes.data_as(ctypes.c_void_p),
                                                       dt, 4, 4, 4, 1, 1, 1, lp, None, 0.0, 0, None, None, enc)
    sb = lambda y, dt, enc: lib.smm_group_apply_sb_pk(None, xp, _lib.SMM_F64, 4, 1, y.ctypes.data_as(ctypes.c_void_p), dt,
                                                      4, 4, 1, 1, lp, None, 0.0, 0, None, None, enc)
    host = lambda y, dt, enc: lib.smm_group_apply_host_pk(None, xp, _lib.SMM_F64, y.ctypes.data_as(ctypes.c_void_p), dt,
                                                          1, 1, 1, 1, lp, None, 0.0, 0, 0, None, enc)
    ok = _lib.CfEncodeStruct(0.25, 1.0, -32768, 0)
    for call in (native, sb, host):
        assert call(yf, _lib.SMM_F64, ctypes.byref(ok)) == _lib.SMM_ERR_INVALID         # enc with a float y_dtype
        assert b"float y_dtype" in lib.smm_last_error()
        assert call(yi, _lib.SMM_I16, None) == _lib.SMM_ERR_INVALID                      # integer Y without enc
        assert b"encode rule" in lib.smm_last_error()
        assert call(yi, _lib.SMM_U16, ctypes.byref(_lib.CfEncodeStruct(0.25, 1.0, -1, 0))) == _lib.SMM_ERR_INVALID
        assert b"representable" in lib.smm_last_error()                                  # -1 is no uint16
        assert call(yi, _lib.SMM_I16, ctypes.byref(_lib.CfEncodeStruct(0.0, 1.0, -32768, 0))) == _lib.SMM_ERR_INVALID
        assert b"scale" in lib.smm_last_error()
        assert call(yi, _lib.SMM_I16, ctypes.byref(_lib.CfEncodeStruct(0.25, 1.0, -32768, 1))) == _lib.SMM_ERR_INVALID
        assert b"reserved" in lib.smm_last_error()
        assert call(yi, _lib.SMM_I16, ctypes.byref(_lib.CfEncodeStruct(float("nan"), 1.0, 0, 0))) == _lib.SMM_ERR_INVALID
        assert call(yi, _lib.SMM_I16, ctypes.byref(_lib.CfEncodeStruct(0.25, float("inf"), 0, 0))) == _lib.SMM_ERR_INVALID
        # a valid rule gets as far as the group handle
        assert call(yi, _lib.SMM_I16, ctypes.byref(ok)) == _lib.SMM_ERR_INVALID
        assert b"null group" in lib.smm_last_error()


def test_keywords_exist():
    for name in ("apply", "apply_sb", "apply_host"):
        p = inspect.signature(getattr(OperatorGroup, name)).parameters
        assert "cf_out" in p and p["cf_out"].default is None, name
    p = inspect.signature(Regridder.__init__).parameters
    assert "packed_out_levels" in p and p["packed_out_levels"].default is False
    assert "cf_out" in inspect.signature(Regridder.regrid3d).parameters


def test_packed_out_levels_needs_packed_out():
    """`packed_out_levels` only widens what `packed_out=True` encodes in the kernels: alone it is a mistake, refused
    before any weights are read."""
    with pytest.raises(ValueError, match="packed_out_levels"):
        Regridder(weights="no_such_file.nc", packed_out_levels=True)
    with pytest.raises(ValueError, match="packed_out_levels"):
        Regridder(weights="no_such_file.nc", packed=True, packed_out_levels=True)
    with pytest.raises(ValueError, match="packed_out_levels"):
        Regridder(weights="no_such_file.nc", packed=True, packed_levels=True, packed_out=False, packed_out_levels=True)
