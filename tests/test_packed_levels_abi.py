"""CF-packed 16-bit fields on masked-level (3-D) weights, host side: the three `smm_group_apply*_cf` entries in the
header, the built library and the ctypes table, and the Python keywords (no device needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from smmregrid_amd import OperatorGroup, Regridder, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"smm_group_apply_cf": "smm_group_apply", "smm_group_apply_sb_cf": "smm_group_apply_sb",
           "smm_group_apply_host_cf": "smm_group_apply_host"}


def _header():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        return f.read()


def _declaration(code, name):
    m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
    assert m, f"{name} is not declared"
    return [" ".join(a.split()) for a in m.group(1).split(",")]


def test_header_declares_the_group_cf_entries():
    text = _header()
    assert "Level groups take no packed input" not in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name, plain in ENTRIES.items():
        args = _declaration(code, name)
        assert args[-1] == "const smm_cf_decode_t* cf", name
        assert args[:-1] == _declaration(code, plain), f"{name} is {plain} plus the decode rule"
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", text)       # entries are only added


def test_library_exports_and_ctypes_table_lists_the_group_cf_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name, plain in ENTRIES.items():
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][-1] is ctypes.POINTER(_lib.CfDecodeStruct)
        assert _lib.SIGNATURES[name][:-1] == _lib.SIGNATURES[plain]
    assert _lib.load().smm_abi_version() == 6
    assert len(_lib.HOST_STATS) == 12            # the byte counts of the packed group pipeline are the existing two


def test_decode_rule_is_validated_before_anything_touches_a_device():
    lib = _lib.load()
    st = _lib.CfDecodeStruct(1.0, 0.0, (ctypes.c_int32 * 2)(-1, 0), 1, _lib.SMM_F32)
    x = np.zeros(4, np.uint16)
    y = np.zeros(4, np.float64)
    lev = np.zeros(1, np.int32)
    xp, yp, lp = (a.ctypes.data_as(ctypes.c_void_p) for a in (x, y, lev))
    native = lambda dt, fl, cf: lib.smm_group_apply_cf(None, xp, dt, 4, 4, 4, yp, _lib.SMM_F64, 4, 4, 4, 1, 1, 1, lp,
                                                       None, 0.0, fl, None, cf)
    sb = lambda dt, fl, cf: lib.smm_group_apply_sb_cf(None, xp, dt, 4, 1, yp, _lib.SMM_F64, 4, 4, 1, 1, lp, None, 0.0,
                                                      fl, None, cf)
    host = lambda dt, fl, cf: lib.smm_group_apply_host_cf(None, xp, dt, yp, _lib.SMM_F64, 1, 1, 1, 1, lp, None, 0.0,
                                                          fl, 0, cf)
    for call in (native, sb, host):
        assert call(_lib.SMM_U16, 0, ctypes.byref(st)) == _lib.SMM_ERR_INVALID        # -1 is no uint16
        assert b"representable" in lib.smm_last_error()
        assert call(_lib.SMM_U16, 0, None) == _lib.SMM_ERR_INVALID                     # integer field, no rule
        assert call(_lib.SMM_F32, 0, ctypes.byref(st)) == _lib.SMM_ERR_INVALID        # a rule with a float field
        st.fill[0] = 65535
        assert call(_lib.SMM_U16, _lib.APPLY_NO_FILL, ctypes.byref(st)) == _lib.SMM_ERR_INVALID   # NO_FILL with a fill
        st.fill[0] = -1


def test_keywords_exist():
    for name in ("apply", "apply_sb", "apply_host"):
        p = inspect.signature(getattr(OperatorGroup, name)).parameters
        assert "cf" in p and p["cf"].default is None, name
    p = inspect.signature(Regridder.__init__).parameters
    assert "packed_levels" in p and p["packed_levels"].default is False
    assert "cf" in inspect.signature(Regridder.regrid3d).parameters


def test_packed_levels_needs_packed():
    """`packed_levels` only widens what `packed=True` regrids raw: alone it is a mistake, refused before any weights
    are read."""
    with pytest.raises(ValueError, match="packed_levels"):
        Regridder(weights="no_such_file.nc", packed_levels=True)
    with pytest.raises(ValueError, match="packed_levels"):
        Regridder(weights="no_such_file.nc", packed=False, packed_levels=True)
