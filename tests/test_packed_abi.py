"""CF-packed 16-bit fields on the host side: the header's dtype codes and `_cf` entries, their ctypes twins, the
`CFDecode` rule against `io._cf_decode`, the keywords, and a packed file opened undecoded (no device needed)."""
import ctypes
import inspect
import os
import re

import numpy as np
import pytest

from smmregrid_amd import CFDecode, DataArray, Dataset, Regridder, SparseOperator, _lib, io

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("smm_apply_cf", "smm_apply_sb_cf", "smm_apply_host_cf")


def _header():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        return f.read()


def test_header_declares_packed_dtypes_and_cf_entries():
    text = _header()
    codes = {m.group(1): int(m.group(2)) for m in re.finditer(r"\b(SMM_[FIU]\d+)\s*=\s*(\d+)", text)}
    assert codes == {"SMM_F32": 0, "SMM_F64": 1, "SMM_I16": 2, "SMM_U16": 3}
    assert (_lib.SMM_I16, _lib.SMM_U16) == (2, 3)
    assert "smm_cf_decode_t" in text
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in ENTRIES:
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", code, flags=re.S)
        assert m, f"{name} is not declared"
        assert "const smm_cf_decode_t*" in m.group(1)


def test_host_stat_byte_counts_are_appended():
    code = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    names = re.findall(r"\b(SMM_HOST_STAT_[A-Z0-9_]+)\b", code)
    names = [n for i, n in enumerate(names) if n not in names[:i]]
    assert names[:10] == ["SMM_HOST_STAT_CALLS", "SMM_HOST_STAT_CHUNKS", "SMM_HOST_STAT_STAGE_IN_MS", "SMM_HOST_STAT_H2D_MS",
                          "SMM_HOST_STAT_KERNEL_MS", "SMM_HOST_STAT_D2H_MS", "SMM_HOST_STAT_COPY_OUT_MS",
                          "SMM_HOST_STAT_WAIT_MS", "SMM_HOST_STAT_TOTAL_MS", "SMM_HOST_STAT_THREADS"]
    assert names[10:] == ["SMM_HOST_STAT_H2D_BYTES", "SMM_HOST_STAT_D2H_BYTES", "SMM_HOST_STAT_COUNT"]
    assert _lib.HOST_STATS[10:] == ("h2d_bytes", "d2h_bytes") and len(_lib.HOST_STATS) == 12


def test_library_exports_and_ctypes_table_lists_the_cf_entries():
    if not os.path.exists(_lib.LIB_PATH):
        _lib.build()
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name), f"{name} is not exported"
        assert name in _lib.SIGNATURES
        assert _lib.SIGNATURES[name][-1] is ctypes.POINTER(_lib.CfDecodeStruct)
        assert _lib.SIGNATURES[name][:-1] == _lib.SIGNATURES[name[:-3]]
    st = _lib.CfDecodeStruct()
    assert ctypes.sizeof(st) == 32 and _lib.CfDecodeStruct.fill.offset == 16 and _lib.CfDecodeStruct.n_fill.offset == 24
    assert _lib.load().smm_abi_version() == 6


def test_refusals_that_need_no_device():
    """The decode rule is validated before anything touches a device."""
    lib = _lib.load()
    st = _lib.CfDecodeStruct(1.0, 0.0, (ctypes.c_int32 * 2)(40000, 0), 1, _lib.SMM_F32)
    x = np.zeros(4, np.int16)
    y = np.zeros(4, np.float64)
    args = (None, x.ctypes.data_as(ctypes.c_void_p), _lib.SMM_I16, 4, y.ctypes.data_as(ctypes.c_void_p), _lib.SMM_F64,
            4, 1, 0.0, 0, None)
    assert lib.smm_apply_cf(*args, ctypes.byref(st)) == _lib.SMM_ERR_INVALID          # 40000 is no int16
    assert b"representable" in lib.smm_last_error()
    assert lib.smm_apply_cf(*args, None) == _lib.SMM_ERR_INVALID                       # integer field, no rule
    st.fill[0] = -32768
    flagged = args[:9] + (_lib.APPLY_NO_FILL,) + args[10:]
    assert lib.smm_apply_cf(*flagged, ctypes.byref(st)) == _lib.SMM_ERR_INVALID       # NO_FILL with a fill value
    st.decode_dtype = _lib.SMM_I16
    assert lib.smm_apply_cf(*args, ctypes.byref(st)) == _lib.SMM_ERR_INVALID


def _raw(rng, dtype, n=4000):
    info = np.iinfo(dtype)
    q = rng.integers(info.min, info.max + 1, size=n).astype(dtype)
    q[:4] = [info.min, info.max, 0, 1]
    return q


@pytest.mark.parametrize("dtype", [np.int16, np.uint16])
@pytest.mark.parametrize("attrs", [
    {"scale_factor": 1.0e-3, "add_offset": 2.7e2},
    {"scale_factor": -0.25},
    {"add_offset": np.float32(273.15)},
    {"scale_factor": np.float64(0.0019), "add_offset": 254.3, "_FillValue": "edge"},
    {"scale_factor": 1.0e-3, "add_offset": 2.7e2, "_FillValue": "edge", "missing_value": 7},
    {"_FillValue": "edge", "missing_value": 12},
    {"scale_factor": 0.5, "missing_value": np.array([3], dtype=np.int64)},
], ids=["scale_offset", "neg_scale", "offset", "one_fill", "two_fills", "fills_only", "array_fill"])
def test_cfdecode_is_the_reader_s_decode(rng, dtype, attrs):
    """`CFDecode.from_attrs(attrs).decode(q)` and `io._cf_decode(q, attrs)`: the same bits (float32 when the variable
    is scaled, float64 with fill values alone); with dtype=float64 the float64 numpy statement of the rule."""
    edge = np.iinfo(dtype).min if dtype == np.int16 else np.iinfo(dtype).max       # -32768 / 65535
    attrs = {k: (dtype(edge) if isinstance(v, str) else v) for k, v in attrs.items()}
    q = _raw(rng, dtype)
    q[10:20] = edge
    q[30:33] = 7
    want = io._cf_decode(q, attrs)
    cf = CFDecode.from_attrs(attrs, raw_dtype=dtype)
    got = cf.decode(q)
    scaled = "scale_factor" in attrs or "add_offset" in attrs
    assert got.dtype == want.dtype == (np.float32 if scaled else np.float64) and cf.dtype == got.dtype
    assert np.array_equal(got.view(np.uint32 if scaled else np.uint64), want.view(np.uint32 if scaled else np.uint64))
    if "_FillValue" in attrs:
        assert np.isnan(got[10:20]).all() and edge in cf.fill_values
    # float64: the rule stated in numpy
    got64 = CFDecode.from_attrs(attrs, dtype=np.float64, raw_dtype=dtype).decode(q)
    ref = q.astype(np.float64)
    if "scale_factor" in attrs:
        ref = ref * np.float64(attrs["scale_factor"])
    if "add_offset" in attrs:
        ref = ref + np.float64(attrs["add_offset"])
    for k in ("_FillValue", "missing_value"):
        if k in attrs:
            ref[q == np.asarray(attrs[k]).ravel()[0]] = np.nan
    assert got64.dtype == np.float64 and np.array_equal(got64.view(np.uint64), ref.view(np.uint64))


def test_cfdecode_constructor_and_struct():
    cf = CFDecode()
    assert (cf.scale_factor, cf.add_offset, cf.fill_values, cf.dtype) == (1.0, 0.0, (), np.dtype(np.float32))
    cf = CFDecode(0.01, 250.0, (-32768, 65535), np.float64)
    st = cf._struct(np.int16)                       # 65535 is no int16: it can never match and is not passed on
    assert (st.scale, st.offset, st.n_fill, st.fill[0], st.decode_dtype) == (0.01, 250.0, 1, -32768, _lib.SMM_F64)
    st = cf._struct(np.uint16)
    assert (st.n_fill, st.fill[0]) == (1, 65535)
    with pytest.raises(ValueError):
        CFDecode(fill_values=(1, 2, 3))
    with pytest.raises(TypeError):
        CFDecode(dtype=np.float16)
    with pytest.raises(TypeError):
        cf.decode(np.zeros(3, np.int32))
    # a fill value no 16-bit integer equals (netCDF's default float fill) is dropped, as it never matches on the host
    assert CFDecode.from_attrs({"_FillValue": 9.969209968386869e36, "scale_factor": 2.0}).fill_values == ()


def test_keywords_exist():
    for name in ("apply", "apply_sb", "apply_host"):
        p = inspect.signature(getattr(SparseOperator, name)).parameters
        assert "cf" in p and p["cf"].default is None, name
    p = inspect.signature(Regridder.__init__).parameters
    assert "packed" in p and p["packed"].default is False
    p = inspect.signature(io.open_dataset).parameters
    assert "decode" in p and p["decode"].default is True
    for fn in (io._open_netcdf4_lite, io._open_netcdf4_h5py):
        assert "decode" in inspect.signature(fn).parameters


def test_packed_file_opened_undecoded_keeps_integers_and_attributes(tmp_path, rng):
    q = _raw(rng, np.int16, 3 * 6 * 8).reshape(3, 6, 8)
    q[1, 2:4, 3:6] = -32768
    attrs = {"scale_factor": np.float64(1.0e-3), "add_offset": np.float64(2.7e2), "_FillValue": np.int16(-32768),
             "units": "K"}
    da = DataArray(q, dims=("time", "lat", "lon"), name="t2m", attrs=attrs,
                   coords={"time": np.arange(3.0), "lat": np.linspace(-75, 75, 6), "lon": np.arange(8) * 45.0})
    path = io.write_netcdf3(Dataset({"t2m": da}, coords=dict(da.coords)), str(tmp_path / "packed.nc"))
    raw = io.open_dataset(path, decode=False)["t2m"]
    assert raw.dtype == np.int16 and np.array_equal(raw.values, q)
    assert raw.attrs["scale_factor"] == 1.0e-3 and raw.attrs["add_offset"] == 2.7e2 and raw.attrs["_FillValue"] == -32768
    dec = io.open_dataset(path)["t2m"]              # the default is unchanged: decoded, packing attributes gone
    assert dec.dtype == np.float32 and not {"scale_factor", "add_offset", "_FillValue"} & set(dec.attrs)
    assert dec.attrs["units"] == "K"
    cf = CFDecode.from_attrs(raw.attrs, raw_dtype=raw.dtype)
    assert np.array_equal(cf.decode(raw.values).view(np.uint32), dec.values.view(np.uint32))
    assert np.isnan(dec.values[1, 2:4, 3:6]).all()
