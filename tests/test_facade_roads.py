"""Which road the Regridder facade sends each variable down, checked without a GPU: the public API -- `Regridder(...)`,
`.regrid`, `.regrid_array`, direct `.apply_weights` / `.regrid3d` -- runs over stand-in operators that record every call
and return zeros of the right shape and dtype, and everything observable (the constructor's refusal, the ordered operator
calls with their keywords, the log records (level, text, how often), the result's dims / shape / container / dtype / attrs, or the exception) is
compared with tests/golden/facade_roads_parent.json, recorded by this same file from the facade as it was before the
routing moved into `smmregrid_amd.road`:

    python tests/test_facade_roads.py record [path]

Nothing private is touched, so the file runs unchanged on either side of that change.
"""
import contextlib
import itertools
import json
import logging
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
GOLDEN = os.path.join(ROOT, "tests", "golden", "facade_roads_parent.json")

SWITCHES = ("packed", "packed_levels", "packed_skipna", "packed_out", "packed_out_levels", "half", "grib_out",
            "grib_out_levels", "grib_out_ccsds", "grib_out_cpx", "gradients")
NT, NLEV, NLAT, NLON, D_LAT, D_LON = 3, 2, 12, 24, 6, 12
S, D = NLAT * NLON, D_LAT * D_LON
FULL = {"scale_factor": 0.01, "add_offset": 273.15, "_FillValue": np.int16(-32768), "missing_value": np.int16(-32768)}


# ------------------------------------------------------------------------------------------------ stand-in operators
def _plain(v):
    """a keyword's value as JSON: scalars as they are, dtypes by name, small arrays as lists, rule objects by repr"""
    if v is None or isinstance(v, (bool, int, float, str)):
        return v
    if isinstance(v, (np.bool_, np.integer, np.floating)):
        return v.item()
    if isinstance(v, (np.dtype, type)):
        return str(np.dtype(v))
    if isinstance(v, np.ndarray):
        return {"array": str(v.dtype), "shape": list(v.shape)} if v.dtype.names or v.size > 16 else v.tolist()
    if type(v).__name__ == "CodedRows":
        return {"coded": v.codec.name, "missing": v.missing is not None}
    return repr(v)


def _field(x):
    from smmregrid_amd import DeviceArray
    if isinstance(x, DeviceArray):
        return {"kind": "device", "dtype": str(x.dtype), "shape": list(x.shape), "layout": x.layout}
    return {"kind": "host", "dtype": str(x.dtype), "shape": list(x.shape), "contiguous": bool(x.flags.c_contiguous)}


class Recorder:
    """Stands where a `SparseOperator` or an `OperatorGroup` stands: records, computes nothing."""

    def __init__(self, calls, n_src, n_dst, members=(), index=0):
        self.calls, self.n_src, self.n_dst, self.members, self.index = calls, n_src, n_dst, list(members), index
        self.handle = None

    def set_epilogue(self, dst_imask=None, dst_frac=None):
        return self

    def mask_apply(self, src_imask):
        return np.full(self.n_dst, 0 if self.index % 2 else 1, dtype=np.int32)

    def close(self):
        pass

    def __len__(self):
        return len(self.members)

    def __getitem__(self, i):
        return self.members[i]

    def _note(self, method, x, kw, **more):
        self.calls.append({"method": ("group." if self.members else "op.") + method, "x": x,
                           **{k: _plain(v) for k, v in more.items()}, "kw": {k: _plain(v) for k, v in sorted(kw.items())}})

    @staticmethod
    def _res(kw):
        return kw["cf_out"].raw_dtype if kw.get("cf_out") is not None else np.dtype(kw.get("out_dtype", np.float64))

    def _levels(self, n_outer, n_lev, n_inner, transpose):
        return (n_outer, n_inner, n_lev, self.n_dst) if transpose else (n_lev, n_outer, n_inner, self.n_dst)

    def _grib_result(self, shape):
        from smmregrid_amd import GribEncode
        return GribEncode(16, 0).encode(np.zeros(shape))

    # -- SparseOperator
    def _op_apply(self, x, **kw):
        from smmregrid_amd import DeviceArray
        self._note("apply", _field(x), kw)
        sb = kw.get("keep_batch_fastest", False)
        n_batch = x.shape[1] if x.layout == "sb" else x.shape[0]
        return DeviceArray((self.n_dst, n_batch) if sb else (n_batch, self.n_dst), self._res(kw), ptr=64,
                           layout="sb" if sb else "bs")

    def _op_apply_host(self, x, **kw):
        self._note("apply_host", _field(x), kw)
        return np.zeros((x.shape[0], self.n_dst), dtype=self._res(kw))

    def _op_apply_host_grib(self, buf, rows, **kw):
        self._note("apply_host_grib", {"kind": "grib", "rows": list(np.shape(rows))}, kw)
        if kw.get("grib_out") is not None:
            return self._grib_result((np.size(rows), self.n_dst))
        return np.zeros((np.size(rows), self.n_dst))

    # -- OperatorGroup
    def _group_apply(self, x, level_index, masked_levels=None, **kw):
        from smmregrid_amd import DeviceArray
        self._note("apply", _field(x), kw, level_index=level_index, masked_levels=masked_levels)
        return DeviceArray(self._levels(*x.shape[:3], kw.get("transpose", True)), self._res(kw), ptr=64)

    def apply_sb(self, x, level_index, masked_levels=None, **kw):
        from smmregrid_amd import DeviceArray
        self._note("apply_sb", _field(x), kw, level_index=level_index, masked_levels=masked_levels)
        n_lev, _, n_batch = x.shape
        if kw.get("keep_batch_fastest", False):
            return DeviceArray((n_lev, self.n_dst, n_batch), self._res(kw), ptr=64, layout="sb")
        shape = (n_batch, n_lev, self.n_dst) if kw.get("transpose", True) else (n_lev, n_batch, self.n_dst)
        return DeviceArray(shape, self._res(kw), ptr=64)

    def _group_apply_host(self, x, level_index, masked_levels=None, **kw):
        self._note("apply_host", _field(x), kw, level_index=level_index, masked_levels=masked_levels)
        return np.zeros(self._levels(*x.shape[:3], kw.get("transpose", True)), dtype=self._res(kw))

    def _group_apply_host_grib(self, buf, rows, level_index, masked_levels=None, **kw):
        self._note("apply_host_grib", {"kind": "grib", "rows": list(np.shape(rows))}, kw, level_index=level_index,
                   masked_levels=masked_levels)
        if kw.get("grib_out") is not None:
            return self._grib_result(np.shape(rows) + (self.n_dst,))
        return np.zeros(self._levels(*np.shape(rows), kw.get("transpose", True)))

    def apply(self, *a, **kw):
        return (self._group_apply if self.members else self._op_apply)(*a, **kw)

    def apply_host(self, *a, **kw):
        return (self._group_apply_host if self.members else self._op_apply_host)(*a, **kw)

    def apply_host_grib(self, *a, **kw):
        return (self._group_apply_host_grib if self.members else self._op_apply_host_grib)(*a, **kw)


@contextlib.contextmanager
def stand_ins(calls):
    """The operator factories of the package replaced by recorders, and the three DeviceArray doors to the device shut:
    a pointer-only DeviceArray reads as zeros and uploads nothing."""
    import importlib
    device, regrid, weights = (importlib.import_module("smmregrid_amd." + m) for m in ("device", "regrid", "weights"))

    def matrix(w, device=None, prune_zeros=False, columns=False):
        calls.append({"method": "compute_weights_matrix", "kw": {"prune_zeros": bool(prune_zeros), "columns": bool(columns)}})
        return Recorder(calls, int(w.sizes["src_grid_size"]), int(w.sizes["dst_grid_size"]))

    def matrix3d(w, mask_dim="lev", device=None, prune_zeros=False, workers=None):
        calls.append({"method": "compute_weights_matrix3d", "kw": {"prune_zeros": bool(prune_zeros)}})
        return [Recorder(calls, int(w.sizes["src_grid_size"]), int(w.sizes["dst_grid_size"]), index=i)
                for i in range(int(w.sizes[mask_dim]))]

    def group(ops):
        return Recorder(calls, ops[0].n_src, ops[0].n_dst, members=ops)

    def to_device(host, dtype=None, stream=None, layout="bs"):
        host = np.asarray(host)
        return device.DeviceArray(host.shape, host.dtype if dtype is None else dtype, ptr=64, layout=layout)

    saved = []

    def put(obj, name, value):
        saved.append((obj, name, getattr(obj, name)))
        setattr(obj, name, value)
    try:
        for mod in (regrid, weights):
            put(mod, "compute_weights_matrix", matrix)
            put(mod, "compute_weights_matrix3d", matrix3d)
        put(regrid, "OperatorGroup", group)
        put(regrid, "to_device", to_device)
        put(device.DeviceArray, "to_host", lambda self, out=None, stream=None: np.zeros(self.shape, dtype=self.dtype))
        put(device.DeviceArray, "copy_from_host", lambda self, host, stream=None: self)
        yield
    finally:
        for obj, name, value in reversed(saved):
            setattr(obj, name, value)


# ------------------------------------------------------------------------------------------------ weights and variables
_MADE = {}


def made(name):
    """The weights ("con", "bic", "levels") and the coordinates, built once (the native generator; no device)."""
    if not _MADE:
        from smmregrid_amd import CdoGenerate, gridgen
        from smmregrid_amd.xrlite import DataArray
        logging.getLogger("smmregrid.CdoGenerate").setLevel(logging.ERROR)
        src = gridgen.parse_grid(f"r{NLON}x{NLAT}")
        _MADE["lat"], _MADE["lon"] = np.asarray(src.lat), np.asarray(src.lon)
        with stand_ins([]):
            for method in ("con", "bic"):
                _MADE[method] = CdoGenerate(f"r{NLON}x{NLAT}", f"r{D_LON}x{D_LAT}", loglevel="ERROR").weights(method=method)
            sea = np.ones((NLEV, NLAT, NLON))
            sea[1, 3:7, 5:11] = np.nan
            field = DataArray(sea, dims=("lev", "lat", "lon"), name="thetao",
                              coords={"lev": np.array([1.0, 2.0]), "lat": _MADE["lat"], "lon": _MADE["lon"]})
            _MADE["levels"] = CdoGenerate(field, f"r{D_LON}x{D_LAT}", loglevel="ERROR").weights(method="con", mask_dim="lev")
    return _MADE[name]


def _values(shape, seed=3):
    return 270.0 + 10.0 * np.random.default_rng(seed).random(shape)


def _var(data, dims, name="tas", attrs=None):
    from smmregrid_amd.xrlite import DataArray
    made("con")
    known = {"time": np.arange(NT), "lev": np.array([1.0, 2.0]), "lat": _MADE["lat"], "lon": _MADE["lon"]}
    return DataArray(data, dims=dims, coords={d: known[d] for d in dims if d in known}, attrs=attrs, name=name)


def _grib(shape, how, n_fields=None):
    """A `GribField` of `shape` (leading axes: one field per index, trailing two: the grid), made on the host."""
    from smmregrid_amd import GribEncode, GribField
    n = int(np.prod(shape[:-2])) if n_fields is None else n_fields
    v = _values((n, S))
    if how == "bitmaps":
        v[:, 5:40] = np.nan
    if how == "complex_mv":
        v[:] = 271.0      # constant rows carry no stream: the records and their missing value management still travel
    codec = {"ccsds": {"ccsds": True}, "complex": {"cpx": True}, "complex_mv": {"cpx": True}}.get(how, {})
    g = GribEncode(16, 1, **codec).encode(v)
    more = {"cpx_missing": np.ones(n, dtype=np.uint8)} if how == "complex_mv" else {}
    return GribField(g.buf, g.rows, shape, S, bitmaps=g.bitmaps if how == "bitmaps" else None, ccsds=g.ccsds, cpx=g.cpx, **more)


def variables_2d():
    from smmregrid_amd import DeviceArray, bfloat16
    from smmregrid_amd.lazy import LazyArray
    from smmregrid_amd.xrlite import DataArray
    shape, dims = (NT, NLAT, NLON), ("time", "lat", "lon")
    raw = np.random.default_rng(5).integers(-2000, 2000, size=shape).astype(np.int16)
    out = {k: _var(_values(shape).astype(k), dims) for k in ("float64", "float32", "float16", "int32")}
    out["bfloat16"] = _var(np.zeros(shape, dtype=np.uint16).view(bfloat16), dims)
    out["int16_full"] = _var(raw, dims, attrs=dict(FULL, units="K"))
    out["int16_nofill"] = _var(raw, dims, attrs={"scale_factor": 0.01, "add_offset": 273.15, "units": "K"})
    out["uint16_three_fills"] = _var(raw.astype(np.uint16), dims, attrs={
        "scale_factor": 0.5, "_FillValue": np.uint16(65535), "missing_value": np.array([65534, 65533], dtype=np.uint16)})
    out["int16_plain"] = _var(raw, dims, attrs={"units": "1"})
    out["lazy"] = _var(LazyArray(shape, np.float64, lambda: _values(shape)), dims)
    out["dev_float64_bs"] = _var(DeviceArray(shape, np.float64, ptr=64), dims)
    out["dev_float32_sb"] = _var(DeviceArray((NLAT, NLON, NT), np.float32, ptr=64, layout="sb"), ("lat", "lon", "time"))
    out["dev_float16"] = _var(DeviceArray(shape, np.float16, ptr=64), dims)
    out["dev_int16_full"] = _var(DeviceArray(shape, np.int16, ptr=64), dims, attrs=dict(FULL))
    for how in ("simple", "bitmaps", "ccsds", "complex", "complex_mv"):
        out["grib_" + how] = _var(_grib(shape, how), dims, name="t2m")
    out["x_bnds"] = DataArray(np.zeros((NLON, 2)), dims=("lon", "bnds"), name="x_bnds")
    out["time_bnds"] = DataArray(np.zeros((NT, 2)), dims=("time", "bnds"), name="time_bnds")
    return out


def variables_levels():
    from smmregrid_amd import DeviceArray
    tl, lt = ("time", "lev", "lat", "lon"), ("lev", "time", "lat", "lon")
    raw = np.random.default_rng(6).integers(-2000, 2000, size=(NT, NLEV, NLAT, NLON)).astype(np.int16)
    return {
        "float64_time_lev": _var(_values((NT, NLEV, NLAT, NLON)), tl, "thetao"),
        "float64_lev_time": _var(_values((NLEV, NT, NLAT, NLON)), lt, "thetao"),
        "float16_time_lev": _var(_values((NT, NLEV, NLAT, NLON)).astype(np.float16), tl, "thetao"),
        "int16_full": _var(raw, tl, "thetao", attrs=dict(FULL)),
        "dev_bs": _var(DeviceArray((NT, NLEV, NLAT, NLON), np.float64, ptr=64), tl, "thetao"),
        "dev_int16_full": _var(DeviceArray((NT, NLEV, NLAT, NLON), np.int16, ptr=64), tl, "thetao", attrs=dict(FULL)),
        "dev_sb": _var(DeviceArray((NLEV, NLAT, NLON, NT), np.float64, ptr=64, layout="sb"), ("lev", "lat", "lon", "time"),
                       "thetao"),
        "grib_time_lev": _var(_grib((NT, NLEV, NLAT, NLON), "simple"), tl, "thetao"),
        "grib_unordered": _var(_grib((NT, NLAT, NLEV, NLON), "simple", NT * NLEV), ("time", "lat", "lev", "lon"), "thetao"),
    }


# ------------------------------------------------------------------------------------------------ option sets
P = {"packed": True}
GO = dict(P, grib_out=True)
OPTIONS_2D = {
    "default": {}, "packed": P, "packed_levels": dict(P, packed_levels=True),
    "packed_skipna": dict(P, skipna=True, packed_skipna=True), "packed_skipna_off": dict(P, skipna=True),
    "packed_out": dict(P, packed_out=True), "packed_out_levels": dict(P, packed_out=True, packed_out_levels=True),
    "half": {"half": True}, "grib_out": GO, "grib_out_levels": dict(GO, packed_levels=True, grib_out_levels=True),
    "grib_out_ccsds": dict(GO, grib_out_ccsds=True), "grib_out_cpx": dict(GO, grib_out_cpx=True),
    "grib_out_skipna": dict(GO, skipna=True, packed_skipna=True),
    "gradients": {"gradients": True}, "skipna": {"skipna": True}, "keep_batch_fastest": {"keep_batch_fastest": True},
    "out_float32": {"out_dtype": "float32"}, "out_float16": {"out_dtype": "float16"}, "out_bfloat16": {"out_dtype": "bfloat16"},
    "packed_out_float32": dict(P, out_dtype="float32"), "packed_out_float16": dict(P, out_dtype="float16"),
    "half_out_float32": {"half": True, "out_dtype": "float32"},
    "lazy": {"lazy": True}, "lazy_packed": dict(P, lazy=True), "lazy_packed_levels": dict(P, lazy=True, packed_levels=True),
    "lazy_packed_skipna": dict(P, lazy=True, skipna=True, packed_skipna=True),
    "lazy_packed_out": dict(P, lazy=True, packed_out=True),
    "lazy_packed_out_levels": dict(P, lazy=True, packed_out=True, packed_out_levels=True),
    "lazy_half": {"lazy": True, "half": True}, "lazy_gradients": {"lazy": True, "gradients": True},
    "lazy_skipna": {"lazy": True, "skipna": True}, "lazy_keep_batch_fastest": {"lazy": True, "keep_batch_fastest": True},
}
PL = dict(P, packed_levels=True)
OPTIONS_LEVELS = {
    "default": {}, "packed": P, "packed_levels": PL,
    "packed_out": dict(P, packed_out=True), "packed_out_levels": dict(P, packed_out=True, packed_out_levels=True),
    "packed_levels_out": dict(PL, packed_out=True), "packed_levels_out_levels": dict(PL, packed_out=True, packed_out_levels=True),
    "grib_out": dict(PL, grib_out=True), "grib_out_levels": dict(PL, grib_out=True, grib_out_levels=True),
    "grib_out_no_levels": GO,
    "skipna": dict(PL, skipna=True), "packed_skipna": dict(PL, skipna=True, packed_skipna=True),
    "skipna_unpacked": {"skipna": True},
    "no_transpose": {"transpose": False}, "no_transpose_packed_levels": dict(PL, transpose=False),
    "no_transpose_grib_out_levels": dict(PL, transpose=False, grib_out=True, grib_out_levels=True),
    "lazy": {"lazy": True}, "lazy_packed_levels": dict(PL, lazy=True),
    "lazy_packed_out": dict(PL, lazy=True, packed_out=True),
    "half": {"half": True}, "keep_batch_fastest": {"keep_batch_fastest": True}, "out_float32": dict(PL, out_dtype="float32"),
    "gradients": {"gradients": True},
}


def _kwargs(options):
    from smmregrid_amd import bfloat16
    kw = dict(options)
    if "out_dtype" in kw:
        kw["out_dtype"] = bfloat16 if kw["out_dtype"] == "bfloat16" else np.dtype(kw["out_dtype"])
    return kw


# ------------------------------------------------------------------------------------------------ what a case shows
class _Lines(logging.Handler):
    def __init__(self):
        super().__init__(level=logging.DEBUG)
        self.lines = []

    def emit(self, record):
        self.lines.append([record.levelname, record.getMessage()])


def _result(out):
    from smmregrid_amd import DeviceArray, GribField
    from smmregrid_amd.lazy import LazyArray
    data = out.data
    seen = {"dims": list(out.dims), "shape": list(out.shape), "container": type(data).__name__,
            "dtype": None if data is None else str(data.dtype), "name": out.name,
            "attrs": {k: repr(v) for k, v in sorted(out.attrs.items())}, "coords": list(out.coords)}
    if isinstance(data, DeviceArray):
        seen["layout"] = data.layout
    if isinstance(data, GribField):
        seen["grib"] = [k for k in ("bitmaps", "ccsds", "cpx", "cpx_missing") if getattr(data, k) is not None]
    if isinstance(data, LazyArray):
        seen["computed"] = list(np.shape(data.compute()))
    return seen


def observe(run, weights, options):
    """One case: a fresh Regridder over stand-ins (`run(regridder)` is the call under test), everything it shows."""
    from smmregrid_amd import Regridder
    from smmregrid_amd.lazy import LazyArray
    calls, lines = [], _Lines()
    log = logging.getLogger("smmregrid.Regrid")
    log.addHandler(lines)
    seen = {}
    try:
        with stand_ins(calls):
            try:
                rg = Regridder(weights=made(weights), loglevel="DEBUG", **_kwargs(options))
            except Exception as err:      # noqa: BLE001 -- the refusal is what is recorded
                return {"constructor": [type(err).__name__, str(err)]}
            del calls[:]
            try:
                out = run(rg)
                if isinstance(out.data, LazyArray):
                    seen["calls_before_compute"] = len(calls)
                seen["result"] = _result(out)
            except Exception as err:      # noqa: BLE001
                seen["raised"] = [type(err).__name__, str(err)]
    finally:
        log.removeHandler(lines)
    seen["calls"], seen["log"] = calls, sorted(lines.lines)      # every line with its level, as often as it came
    return seen


def constructor_outcomes():
    """{"accepted" or the message: the switch combinations that end so}, a combination written as the bits of SWITCHES
    (bit i: SWITCHES[i]) plus 2048 with skipna on."""
    from smmregrid_amd import Regridder
    out = {}
    with stand_ins([]):
        for skipna, bits in itertools.product((False, True), range(1 << len(SWITCHES))):
            kw = {name: bool(bits >> i & 1) for i, name in enumerate(SWITCHES)}
            try:
                Regridder(weights=made("bic"), skipna=skipna, **kw)
                key = "accepted"
            except ValueError as err:
                key = str(err)
            out.setdefault(key, []).append(bits + (1 << len(SWITCHES)) * skipna)
    return out


def roads(options_table, variables, weights_of):
    return {f"{oname}/{vname}": observe(lambda rg, v=var: rg.regrid_array(v), weights_of(options), options)
            for oname, options in options_table.items() for vname, var in variables.items()}


def roads_2d():
    return roads(OPTIONS_2D, variables_2d(), lambda o: "bic" if o.get("gradients") else "con")


def roads_levels():
    return roads(OPTIONS_LEVELS, variables_levels(), lambda o: "levels")


def datasets():
    from smmregrid_amd.xrlite import Dataset
    v = variables_2d()
    ds = Dataset({"tas": v["float64"], "tp": v["int16_full"], "t2m": v["grib_simple"], "x_bnds": v["x_bnds"],
                  "time_bnds": v["time_bnds"]})

    def run(rg):
        out = rg.regrid(ds)
        first = out["tas"]
        first.attrs = dict(first.attrs, variables=list(out.data_vars),
                           dtypes=[str(a.data.dtype) for a in out.data_vars.values()])
        return first
    return {name: observe(run, "con", OPTIONS_2D[name]) for name in ("default", "packed", "grib_out", "lazy_packed_out")}


def direct_calls():
    from smmregrid_amd.gradients import GradientRule
    from smmregrid_amd.gridtype import GridType
    v2, v3 = variables_2d(), variables_levels()
    hd = ["lat", "lon"]
    rule = GradientRule.from_weights(made("bic"))

    def aw(var, weights, **kw):
        return lambda rg: rg.apply_weights(var, made(weights), horizontal_dims=hd, **kw)

    def r3(var):
        return lambda rg: rg.regrid3d(var, GridType(dims=var.dims, extra_dims={"mask": ["lev"]}))
    cases = {
        "apply_weights/grib/default": (aw(v2["grib_simple"], "con"), "con", {}),
        "apply_weights/grib/packed": (aw(v2["grib_simple"], "con"), "con", P),
        "apply_weights/grib/packed_skipna_off": (aw(v2["grib_simple"], "con"), "con", dict(P, skipna=True)),
        "apply_weights/grib_ccsds/grib_out": (aw(v2["grib_ccsds"], "con"), "con", GO),
        "apply_weights/grib/out_float32": (aw(v2["grib_simple"], "con", out_dtype=np.float32), "con", P),
        "apply_weights/float16/half": (aw(v2["float16"], "con"), "con", {"half": True}),
        "apply_weights/sb/gradients_keyword": (aw(v2["dev_float32_sb"], "bic", gradients=rule), "bic", {}),
        "apply_weights/sb/gradients_switch": (aw(v2["dev_float32_sb"], "bic"), "bic", {"gradients": True}),
        "apply_weights/float64/gradients_keyword": (aw(v2["float64"], "bic", gradients=rule), "bic", {}),
        "apply_weights/float64/keep_batch_fastest": (aw(v2["float64"], "con"), "con", {"keep_batch_fastest": True}),
        "regrid3d/grib/default": (r3(v3["grib_time_lev"]), "levels", {}),
        "regrid3d/grib/packed": (r3(v3["grib_time_lev"]), "levels", P),
        "regrid3d/grib/packed_levels": (r3(v3["grib_time_lev"]), "levels", PL),
        "regrid3d/grib_unordered/packed_levels": (r3(v3["grib_unordered"]), "levels", PL),
        "regrid3d/grib/grib_out_keyword": (
            lambda rg: rg.regrid3d(v3["grib_time_lev"], GridType(dims=v3["grib_time_lev"].dims, extra_dims={"mask": ["lev"]}),
                                   grib_out=True), "levels", dict(PL, grib_out=True, grib_out_levels=True)),
        "regrid3d/sb/keep_batch_fastest": (r3(v3["dev_sb"]), "levels", {"keep_batch_fastest": True}),
        "regrid3d/float64/keep_batch_fastest": (r3(v3["float64_time_lev"]), "levels", {"keep_batch_fastest": True}),
    }
    return {name: observe(run, weights, options) for name, (run, weights, options) in cases.items()}


PARTS = {"constructor": constructor_outcomes, "roads_2d": roads_2d, "roads_levels": roads_levels, "datasets": datasets,
         "direct": direct_calls}


def _json(obj):
    return json.loads(json.dumps(obj))


def record(path=GOLDEN):
    """Write the golden: the outcomes, each distinct one stored once."""
    table, index, parts = [], {}, {}
    for part, make in PARTS.items():
        seen = _json(make())
        if part == "constructor":
            parts[part] = seen
            continue
        parts[part] = {}
        for case, outcome in seen.items():
            key = json.dumps(outcome, sort_keys=True)
            if key not in index:
                index[key] = len(table)
                table.append(outcome)
            parts[part][case] = index[key]
    with open(path, "w") as f:
        json.dump({"outcomes": table, "cases": parts}, f, sort_keys=True, separators=(",", ":"))
        f.write("\n")
    return {k: len(v) for k, v in parts.items()}


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)


def test_constructor_accepts_and_refuses_every_switch_combination_as_before(golden):
    now, then = _json(constructor_outcomes()), golden["cases"]["constructor"]
    assert sum(len(v) for v in then.values()) == 2 << len(SWITCHES)
    assert sorted(now) == sorted(then)
    for message in then:
        assert now[message] == then[message], message


@pytest.mark.parametrize("part", [p for p in PARTS if p != "constructor"])
def test_every_case_takes_the_road_it_took(golden, part):
    now, then = _json(PARTS[part]()), golden["cases"][part]
    assert sorted(now) == sorted(then)      # no case dropped, none added
    different = [case for case in then if now[case] != golden["outcomes"][then[case]]]
    for case in different[:3]:
        print(case, "\n  was", json.dumps(golden["outcomes"][then[case]], sort_keys=True), "\n  is ",
              json.dumps(now[case], sort_keys=True))
    assert not different, f"{len(different)} of {len(then)} cases differ: {different[:10]}"


if __name__ == "__main__":
    if len(sys.argv) >= 2 and sys.argv[1] == "record":
        print(record(*sys.argv[2:3]))
    else:
        sys.exit("usage: test_facade_roads.py record [path]")
