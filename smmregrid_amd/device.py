"""HBM buffers, streams and events over the C ABI (no torch, no cupy)."""
import ctypes

import numpy as np

from . import _lib

# numpy has no bfloat16: a 2-byte dtype of the project's own (one `<u2` field holding the bits) names it, so that
# `np.empty(shape, bfloat16)`, `bits.view(bfloat16)` and `DeviceArray(shape, bfloat16)` work; `to_bfloat16` /
# `from_bfloat16` convert
bfloat16 = np.dtype([("bfloat16", "<u2")])

_DTYPE_CODE = {np.dtype(np.float32): _lib.SMM_F32, np.dtype(np.float64): _lib.SMM_F64,
               np.dtype(np.float16): _lib.SMM_F16, bfloat16: _lib.SMM_BF16}
_HALF = (np.dtype(np.float16), bfloat16)
# (field dtype, result dtype) pairs the kernels are built for when either is a half type (SMM_BUILT)
HALF_PAIRS = tuple((h, y) for h in _HALF for y in (np.dtype(np.float64), h)) + \
    tuple((x, h) for h in _HALF for x in (np.dtype(np.float32), np.dtype(np.float64)))


def dtype_code(dtype):
    try:
        return _DTYPE_CODE[np.dtype(dtype)]
    except KeyError:
        raise TypeError(f"field dtype {dtype} not supported on device (float32/float64, float16/bfloat16 only)")


def is_half_dtype(dtype):
    """float16 / `bfloat16`: regridded as 2-byte elements (widened to float32 in the kernels' registers)."""
    return dtype is not None and np.dtype(dtype) in _HALF


def _dtype_name(dtype):
    return "bfloat16" if np.dtype(dtype) == bfloat16 else np.dtype(dtype).name


def check_half_pair(x_dtype, y_dtype):
    """TypeError for a (field, result) dtype pair with a half type that the kernels are not built for."""
    x_dtype, y_dtype = np.dtype(x_dtype), np.dtype(y_dtype)
    if (x_dtype in _HALF or y_dtype in _HALF) and (x_dtype, y_dtype) not in HALF_PAIRS:
        built = ", ".join(f"{_dtype_name(a)} -> {_dtype_name(b)}" for a, b in HALF_PAIRS)
        raise TypeError(f"{_dtype_name(x_dtype)} -> {_dtype_name(y_dtype)} is not built; the half-precision pairs "
                        f"(field -> result) are: {built}")


def _round_bits(u, drop):
    """u >> drop rounded to nearest, ties to even (integer arrays)."""
    q = u >> drop
    rem = u & ((1 << drop) - 1)
    half = 1 << (drop - 1)
    return q + ((rem > half) | ((rem == half) & ((q & 1) == 1))).astype(u.dtype)


def to_bfloat16(a):
    """float32 / float64 (float16 is widened exactly) -> `bfloat16`, round to nearest even, correctly rounded from the
    input's OWN precision (a float64 never passes through float32).  Overflow gives +-inf, NaN the quiet NaN 0x7FC0
    with the sign kept."""
    a = np.asarray(a)
    if a.dtype == np.float16:
        a = a.astype(np.float32)
    if a.dtype == np.float32:
        u = np.ascontiguousarray(a).view(np.uint32).astype(np.uint64)
        mag, sign = u & 0x7FFFFFFF, (u >> 16) & 0x8000
        bits = _round_bits(mag, 16)          # the carry moves into the exponent: next binade or inf
        bits = np.where(mag > 0x7F800000, 0x7FC0, bits)
    elif a.dtype == np.float64:
        u = np.ascontiguousarray(a).view(np.uint64)
        mag, sign = u & 0x7FFFFFFFFFFFFFFF, (u >> 48) & 0x8000
        he = (mag >> 52).astype(np.int64) - 1023 + 127        # biased bfloat16 exponent before rounding
        m = (mag & 0x000FFFFFFFFFFFFF) | 0x0010000000000000
        drop = np.minimum(45 + np.where(he <= 0, 1 - he, 0), 63).astype(np.uint64)
        q = m >> drop
        rem, half = m & ((np.uint64(1) << drop) - np.uint64(1)), np.uint64(1) << (drop - np.uint64(1))
        up = (rem > half) | ((rem == half) & ((q & np.uint64(1)) == 1))
        bits = (np.maximum(he - 1, 0).astype(np.uint64) << np.uint64(7)) + q + up.astype(np.uint64)
        bits = np.where(he >= 255, 0x7F80, bits)
        bits = np.where(mag > 0x7FF0000000000000, 0x7FC0, bits)
    else:
        raise TypeError(f"to_bfloat16 takes float32 or float64, got {a.dtype}")
    return (bits | sign).astype(np.uint16).view(bfloat16).reshape(a.shape)


def from_bfloat16(a):
    """`bfloat16` (or its raw uint16 bits) -> float32, exact."""
    a = np.asarray(a)
    if a.dtype != bfloat16 and a.dtype != np.uint16:
        raise TypeError(f"from_bfloat16 takes bfloat16 (or uint16 bits), got {a.dtype}")
    bits = np.ascontiguousarray(a).view(np.uint16)
    return (bits.astype(np.uint32) << 16).view(np.float32).reshape(a.shape)


_PACKED_CODE = {np.dtype(np.int16): _lib.SMM_I16, np.dtype(np.uint16): _lib.SMM_U16}


def is_packed_dtype(dtype):
    """int16 / uint16: what a CF-packed field holds (regridded raw with a `CFDecode`)."""
    return np.dtype(dtype) in _PACKED_CODE


def field_dtype_code(dtype, cf=None):
    """dtype_code for a field that may be CF-packed: int16 / uint16 are taken with a decode rule only."""
    if cf is not None and is_packed_dtype(dtype):
        return _PACKED_CODE[np.dtype(dtype)]
    if cf is not None:
        raise TypeError(f"a CFDecode rule goes with a raw int16 / uint16 field, not {np.dtype(dtype)}")
    return dtype_code(dtype)


class CFDecode:
    """How a CF-packed 16-bit field becomes values (`scale_factor`, `add_offset`, `_FillValue` / `missing_value`):

        v = dtype(q);  v = v * dtype(scale_factor);  v = v + dtype(add_offset);  q in fill_values -> NaN

    two rounded operations in `dtype` (float32, what `io.open_dataset` decodes 2-byte integers to, or float64), the
    fill values compared on the raw integers.  Passed as `cf=` to `SparseOperator.apply` / `apply_sb` / `apply_host`
    the raw int16 / uint16 field is decoded inside the kernels; the result is bit-identical to regridding
    `cf.decode(q)`.  `scale_factor` / `add_offset` None = absent (the step is skipped)."""

    def __init__(self, scale_factor=1.0, add_offset=0.0, fill_values=(), dtype=np.float32):
        self.dtype = np.dtype(dtype)
        if self.dtype not in (np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError("CFDecode dtype must be float32 or float64")
        self.scale_factor = None if scale_factor is None else float(scale_factor)
        self.add_offset = None if add_offset is None else float(add_offset)
        fills = []
        for f in np.atleast_1d(np.asarray(fill_values)).ravel().tolist() if np.size(fill_values) else []:
            if float(f) != int(f):
                raise ValueError(f"fill value {f!r} is not an integer")
            if int(f) not in fills:
                fills.append(int(f))
        if len(fills) > 2:
            raise ValueError("at most two distinct fill values (_FillValue and missing_value)")
        self.fill_values = tuple(fills)

    @classmethod
    def from_attrs(cls, attrs, dtype=None, raw_dtype=None):
        """The rule of a variable's CF attributes.  dtype None = what `io.open_dataset` picks for a 2-byte integer
        variable: float32 with a scale_factor / add_offset, float64 with fill values alone.  Fill values no element
        of raw_dtype (or, without it, no 16-bit integer) can equal -- a NaN, 9.96921e36 -- are dropped: they never
        match on the host either."""
        scale, offset = attrs.get("scale_factor"), attrs.get("add_offset")
        if dtype is None:
            dtype = np.float32 if (scale is not None or offset is not None) else np.float64
        lo, hi = (-32768, 65535) if raw_dtype is None else (np.iinfo(raw_dtype).min, np.iinfo(raw_dtype).max)
        fills = []
        for k in ("_FillValue", "missing_value"):
            if k in attrs:
                for f in np.atleast_1d(np.asarray(attrs[k])).ravel().tolist():
                    if isinstance(f, (int, float)) and f == f and float(f) == int(f) and lo <= int(f) <= hi:
                        fills.append(int(f))
        return cls(None if scale is None else np.asarray(scale).ravel()[0],
                   None if offset is None else np.asarray(offset).ravel()[0], fills, dtype)

    def decode(self, values):
        """The numpy statement of the rule (what the kernels reproduce bit for bit)."""
        values = np.asarray(values)
        if not is_packed_dtype(values.dtype):
            raise TypeError(f"CFDecode.decode takes int16 / uint16, got {values.dtype}")
        out = values.astype(self.dtype)
        if self.scale_factor is not None:
            out = out * np.asarray(self.scale_factor, dtype=self.dtype)
        if self.add_offset is not None:
            out = out + np.asarray(self.add_offset, dtype=self.dtype)
        for f in self.fill_values:
            if np.iinfo(values.dtype).min <= f <= np.iinfo(values.dtype).max:
                out[values == f] = np.nan
        return out

    def _struct(self, raw_dtype):
        """smm_cf_decode_t for a field of raw_dtype (fills the raw type cannot hold never match: dropped)."""
        info = np.iinfo(raw_dtype)
        fills = [f for f in self.fill_values if info.min <= f <= info.max]
        st = _lib.CfDecodeStruct()
        st.scale = 1.0 if self.scale_factor is None else self.scale_factor
        st.offset = 0.0 if self.add_offset is None else self.add_offset
        for i, f in enumerate(fills):
            st.fill[i] = f
        st.n_fill = len(fills)
        st.decode_dtype = dtype_code(self.dtype)
        return st

    def __repr__(self):
        return (f"CFDecode(scale_factor={self.scale_factor}, add_offset={self.add_offset}, "
                f"fill_values={self.fill_values}, dtype={self.dtype.name})")


class CFEncode:
    """How a float64 regrid result becomes a CF-packed 16-bit variable (`scale_factor`, `add_offset`, `_FillValue`):

        t = (float64(y) - float64(add_offset)) / float64(scale_factor)      two rounded float64 operations
        r = rint(t)                                                         ties to even
        q = fill_value  where  y is not finite  or  r < iinfo.min  or  r > iinfo.max,  else raw_dtype(r)

    Always float64 arithmetic: the regrid result is float64.  NaN results go to `fill_value`, and so does every value
    that rounds outside the raw range: there is NO wrap-around and NO saturation.  A valid value that happens to
    round onto `fill_value` is stored as is (as xarray does): it reads back as missing.  Passed as `cf_out=` to
    `SparseOperator.apply` / `apply_sb` / `apply_host` the rule runs inside the kernels' stores and the result has
    `raw_dtype`; the bits are those of `encode` applied to the float64 result.  `scale_factor` / `add_offset` None =
    absent (1 / 0).  `fill_value` is mandatory: NaN results need somewhere to go."""

    def __init__(self, scale_factor, add_offset, fill_value, raw_dtype):
        self.raw_dtype = np.dtype(raw_dtype)
        if not is_packed_dtype(self.raw_dtype):
            raise TypeError("CFEncode raw_dtype must be int16 or uint16")
        self.scale_factor = None if scale_factor is None else float(np.asarray(scale_factor).ravel()[0])
        self.add_offset = None if add_offset is None else float(np.asarray(add_offset).ravel()[0])
        if self.scale_factor is not None and (not np.isfinite(self.scale_factor) or self.scale_factor == 0.0):
            raise ValueError(f"scale_factor must be finite and non-zero, got {self.scale_factor}")
        if self.add_offset is not None and not np.isfinite(self.add_offset):
            raise ValueError(f"add_offset must be finite, got {self.add_offset}")
        if fill_value is None:
            raise ValueError("CFEncode needs a fill_value: NaN results need somewhere to go")
        f = np.asarray(fill_value).ravel()[0].item()
        info = np.iinfo(self.raw_dtype)
        if f != f or float(f) != int(f) or not info.min <= int(f) <= info.max:
            raise ValueError(f"fill value {f!r} is not representable in {self.raw_dtype.name}")
        self.fill_value = int(f)

    @classmethod
    def from_attrs(cls, attrs, raw_dtype):
        """The rule of a variable's CF attributes: `_FillValue`, else `missing_value` (ValueError without one)."""
        fill = attrs.get("_FillValue", attrs.get("missing_value"))
        if fill is None:
            raise ValueError("no _FillValue / missing_value attribute: NaN results would have nowhere to go")
        return cls(attrs.get("scale_factor"), attrs.get("add_offset"), fill, raw_dtype)

    def attrs(self):
        """The attributes to put on an encoded result (it then reads back through `CFDecode.from_attrs`)."""
        out = {}
        if self.scale_factor is not None:
            out["scale_factor"] = np.float64(self.scale_factor)
        if self.add_offset is not None:
            out["add_offset"] = np.float64(self.add_offset)
        out["_FillValue"] = self.raw_dtype.type(self.fill_value)
        return out

    def encode(self, values):
        """The numpy statement of the rule (what the kernels reproduce bit for bit)."""
        y = np.asarray(values, dtype=np.float64)
        info = np.iinfo(self.raw_dtype)
        with np.errstate(invalid="ignore", over="ignore"):
            t = (y - np.float64(0.0 if self.add_offset is None else self.add_offset)) \
                / np.float64(1.0 if self.scale_factor is None else self.scale_factor)
            r = np.rint(t)
            bad = ~np.isfinite(y) | (r < info.min) | (r > info.max)
            return np.where(bad, self.fill_value, r).astype(self.raw_dtype)

    def _struct(self):
        """smm_cf_encode_t"""
        return _lib.CfEncodeStruct(1.0 if self.scale_factor is None else self.scale_factor,
                                   0.0 if self.add_offset is None else self.add_offset, self.fill_value, 0)

    def __repr__(self):
        return (f"CFEncode(scale_factor={self.scale_factor}, add_offset={self.add_offset}, "
                f"fill_value={self.fill_value}, raw_dtype={self.raw_dtype.name})")


def result_dtype(out_dtype, cf_out):
    """(numpy dtype, ABI code) of an apply result: `out_dtype`, or the raw dtype of a `CFEncode` given as cf_out
    (which excludes out_dtype=float32)."""
    if cf_out is None:
        return np.dtype(out_dtype), dtype_code(out_dtype)
    if not isinstance(cf_out, CFEncode):
        raise TypeError("cf_out must be a CFEncode")
    if np.dtype(out_dtype) != np.dtype(np.float64):
        raise ValueError("cf_out encodes the float64 result: out_dtype must stay float64")
    return cf_out.raw_dtype, _PACKED_CODE[cf_out.raw_dtype]


def device_count():
    return _lib.device_count()


def set_device(device):
    _lib.call("smm_set_device", int(device))


def current_device():
    d = ctypes.c_int(0)
    _lib.call("smm_get_device", ctypes.byref(d))
    return d.value


def device_name(device=0):
    buf = ctypes.create_string_buffer(256)
    _lib.call("smm_device_name", int(device), buf, 256)
    return buf.value.decode().strip()        # boxes without a marketing name report " (gfx950..., 256 CUs)"


def mem_info():
    f, t = ctypes.c_size_t(0), ctypes.c_size_t(0)
    _lib.call("smm_mem_info", ctypes.byref(f), ctypes.byref(t))
    return f.value, t.value


def synchronize():
    _lib.call("smm_device_sync")


class Stream:
    def __init__(self):
        h = ctypes.c_void_p()
        _lib.call("smm_stream_create", ctypes.byref(h))
        self.handle = h

    def synchronize(self):
        _lib.call("smm_stream_sync", self.handle)

    def wait_event(self, event):
        """Work queued on this stream afterwards waits for `event`."""
        _lib.call("smm_stream_wait_event", self.handle, event.handle)

    def close(self):
        if self.handle:
            _lib.call("smm_stream_destroy", self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _stream_handle(stream):
    if stream is None:
        return None
    return stream.handle if isinstance(stream, Stream) else stream


class Event:
    def __init__(self):
        h = ctypes.c_void_p()
        _lib.call("smm_event_create", ctypes.byref(h))
        self.handle = h

    def record(self, stream=None):
        _lib.call("smm_event_record", self.handle, _stream_handle(stream))

    def synchronize(self):
        _lib.call("smm_event_sync", self.handle)

    def elapsed_ms(self, stop):
        ms = ctypes.c_float(0)
        _lib.call("smm_event_elapsed_ms", self.handle, stop.handle, ctypes.byref(ms))
        return ms.value

    def __del__(self):
        try:
            if self.handle:
                _lib.call("smm_event_destroy", self.handle)
                self.handle = None
        except Exception:
            pass


class DeviceArray:
    """A C-contiguous array resident in HBM.  Owns its allocation unless it is a view.

    `layout` tags how a FIELD is laid out: "bs" (default) -- the reference's native order, horizontal
    cells fastest, (batch..., S) (regrid.py:539-541); "sb" -- batch-fastest, (S..., batch...): the batch
    values of one cell are contiguous.  `SparseOperator.apply` / `Regridder` route an "sb" field to the
    batch-fastest kernel (smm_apply_sb), whose HBM traffic equals the algorithmic bytes."""

    def __init__(self, shape, dtype, ptr=None, base=None, layout="bs"):
        self.shape = tuple(int(s) for s in np.atleast_1d(shape)) if not isinstance(shape, tuple) \
            else tuple(int(s) for s in shape)
        self.dtype = np.dtype(dtype)
        self.base = base
        if layout not in ("bs", "sb"):
            raise ValueError("layout must be 'bs' (cells fastest) or 'sb' (batch fastest)")
        self.layout = layout
        if ptr is None:
            h = ctypes.c_void_p()
            _lib.call("smm_malloc", ctypes.byref(h), self.nbytes)
            self.ptr = h.value or 0
            self._owned = True
        else:
            self.ptr = int(ptr)
            self._owned = False

    @property
    def size(self):
        n = 1
        for s in self.shape:
            n *= s
        return n

    @property
    def nbytes(self):
        return self.size * self.dtype.itemsize

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def __cuda_array_interface__(self):
        """Zero-copy hand-over to array libraries that speak the protocol (``torch.as_tensor``,
        cupy, numba): the buffer stays owned by this DeviceArray."""
        return {"shape": self.shape, "typestr": self.dtype.str, "data": (int(self.ptr), False),
                "version": 2, "strides": None}

    @classmethod
    def from_interface(cls, obj, layout="bs"):
        """Zero-copy view of any C-contiguous object that speaks ``__cuda_array_interface__`` (a torch or cupy
        tensor on this device, another DeviceArray) holding float16 / float32 / float64.  The view keeps a reference
        to `obj`, which keeps owning the memory.  A torch bfloat16 tensor does not export the protocol: wrap it
        with ``DeviceArray(t.shape, bfloat16, ptr=t.data_ptr(), base=t)``."""
        iface = getattr(obj, "__cuda_array_interface__", None)
        if not isinstance(iface, dict):
            raise TypeError(f"{type(obj).__name__} does not export __cuda_array_interface__")
        dtype = np.dtype(iface["typestr"])
        if dtype not in (np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)):
            raise TypeError(f"from_interface takes float16 / float32 / float64, got {iface['typestr']}")
        shape = tuple(int(n) for n in iface["shape"])
        strides = iface.get("strides")
        if strides is not None:
            want, step = [], dtype.itemsize
            for n in reversed(shape):
                want.append(step)
                step *= max(n, 1)
            if any(n > 1 and int(st) != w for n, st, w in zip(shape, strides, reversed(want))):
                raise ValueError("from_interface needs a C-contiguous array")
        ptr = iface["data"][0]
        return cls(shape, dtype, ptr=int(ptr or 0), base=obj, layout=layout)

    def reshape(self, *shape):
        if len(shape) == 1 and isinstance(shape[0], (tuple, list)):
            shape = tuple(shape[0])
        shape = list(shape)
        if -1 in shape:
            i = shape.index(-1)
            known = 1
            for k, s in enumerate(shape):
                if k != i:
                    known *= s
            shape[i] = self.size // known if known else 0
        out = DeviceArray(tuple(shape), self.dtype, ptr=self.ptr, base=self.base or self, layout=self.layout)
        if out.size != self.size:
            raise ValueError(f"cannot reshape {self.shape} into {tuple(shape)}")
        return out

    def rows(self, start, stop):
        """View of rows [start, stop) along the first axis."""
        start, stop = int(start), int(stop)
        if not 0 <= start <= stop <= self.shape[0]:
            raise IndexError("row range out of bounds")
        row = self.size // self.shape[0] if self.shape[0] else 0
        return DeviceArray((stop - start,) + self.shape[1:], self.dtype,
                           ptr=self.ptr + start * row * self.dtype.itemsize, base=self.base or self,
                           layout=self.layout)

    def copy_from_host(self, host, stream=None):
        host = np.ascontiguousarray(host, dtype=self.dtype)
        if host.size != self.size:
            raise ValueError("size mismatch in copy_from_host")
        _lib.call("smm_memcpy_h2d", ctypes.c_void_p(self.ptr), host.ctypes.data_as(ctypes.c_void_p),
                  self.nbytes, _stream_handle(stream))
        return self

    def to_host(self, out=None, stream=None):
        if out is None:
            out = np.empty(self.shape, dtype=self.dtype)
        if out.nbytes != self.nbytes or not out.flags.c_contiguous:
            raise ValueError("to_host needs a C-contiguous buffer of the same size")
        _lib.call("smm_memcpy_d2h", out.ctypes.data_as(ctypes.c_void_p), ctypes.c_void_p(self.ptr),
                  self.nbytes, _stream_handle(stream))
        if stream is not None:
            _lib.call("smm_stream_sync", _stream_handle(stream))
        return out

    def fill_bytes(self, value=0, stream=None):
        _lib.call("smm_memset", ctypes.c_void_p(self.ptr), int(value), self.nbytes,
                  _stream_handle(stream))
        return self

    def fill_random(self, seed, mean=0.0, sigma=1.0, stream=None):
        """Counter-based pseudo-normal fill on the device (benchmarks, full-size tests)."""
        _lib.call("smm_fill_random", ctypes.c_void_p(self.ptr), dtype_code(self.dtype), self.size,
                  ctypes.c_uint64(int(seed) & 0xFFFFFFFFFFFFFFFF), float(mean), float(sigma),
                  _stream_handle(stream))
        return self

    def free(self):
        if self._owned and self.ptr:
            _lib.call("smm_free", ctypes.c_void_p(self.ptr))
        self.ptr = 0
        self._owned = False

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def __repr__(self):
        return f"DeviceArray(shape={self.shape}, dtype={self.dtype}, layout={self.layout!r}, ptr=0x{self.ptr:x})"


def to_device(host, dtype=None, stream=None, layout="bs"):
    """Upload a host array.  layout="sb" tags it as a batch-fastest field (the array must already be
    ordered cells first, batch last -- e.g. a (lat, lon, time) field)."""
    host = np.asarray(host)
    if dtype is None:
        dtype = host.dtype
    return DeviceArray(host.shape, dtype, layout=layout).copy_from_host(host, stream=stream)


def aligned_pitch(n_elems, dtype, line_bytes=128):
    """Smallest row pitch (in elements) >= n_elems whose rows start on `line_bytes` boundaries: the
    tile kernels stage whole 128-B lines of a row, a row that starts mid-line costs one more line per
    staged run (config 3's 1442 x 1021 source: 14.0 vs 12.3 ms)."""
    isz = np.dtype(dtype).itemsize
    per = max(1, line_bytes // isz)
    return -(-int(n_elems) // per) * per


def to_device_pitched(host, dtype=None, stream=None):
    """Upload a host field of shape (..., S) into a DeviceArray of shape (..., pitch) whose rows start
    on 128-B lines (pitch = aligned_pitch(S)); pass it to SparseOperator.apply / OperatorGroup.apply
    as it is (they take the last axis as the row pitch)."""
    host = np.ascontiguousarray(host, dtype=dtype)
    n = host.shape[-1]
    pitch = aligned_pitch(n, host.dtype)
    out = DeviceArray(host.shape[:-1] + (pitch,), host.dtype)
    rows = host.size // n if n else 0
    isz = host.dtype.itemsize
    if rows and n:
        _lib.call("smm_memcpy2d_h2d", ctypes.c_void_p(out.ptr), pitch * isz, host.ctypes.data_as(ctypes.c_void_p),
                  n * isz, n * isz, rows, _stream_handle(stream))
    return out


def packed_out(out, total):
    """out -- given or fresh -- as the uint8 `DeviceArray` a device step writes at most `total` packed bytes into."""
    if out is None:
        return DeviceArray((max(total, 4),), np.uint8)
    if not isinstance(out, DeviceArray) or out.dtype != np.uint8 or out.nbytes < total:
        raise ValueError(f"out must be a uint8 DeviceArray of at least {total} bytes")
    return out


def grib_pack(y, enc, n_points=None, out=None, stream=None):
    """Pack a float64 `DeviceArray` (..., ld) into GRIB simple packing on the device (smm_grib_pack): every leading
    index is one field of n_points cells (default: the whole last axis; a smaller n_points leaves the row's tail
    unread).  enc: a `GribEncode`.  Returns (DeviceArray of uint8 in the layout of `enc.layout`, GRIB_ROW_DTYPE
    records, GRIB_BITMAP_DTYPE records) -- what `SparseOperator.apply_grib(x, rows, bitmaps=bitmaps)` takes as it is,
    and bytewise what `enc.encode` gives for the same values.  out: a uint8 DeviceArray to pack into (at least the
    layout's bytes).  The stream is synchronised on return."""
    from .griblite import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE
    if not isinstance(y, DeviceArray) or y.dtype != np.float64 or y.ndim < 1:
        raise TypeError("grib_pack takes a float64 DeviceArray")
    ld = y.shape[-1]
    n_points = ld if n_points is None else int(n_points)
    n_fields = y.size // ld if ld else 0
    _, total = enc.layout(n_points, n_fields)
    out = packed_out(out, total)
    rec = enc.records(n_fields)
    rows = np.zeros(n_fields, dtype=GRIB_ROW_DTYPE)
    bitmaps = np.zeros(n_fields, dtype=GRIB_BITMAP_DTYPE)
    _lib.call("smm_grib_pack", current_device(), ctypes.c_void_p(y.ptr), ld, n_points, n_fields,
              ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)), ctypes.c_void_p(out.ptr), out.nbytes,
              ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
              ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), _stream_handle(stream))
    return out, rows, bitmaps


def grib_unpack(device_bytes, rows, ccsds, x_bytes=None, out=None, stream=None):
    """Turn the CCSDS streams of GRIB-2 fields (template 5.42) resident in HBM into simple-packed streams on the device
    (smm_grib_aec_unpack).  device_bytes: a uint8 `DeviceArray` holding the streams (the array must cover x_bytes
    rounded up to 4); rows: one GRIB_ROW_DTYPE record per field (its R, 2^E, 10^D and width); ccsds: one GRIB_AEC_DTYPE
    record per field (where its stream lies, how many integers it codes, block size, interval, flags).  Returns
    (DeviceArray of uint8, GRIB_ROW_DTYPE records): each field's integers big-endian with the field's own width at a
    4-byte-aligned offset -- what `SparseOperator.apply_grib(x, rows, bitmaps=...)` takes as it is.  A field of width 0
    passes through untouched.  out: a uint8 DeviceArray to unpack into.  The stream is synchronised on return."""
    from . import _grib
    return _grib.unpack_device("grib_unpack", device_bytes, rows, x_bytes, out, stream, ccsds=ccsds)[:2]


def grib_unpack_cpx(device_bytes, rows, cpx, x_bytes=None, out=None, stream=None):
    """Turn the complex-packed streams of GRIB-2 fields (templates 5.2 / 5.3) resident in HBM into simple-packed streams
    on the device (smm_grib_cpx_unpack).  device_bytes: a uint8 `DeviceArray` holding the streams (the array must cover
    x_bytes rounded up to 4); rows: one GRIB_ROW_DTYPE record per field (its R, 2^E, 10^D; nbits is not read); cpx: one
    GRIB_CPX_DTYPE record per field (where section 7's bytes lie, how many integers they code, section 5's group
    parameters).  Returns (DeviceArray of uint8, GRIB_ROW_DTYPE records): each field's integers big-endian at the start
    of a slot of 4 bytes per value, with the field's own minimal width -- the bit length of its largest integer, which
    the returned record's nbits holds -- what `SparseOperator.apply_grib(x, rows, bitmaps=...)` takes as it is.  A field
    whose record is marked GRIB_CPX_SIMPLE passes through untouched.  out: a uint8 DeviceArray to unpack into.  The
    stream is synchronised on return."""
    from . import _grib
    return _grib.unpack_device("grib_unpack_cpx", device_bytes, rows, x_bytes, out, stream, cpx=cpx)[:2]


def grib_unpack_cpx_mv(device_bytes, rows, cpx, missing, x_bytes=None, out=None, stream=None):
    """`grib_unpack_cpx` for fields whose missing values are coded inside the groups (smm_grib_cpx_unpack_mv).  missing:
    one uint8 per field, section 5's missing value management -- 0, or 1 / 2 (the rule: smm_grib_cpx.hpp) -- or None
    for all zero.  Returns (out, rows_out, bitmaps_out): a field with missing != 0 gets its P present integers at its
    slot's start at their own minimal width and, behind the slot, a bitmap of n_values bits (MSB first);
    bitmaps_out -- GRIB_BITMAP_DTYPE records -- says where that bitmap lies in `out` and P, and GRIB_NO_BITMAP for the
    other fields: rows_out and bitmaps_out are what `SparseOperator.apply_grib(out, rows_out, bitmaps=bitmaps_out)`
    takes."""
    from . import _grib
    missing = np.zeros(np.size(cpx), dtype=np.uint8) if missing is None else missing
    return _grib.unpack_device("grib_unpack_cpx_mv", device_bytes, rows, x_bytes, out, stream, cpx=cpx, cpx_missing=missing)


def grib_aec_pack(device_bytes, rows, ccsds, x_bytes=None, out=None, stream=None):
    """Code simple-packed streams resident in HBM as the CCSDS streams of GRIB-2 template 5.42 on the device
    (smm_grib_aec_pack) -- the twin of `grib_unpack`, and what follows `grib_pack` when results leave CCSDS-packed.
    device_bytes: a uint8 `DeviceArray` (it must cover x_bytes rounded up to 4); rows: one GRIB_ROW_DTYPE record per
    field -- where its integers begin, their width; ccsds: one GRIB_AEC_DTYPE record per field with the parameters wanted
    (n_values and nbits as the field has them, block_size, rsi, flags; `GribEncode.ccsds_records`).  Returns
    (DeviceArray of uint8 cut to the bytes used, the rows with byte_off at their streams, GRIB_AEC_DTYPE records with
    byte_off and byte_len set): the streams lie back to back in field order, each at a 4-byte-aligned offset, bytewise what
    `griblite.aec_encode` gives.  A field of width 0 has no stream (byte_len 0, block_size 0).  out: a uint8 DeviceArray of
    at least the bound (smm_grib_aec_pack_bound) to code into.  The stream is synchronised on return."""
    from . import _grib
    return _grib.pack_device("grib_aec_pack", device_bytes, rows, x_bytes, out, stream, ccsds=ccsds)


def grib_cpx_pack(device_bytes, rows, cpx, x_bytes=None, out=None, stream=None):
    """Code simple-packed streams resident in HBM as the complex-packed streams of GRIB-2 templates 5.2 / 5.3 on the
    device (smm_grib_cpx_pack) -- the twin of `grib_unpack_cpx`, and what follows `grib_pack` when results leave
    complex-packed.  device_bytes: a uint8 `DeviceArray` (it must cover x_bytes rounded up to 4); rows: one GRIB_ROW_DTYPE
    record per field -- where its integers begin, their width; cpx: one GRIB_CPX_DTYPE record per field with the
    parameters wanted (n_values and nbits as the field has them, order, length_ref = the group length;
    `GribEncode.cpx_records`, `griblite.cpx_want`).  Returns (DeviceArray of uint8 cut to the bytes used, the rows with
    byte_off at their streams -- nbits stays the width of the integers --, the full GRIB_CPX_DTYPE records of the streams
    written): the streams lie back to back in field order, each at a 4-byte-aligned offset, bytewise what
    `griblite.cpx_encode` gives.  A field of width 0 is not coded (byte_len 0, order GRIB_CPX_SIMPLE).  out: a uint8 DeviceArray of at least the bound (smm_grib_cpx_pack_bound) to code into.  The stream is synchronised
    on return."""
    from . import _grib
    return _grib.pack_device("grib_cpx_pack", device_bytes, rows, x_bytes, out, stream, cpx=cpx)


def empty(shape, dtype=np.float64):
    if not isinstance(shape, tuple):
        shape = tuple(np.atleast_1d(shape).tolist())
    return DeviceArray(shape, dtype)


class _PinnedBlock:
    """Owner of one hipHostMalloc allocation (kept alive by the numpy array's base)."""

    def __init__(self, nbytes):
        h = ctypes.c_void_p()
        _lib.call("smm_host_alloc", ctypes.byref(h), max(int(nbytes), 1))
        self.ptr = h.value
        self.nbytes = int(nbytes)

    def __del__(self):
        try:
            if self.ptr:
                _lib.call("smm_host_free", ctypes.c_void_p(self.ptr))
                self.ptr = None
        except Exception:
            pass


def pinned_empty(shape, dtype=np.float64):
    """numpy array in page-locked host memory: smm_apply_host DMAs it without staging copies."""
    dtype = np.dtype(dtype)
    shape = tuple(int(s) for s in (shape if isinstance(shape, (tuple, list)) else (shape,)))
    n = int(np.prod(shape)) if shape else 1
    block = _PinnedBlock(n * dtype.itemsize)
    buf = (ctypes.c_char * max(block.nbytes, 1)).from_address(block.ptr)
    arr = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
    _PINNED_KEEPALIVE[id(buf)] = block
    import weakref
    weakref.finalize(buf, _PINNED_KEEPALIVE.pop, id(buf), None)
    return arr


_PINNED_KEEPALIVE = {}


class _ResultCache:
    """Page-locked buffers for the RESULTS of the host pipelines ("direct write of Y tiles to the consumer").

    `SparseOperator.apply_host` / `OperatorGroup.apply_host` return a fresh array per call, as the reference does.  A fresh
    pageable array costs its first-touch page faults inside the pipeline's copy-out and a staging copy (config 2, 512 rows:
    10 of 33 ms); a page-locked one is written by the DMA engine directly.  But hipHostMalloc is slow (it pins every page:
    ~0.17 s per GB), so it never runs on the caller's path: a call that finds no fitting block gets an ordinary array at once
    and a block of that size is prepared in the background; when the numpy array a block backs is garbage-collected the block
    returns to the cache instead of being freed.  A caller that regrids in a loop therefore gets page-locked results from its
    second or third call on (512 rows: 33.6 -> 26 ms, 2048 rows: 101 -> 80 ms); a single call is as before.  Bounded: at most
    `max_cached` bytes wait in the cache, at most `max_live` bytes are handed out at a time, small results are ordinary arrays,
    a failing hipHostMalloc just leaves the cache empty.  `SMM_RESULT_CACHE=0` switches it off."""

    def __init__(self, min_bytes=8 << 20, max_cached=4 << 30, max_live=16 << 30):
        import threading
        self.min_bytes, self.max_cached, self.max_live = int(min_bytes), int(max_cached), int(max_live)
        self.free = []            # (nbytes, _PinnedBlock), smallest first
        self.cached = 0           # bytes waiting in `free`
        self.live = 0             # bytes of blocks backing arrays that are still alive
        self.pending = {}         # nbytes -> thread preparing a block of that size
        self.lock = threading.RLock()      # re-entrant: a finaliser may fire inside a locked region of the same thread
        self.hits = self.misses = 0

    def _add(self, block):
        with self.lock:
            if self.cached + block.nbytes <= self.max_cached:
                self.free.append((block.nbytes, block))
                self.free.sort(key=lambda e: e[0])
                self.cached += block.nbytes
                return True
        return False              # the caller drops the block: its __del__ frees it

    def _release(self, key):
        block = _PINNED_KEEPALIVE.pop(key, None)
        if block is not None:
            with self.lock:
                self.live -= block.nbytes
            self._add(block)

    def _prepare(self, nbytes, device):
        try:
            if device is not None:
                _lib.call("smm_set_device", int(device))
            self._add(_PinnedBlock(nbytes))
        except Exception:          # cannot pin that much (or no device any more): ordinary arrays keep doing the job
            pass
        finally:
            with self.lock:
                self.pending.pop(nbytes, None)

    def wait(self, timeout=30.0):
        """Block until the background preparations in flight are done (tests, benchmarks of the steady state)."""
        with self.lock:
            threads = [th for th in self.pending.values() if th is not None]
        for th in threads:
            th.join(timeout)

    def empty(self, shape, dtype):
        """A C-contiguous array of `shape` / `dtype`: a recycled page-locked block if one fits, else np.empty."""
        import os
        import threading
        import weakref
        dtype = np.dtype(dtype)
        shape = tuple(int(v) for v in shape)
        n = int(np.prod(shape)) if shape else 1
        nbytes = n * dtype.itemsize
        if nbytes < self.min_bytes or os.environ.get("SMM_RESULT_CACHE") == "0":
            return np.empty(shape, dtype)
        block, spawn = None, False
        with self.lock:       # short, allocation-free where it can be: a finaliser (`_release`) may run whenever memory is allocated
            if self.live + nbytes <= self.max_live:
                for entry in self.free:
                    if nbytes <= entry[0] <= 2 * nbytes + (1 << 20):          # a fitting block, not a much larger one
                        block = entry[1]
                        break
                if block is not None:
                    self.free.remove(entry)
                    self.cached -= block.nbytes
                    self.live += block.nbytes
                    self.hits += 1
                else:
                    self.misses += 1
                    if nbytes not in self.pending and self.cached + nbytes <= self.max_cached:
                        self.pending[nbytes] = None                            # reserved; the thread is made outside the lock
                        spawn = True
        if spawn:
            try:
                dev = current_device()
            except Exception:
                dev = None
            th = threading.Thread(target=self._prepare, args=(nbytes, dev), daemon=True)
            with self.lock:
                self.pending[nbytes] = th
            th.start()
        if block is None:
            return np.empty(shape, dtype)
        buf = (ctypes.c_char * max(block.nbytes, 1)).from_address(block.ptr)
        arr = np.frombuffer(buf, dtype=dtype, count=n).reshape(shape)
        _PINNED_KEEPALIVE[id(buf)] = block
        weakref.finalize(buf, self._release, id(buf))
        return arr

    def clear(self):
        self.wait()
        with self.lock:
            self.free, self.cached = [], 0


result_cache = _ResultCache()


def _join_result_cache():      # interpreter exit: no thread may still be inside hipHostMalloc when the runtime goes away
    try:
        result_cache.wait(timeout=10.0)
    except Exception:
        pass


import atexit  # noqa: E402

atexit.register(_join_result_cache)
