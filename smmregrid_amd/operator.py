"""Sparse regrid operators resident in HBM.

`SparseOperator` stands where the reference keeps a lazy
``dask.array`` of one ``sparse.COO`` of shape (S, D) (weights.py:37-42);
`OperatorGroup` stands where it keeps the per-level Python list
(weights.py:18-23).
"""
import ctypes
import time

import numpy as np

from . import _grib, _lib
from .device import (DeviceArray, bfloat16, check_half_pair, dtype_code, field_dtype_code, is_half_dtype,
                     is_packed_dtype, result_cache, result_dtype, _stream_handle, current_device, grib_pack)


def _cptr(a):
    return None if a is None else a.ctypes.data_as(ctypes.c_void_p)


def _ptr(a):
    return _cptr(a) if isinstance(a, np.ndarray) else ctypes.c_void_p(a.ptr)


def _apply_call(entry, handle, x, mid, y, rest, y_res, cf, cf_out, y_name="Y"):
    """One apply through `entry`: the plain entry, `entry`_cf with a CFDecode (cf), `entry`_pk with a CFEncode (cf_out).
    The arguments are handle, X, its dtype code, *mid, Y, its dtype code, *rest, then the rule structs the entry takes.
    y_res: result_dtype(out_dtype, cf_out) -- what the result array of a cf_out call must be.  Returns y."""
    rules = []
    if is_half_dtype(x.dtype) or is_half_dtype(y.dtype):
        if cf is not None or cf_out is not None:
            raise TypeError("float16 / bfloat16 fields and results take no CFDecode / CFEncode rule")
        check_half_pair(x.dtype, y.dtype)      # an unbuilt pairing names the built ones
    if cf_out is not None:
        if y.dtype != y_res[0]:
            raise TypeError(f"{y_name} must be {y_res[0]} for this cf_out, got {y.dtype}")
        entry, y_code = entry + "_pk", y_res[1]
        rules = [None if cf is None else ctypes.byref(cf._struct(x.dtype)), ctypes.byref(cf_out._struct())]
    else:
        y_code = dtype_code(y.dtype)
    x_code = field_dtype_code(x.dtype, cf)
    if cf is not None and cf_out is None:
        entry, rules = entry + "_cf", [ctypes.byref(cf._struct(x.dtype))]
    _lib.call(entry, handle, _ptr(x), x_code, *mid, _ptr(y), y_code, *rest, *rules)
    return y


def _host_field(x, cf, half):
    """A host field as the host entries ship it: float32 / float64 and raw CF-packed integers as they are, `bfloat16`
    as it is, float16 as it is with half=True; anything else -- float16 by default -- is promoted to float64
    (result_type(x, f64), regrid.py:550)."""
    x = np.asarray(x)
    if cf is not None and not is_packed_dtype(x.dtype):
        raise TypeError(f"a CFDecode rule goes with a raw int16 / uint16 field, not {x.dtype}")
    if cf is None and x.dtype not in (np.float32, np.float64) and x.dtype != bfloat16 \
            and not (half and x.dtype == np.float16):
        x = x.astype(np.float64)
    return x


def _device_result(y, shape, dtype, layout="bs"):
    """y, or without one a fresh DeviceArray for the result; a y of another shape is refused."""
    if y is None:
        return DeviceArray(shape, dtype, layout=layout)
    if y.shape != shape:
        raise ValueError(f"Y must be {shape}, got {y.shape}")
    return y


class _Handle:
    """Owns one handle of the library; `_destroy` names the entry that releases it."""

    def close(self):
        if getattr(self, "handle", None):
            _lib.call(self._destroy, self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _flags(flags, masked=False, skipna=False, sb_packed=False, y_sb=False):
    """The `flags` word of an apply entry: the caller's bits and those its keywords stand for."""
    return int(flags) | (_lib.APPLY_MASKED if masked else 0) | (_lib.APPLY_SKIPNA if skipna else 0) | \
        (_lib.APPLY_SB_PACKED if sb_packed else 0) | (_lib.APPLY_SB_Y_SB if y_sb else 0)


def _level_result(n_outer, n_lev, n_inner, n_dst, transpose):
    """(shape, (outer, lev, inner) strides in cells) of a level group's result: (n_outer, n_inner, n_lev, D) when
    transpose (regrid.py:420-427) else (n_lev, n_outer, n_inner, D) (the concat order, regrid.py:410)."""
    if transpose:
        return (n_outer, n_inner, n_lev, n_dst), (n_inner * n_lev * n_dst, n_dst, n_lev * n_dst)
    return (n_lev, n_outer, n_inner, n_dst), (n_inner * n_dst, n_outer * n_inner * n_dst, n_dst)


def _launch_info(fn, handle, dt, sizes, flags):
    ints = [ctypes.c_int(0) for _ in range(5)]
    nb, lds = ctypes.c_int64(0), ctypes.c_int64(0)
    _lib.call(fn, handle, dt, *sizes, int(flags), ctypes.byref(ints[0]), ctypes.byref(ints[1]),
              ctypes.byref(ints[2]), ctypes.byref(ints[3]), ctypes.byref(nb), ctypes.byref(lds),
              ctypes.byref(ints[4]))
    return {"kernel": ("sell", "tile", "tile-dma")[ints[0].value], "j_per_block": ints[1].value,
            "rows_per_step": ints[2].value, "rows_per_block": ints[3].value, "n_blocks": nb.value,
            "lds_bytes": lds.value, "big_operator": bool(ints[4].value)}


class SparseOperator(_Handle):
    """(S x D) weights matrix in HBM, built from SCRIP links (weights.py:25-44)."""
    _destroy = "smm_operator_destroy"

    def __init__(self, n_src, n_dst, src_address, dst_address, remap_matrix, device=None, dst_dims=None,
                 prune_zeros=False, columns=False):
        """dst_dims: shape of the destination grid as the weights file gives it (`dst_grid_dims`,
        fastest dimension first); kept as metadata (save / load).
        prune_zeros: drop links whose weight is exactly zero (bilinear weights between aligned grids are
        mostly zeros); results stay bit-identical because every gathered value is finite after the fill.
        columns: keep every column of a 2-D remap_matrix (smm_operator_create_cols; 1..4 columns) -- the gradient
        weights of bicubic and second-order conservative files, which `apply(..., gradients=rule)` applies.  Column 0
        of such an operator is the operator built without `columns`, and everything else works on it as before;
        prune_zeros then drops a link only when all its columns are zero."""
        src = np.ascontiguousarray(src_address, dtype=np.int32).ravel()
        dst = np.ascontiguousarray(dst_address, dtype=np.int32).ravel()
        w = np.asarray(remap_matrix, dtype=np.float64)
        keep_cols = bool(columns) and w.ndim == 2
        if keep_cols:
            w = np.ascontiguousarray(w)
            n_links = w.shape[0]
        else:
            if w.ndim == 2:
                w = w[:, 0]          # only the first weight column is used (weights.py:33)
            w = np.ascontiguousarray(w).ravel()
            n_links = w.size
        if not (src.size == dst.size == n_links):
            raise ValueError("src_address, dst_address and remap_matrix differ in length")
        if device is None:
            device = current_device()
        self.device = int(device)
        h = ctypes.c_void_p()
        t0 = time.perf_counter()
        options = _lib.CREATE_PRUNE_ZEROS if prune_zeros else 0
        if keep_cols:
            _lib.call("smm_operator_create_cols", int(n_src), int(n_dst), int(src.size), _cptr(src), _cptr(dst),
                      _cptr(w), int(w.shape[1]), options, self.device, ctypes.byref(h))
        else:
            _lib.call("smm_operator_create_opt", int(n_src), int(n_dst), int(src.size), _cptr(src),
                      _cptr(dst), _cptr(w), options, self.device, ctypes.byref(h))
        self.create_ms = (time.perf_counter() - t0) * 1e3     # sort + duplicate sum + layouts + upload
        self.dst_dims = None if dst_dims is None else tuple(int(v) for v in np.asarray(dst_dims).ravel())
        self._adopt(h)

    def _adopt(self, handle):
        self.handle = handle
        vals = [ctypes.c_int64(0) for _ in range(5)]
        _lib.call("smm_operator_info", self.handle, *[ctypes.byref(v) for v in vals])
        self.n_src, self.n_dst, self.nnz, self.n_used_src, self.max_row_nnz = [v.value for v in vals]
        n_cols = ctypes.c_int(1)
        _lib.call("smm_operator_cols", self.handle, ctypes.byref(n_cols))
        self.n_cols = n_cols.value      # weight columns kept (SparseOperator(..., columns=True)); 1 otherwise
        self.has_imask = False
        self.has_frac = False

    @classmethod
    def from_csr(cls, n_src, n_dst, rowptr, col, val, device=None, dst_dims=None):
        """Operator from a canonical CSR (what export_csr returned): no sort, no duplicate pass.
        A non-canonical CSR (unsorted or repeated columns, bad rowptr) is a ValueError."""
        rowptr = np.ascontiguousarray(rowptr, dtype=np.int64).ravel()
        col = np.ascontiguousarray(col, dtype=np.int32).ravel()
        val = np.ascontiguousarray(val, dtype=np.float64).ravel()
        if rowptr.size != int(n_dst) + 1:
            raise ValueError(f"rowptr has {rowptr.size} entries, expected n_dst + 1 = {int(n_dst) + 1}")
        if col.size != val.size or (rowptr.size and col.size != rowptr[-1]):
            raise ValueError("col / val length differs from rowptr[-1]")
        self = cls.__new__(cls)
        self.device = int(current_device() if device is None else device)
        h = ctypes.c_void_p()
        self.dst_dims = None if dst_dims is None else tuple(int(v) for v in np.asarray(dst_dims).ravel())
        t0 = time.perf_counter()
        try:
            _lib.call("smm_operator_create_csr", int(n_src), int(n_dst), _cptr(rowptr), _cptr(col),
                      _cptr(val), self.device, ctypes.byref(h))
        except _lib.SmmError as e:
            if e.code == _lib.SMM_ERR_INVALID:
                raise ValueError(str(e)) from None
            raise
        self.create_ms = (time.perf_counter() - t0) * 1e3
        self._adopt(h)
        return self

    def save(self, path):
        """Persist the ready CSR (+ epilogue arrays if given to set_epilogue) as .npz -- the
        'native CSR cache' of SURVEY f1; reload with SparseOperator.load."""
        rowptr, col, val = self.export_csr()
        payload = {"shape": np.array([self.n_src, self.n_dst], dtype=np.int64), "rowptr": rowptr, "col": col,
                   "val": val}
        if getattr(self, "dst_dims", None):
            payload["dst_dims"] = np.asarray(self.dst_dims, dtype=np.int32)
        for name in ("_dst_imask", "_dst_frac"):
            a = getattr(self, name, None)
            if a is not None:
                payload[name[1:]] = a
        np.savez(path, **payload)

    @classmethod
    def load(cls, path, device=None):
        z = np.load(path, allow_pickle=False)
        n_src, n_dst = (int(v) for v in z["shape"])
        op = cls.from_csr(n_src, n_dst, z["rowptr"], z["col"], z["val"], device=device,
                          dst_dims=z["dst_dims"] if "dst_dims" in z.files else None)
        if "dst_imask" in z.files or "dst_frac" in z.files:
            op.set_epilogue(z["dst_imask"] if "dst_imask" in z.files else None,
                            z["dst_frac"] if "dst_frac" in z.files else None)
        return op

    # the reference's matrix is (S, D): keep .shape for code that inspects it
    @property
    def shape(self):
        return (self.n_src, self.n_dst)

    def set_epilogue(self, dst_imask=None, dst_frac=None):
        """dst_grid_imask / dst_grid_frac of the weights file (regrid.py:509-510)."""
        im = None if dst_imask is None else np.ascontiguousarray(dst_imask, dtype=np.int32).ravel()
        fr = None if dst_frac is None else np.ascontiguousarray(dst_frac, dtype=np.float64).ravel()
        for a, name in ((im, "dst_imask"), (fr, "dst_frac")):
            if a is not None and a.size != self.n_dst:
                raise ValueError(f"{name} has {a.size} entries, expected {self.n_dst}")
        _lib.call("smm_operator_set_epilogue", self.handle, _cptr(im), _cptr(fr))
        self._dst_imask, self._dst_frac = im, fr     # kept for save()
        self.has_imask = im is not None
        self.has_frac = fr is not None
        return self

    def export_csr(self):
        """(rowptr int64[D+1], col int32[nnz], val float64[nnz]) -- the canonical CSR."""
        rowptr = np.zeros(self.n_dst + 1, dtype=np.int64)
        col = np.zeros(self.nnz, dtype=np.int32)
        val = np.zeros(self.nnz, dtype=np.float64)
        _lib.call("smm_operator_export_csr", self.handle, _cptr(rowptr), _cptr(col), _cptr(val))
        return rowptr, col, val

    def export_cols(self):
        """Every weight column of the canonical CSR, float64 (nnz, n_cols), the links in `export_csr`'s order."""
        val = np.zeros((self.nnz, self.n_cols), dtype=np.float64)
        _lib.call("smm_operator_export_cols", self.handle, _cptr(val))
        return val

    def _check_rule(self, rule):
        if rule.size != self.n_src:
            raise ValueError(f"the gradient rule's grid has {rule.size} cells, the operator {self.n_src} source cells")

    def gradients(self, x, rule, out=None, stream=None):
        """The gradient planes of a device-resident field x (B, S) -- or (B, ldx >= S) -- of float32 / float64 by
        `rule` (a `GradientRule`), computed on the device (smm_gradients): a float64 DeviceArray (B, n_planes, S),
        bit for bit `rule.gradients` of every row."""
        if not isinstance(x, DeviceArray):
            raise TypeError("SparseOperator.gradients takes a DeviceArray")
        self._check_rule(rule)
        if x.ndim != 2 or x.shape[1] < self.n_src:
            raise ValueError(f"X must be (B, >= {self.n_src}), got {x.shape}")
        shape = (x.shape[0], rule.n_planes, self.n_src)
        if out is None:
            out = DeviceArray(shape, np.float64)
        elif out.shape != shape or out.dtype != np.float64:
            raise ValueError(f"out must be a float64 DeviceArray {shape}")
        _lib.call("smm_gradients", rule.plan(self.device), _ptr(x), dtype_code(x.dtype), x.shape[1], _ptr(out),
                  self.n_src, rule.n_planes * self.n_src, x.shape[0], _stream_handle(stream))
        return out

    def _apply_cols(self, x, y, rule, masked, remap_area_min, out_dtype, flags, stream, scratch_rows, scratch=None):
        """`apply(..., gradients=rule)`: smm_apply_cols.  The planes' scratch -- the caller's, or one made here for
        scratch_rows rows -- lives as long as the result."""
        self._check_rule(rule)
        if x.ndim != 2 or x.shape[1] < self.n_src:
            raise ValueError(f"X must be (B, >= {self.n_src}), got {x.shape}")
        n_batch = x.shape[0]
        y = _device_result(y, (n_batch, self.n_dst), np.dtype(out_dtype))
        per_row = rule.n_planes * self.n_src * 8
        if scratch_rows is None:      # all rows when they fit 256 MiB, else as many as do
            scratch_rows = max(1, min(n_batch, (256 << 20) // max(per_row, 1)))
        if scratch is None:
            scratch = DeviceArray((max(int(scratch_rows), 0) * per_row,), np.uint8)
        fl = _flags(flags, masked)
        _lib.call("smm_apply_cols", self.handle, rule.plan(self.device), _ptr(x), dtype_code(x.dtype), x.shape[1],
                  _ptr(y), dtype_code(y.dtype), self.n_dst, n_batch, float(remap_area_min), fl,
                  ctypes.c_void_p(scratch.ptr), scratch.nbytes, _stream_handle(stream))
        y._scratch = scratch      # the gather may still be reading it when this returns
        return y

    # ------------------------------------------------------------------ categorical fields (largest area fraction)
    _MODE_CODES = {np.dtype(np.float32): _lib.SMM_F32, np.dtype(np.float64): _lib.SMM_F64,
                   np.dtype(np.int16): _lib.SMM_I16, np.dtype(np.uint16): _lib.SMM_U16}

    def _mode_code(self, dtype):
        try:
            return self._MODE_CODES[np.dtype(dtype)]
        except (KeyError, TypeError):
            from .categorical import built_words
            raise TypeError(f"apply_mode is built for {built_words()} class fields, not {dtype}") from None

    def mode_launch_info(self, dtype):
        """How `apply_mode` runs this operator for fields of `dtype` (smm_mode_launch_info; nothing is launched):
        capacity -- the most slots of a slice the LDS form of the kernel takes; lds_slots / lds_bytes -- what a launch
        asks for per wave / per workgroup; lds_slices / global_slices -- the slices that take each form."""
        cap, slots = ctypes.c_int(0), ctypes.c_int(0)
        lds, n_lds, n_glob = ctypes.c_int64(0), ctypes.c_int64(0), ctypes.c_int64(0)
        _lib.call("smm_mode_launch_info", self.handle, self._mode_code(dtype), ctypes.byref(cap), ctypes.byref(slots),
                  ctypes.byref(lds), ctypes.byref(n_lds), ctypes.byref(n_glob))
        return {"capacity": cap.value, "lds_slots": slots.value, "lds_bytes": lds.value, "lds_slices": n_lds.value,
                "global_slices": n_glob.value}

    def apply_mode(self, x, y=None, masked=False, remap_area_min=0.0, fill=(), fill_out=None, share=False, flags=0,
                   stream=None):
        """A field of class codes regridded by largest area fraction (smm_apply_mode): per destination cell and batch
        row, the value whose links carry the largest summed weight -- `categorical.ModeRule.apply`, bit for bit.  Meant
        for conservative weights; `method="laf"` weights are the one-cell approximation of it.
        x: a `DeviceArray` (B, S) -- or (B, ldx >= S) -- of float32 / float64 (missing: whatever is not finite) or
        int16 / uint16 (missing: the raw values in `fill`, at most two); fill_out: what a dead row of an integer field
        stores (default: the first of `fill`), a float field's dead rows are NaN.  y: a DeviceArray of x's dtype,
        (B, ldy >= D), or None.  share: True -- the winner's summed weight comes back too, float64 (B, D); a float64
        DeviceArray (B, ld_share >= D) is filled instead of a fresh one.  Returns y, or (y, share)."""
        if not isinstance(x, DeviceArray):
            raise TypeError("SparseOperator.apply_mode takes a DeviceArray (apply_mode_host for host data)")
        if x.layout == "sb":
            raise ValueError("apply_mode takes the native (B, S) layout: no batch-fastest field")
        from .categorical import ModeRule
        code = self._mode_code(x.dtype)
        fills, fill_out = ModeRule(fill, fill_out).checked(x.dtype)
        if x.ndim != 2 or x.shape[1] < self.n_src:
            raise ValueError(f"X must be (B, >= {self.n_src}), got {x.shape}")
        n_batch = x.shape[0]
        if y is None:
            y = DeviceArray((n_batch, self.n_dst), x.dtype)
        elif not isinstance(y, DeviceArray) or y.ndim != 2 or y.shape[0] != n_batch or y.shape[1] < self.n_dst \
                or y.dtype != x.dtype:
            raise ValueError(f"Y must be a {x.dtype} DeviceArray ({n_batch}, >= {self.n_dst})")
        sh = None
        if isinstance(share, DeviceArray):
            sh = share
            if sh.ndim != 2 or sh.shape[0] != n_batch or sh.shape[1] < self.n_dst or sh.dtype != np.float64:
                raise ValueError(f"share must be a float64 DeviceArray ({n_batch}, >= {self.n_dst})")
        elif share:
            sh = DeviceArray((n_batch, self.n_dst), np.float64)
        rule = None
        if x.dtype.kind != "f":
            rule = _lib.ModeRuleStruct(len(fills), (ctypes.c_int32 * 2)(*(list(fills) + [0, 0])[:2]), int(fill_out), 0)
        _lib.call("smm_apply_mode", self.handle, _ptr(x), code, x.shape[1], _ptr(y), y.shape[1],
                  None if sh is None else _ptr(sh), 0 if sh is None else sh.shape[1], n_batch, float(remap_area_min),
                  _flags(flags, masked), None if rule is None else ctypes.byref(rule), _stream_handle(stream))
        return y if sh is None else (y, sh)

    def apply_mode_host(self, x, out=None, masked=False, remap_area_min=0.0, fill=(), fill_out=None, share=False,
                        flags=0, chunk_rows=0):
        """`apply_mode` for a host (numpy) array of shape (B, S).  This is the first form of that road: a synchronous
        loop over chunks of rows -- H2D copy of the chunk, smm_apply_mode, D2H copy -- which overlaps nothing.  A
        chunk's X, Y and share stay within 256 MiB and a quarter of the free device memory; chunk_rows > 0 fixes the
        rows per chunk.  int8 / uint8 fields -- the usual type of land-cover classes -- are widened exactly to int16 on
        the host and the result is narrowed back; fill and fill_out must then be values of the original type.  Any other
        dtype (int32, int64, ...) is a TypeError.  Returns a (B, D) array of x's dtype, or (y, share)."""
        from .categorical import BUILT_DTYPES, WIDENED_DTYPES, ModeRule, built_words
        x = np.asarray(x)
        own = x.dtype
        if own not in BUILT_DTYPES and own not in WIDENED_DTYPES:
            raise TypeError(f"apply_mode_host is built for {built_words()} class fields, not {own}")
        fills, fill_out = ModeRule(fill, fill_out).checked(own)      # of the ORIGINAL type: the result is narrowed back
        if x.ndim != 2 or x.shape[1] != self.n_src:
            raise ValueError(f"X must be (B, {self.n_src}), got {x.shape}")
        work = np.dtype(np.int16) if own in WIDENED_DTYPES else own
        n_batch = x.shape[0]
        if out is None:
            out = np.empty((n_batch, self.n_dst), dtype=own)
        if out.shape != (n_batch, self.n_dst) or not out.flags.c_contiguous or out.dtype != own:
            raise ValueError(f"out must be a C-contiguous {own} ({n_batch}, {self.n_dst}) array")
        share_out = np.empty((n_batch, self.n_dst), dtype=np.float64) if share else None
        if n_batch == 0:
            return (out, share_out) if share else out
        if chunk_rows <= 0:
            from .device import mem_info
            per_row = self.n_src * work.itemsize + self.n_dst * (work.itemsize + (8 if share else 0))
            budget = min(256 << 20, mem_info()[0] // 4)
            chunk_rows = max(1, budget // max(per_row, 1))
        chunk_rows = min(int(chunk_rows), n_batch)
        dx = DeviceArray((chunk_rows, self.n_src), work)
        dy = DeviceArray((chunk_rows, self.n_dst), work)
        ds = DeviceArray((chunk_rows, self.n_dst), np.float64) if share else None
        for r0 in range(0, n_batch, chunk_rows):
            r1 = min(n_batch, r0 + chunk_rows)
            xc, yc = dx.rows(0, r1 - r0), dy.rows(0, r1 - r0)
            xc.copy_from_host(x[r0:r1].astype(work, copy=False))
            self.apply_mode(xc, yc, masked=masked, remap_area_min=remap_area_min, fill=fills, fill_out=fill_out,
                            share=ds.rows(0, r1 - r0) if share else False, flags=flags)
            if work == own:
                yc.to_host(out=out[r0:r1])      # a blocking copy on the default stream: the chunk is done
            else:
                out[r0:r1] = yc.to_host().astype(own)      # every value is a source value or fill_out: it fits
            if share:
                ds.rows(0, r1 - r0).to_host(out=share_out[r0:r1])
        return (out, share_out) if share else out

    def plan_info(self):
        kind = ctypes.c_int(0)
        lds = ctypes.c_int64(0)
        staged = ctypes.c_int64(0)
        _lib.call("smm_operator_plan_info", self.handle, ctypes.byref(kind), ctypes.byref(lds),
                  ctypes.byref(staged))
        return {"tile_plan": bool(kind.value & 1), "tile_preferred": bool(kind.value & 2),
                "lds_bytes": lds.value, "staged_src_elems": staged.value,
                "rows_per_block": kind.value >> 8}

    def launch_info(self, n_batch, dtype=np.float64, flags=0):
        """Launch geometry `apply` would use for `n_batch` rows (nothing is launched).  dtype int16 / uint16: a
        CF-packed field given with `cf=` (always the SELL kernel)."""
        code = field_dtype_code(dtype, cf=True) if is_packed_dtype(dtype) else dtype_code(np.dtype(dtype))
        return _launch_info("smm_operator_launch_info", self.handle, code, (int(n_batch),), flags)

    def mask_apply(self, src_imask):
        """weights.py:47-52 on the device: (src_imask . W) < 0.5 ? 0 : 1."""
        src = np.ascontiguousarray(src_imask, dtype=np.int32).ravel()
        if src.size != self.n_src:
            raise ValueError(f"src_imask has {src.size} entries, expected {self.n_src}")
        out = np.empty(self.n_dst, dtype=np.int32)
        _lib.call("smm_operator_mask_apply", self.handle, _cptr(src), _cptr(out))
        return out

    def apply(self, x, y=None, masked=False, remap_area_min=0.0, out_dtype=np.float64,
              flags=0, stream=None, keep_batch_fastest=False, skipna=False, cf=None, cf_out=None, gradients=None,
              scratch_rows=None, scratch=None):
        """Y = epilogue(fill(X) . W) for a device-resident X of shape (B, S), or (B, ldx) with a
        padded row pitch ldx >= S (rows that start on 128-B lines are staged without straddling).
        A field tagged batch-fastest (`x.layout == "sb"`, shape (S, B)) goes through the batch-fastest
        kernel (`apply_sb`); with keep_batch_fastest the result stays batch-fastest too, (D, B).
        x float16 / `bfloat16` (2-byte elements widened exactly to float32 in the kernel, then treated as a float32
        field) and out_dtype float16 / `bfloat16` (the float64 result stored with one correctly rounded conversion) are
        built for the pairs of `device.HALF_PAIRS`; any other pairing with a half type is a TypeError.
        skipna: non-finite source values drop out of each batch row's sums and the row is renormalised over
        the valid weight (SMM_APPLY_SKIPNA; rows without one are bit-identical to the plain apply).
        cf: a `CFDecode` -- x holds the raw int16 / uint16 of a CF-packed field, decoded inside the kernel
        (bit-identical to applying `cf.decode` on the host first; float64 results only).
        cf_out: a `CFEncode` -- the result is stored as raw int16 / uint16, encoded inside the kernel's stores
        (bit-identical to `cf_out.encode` of the float64 result; out of range -> fill value, never wrapped).
        gradients: a `GradientRule` -- every weight column of an operator built with columns=True is applied
        (smm_apply_cols): the gradient planes of each batch row are computed on the device and gathered beside the
        field, sum over links of w0 * f + w1 * g1 + ...  float32 / float64 fields in the native (B, S) layout to
        float64 results; skipna, a half or float32 out_dtype and the forced tile kernel are refused by the library
        (SMM_ERR_UNSUPPORTED), cf / cf_out / a batch-fastest field here.  scratch_rows: batch rows whose planes the
        scratch holds at a time (default: all of them up to 256 MiB); scratch: a DeviceArray to hold them instead of
        one made by the call (its bytes decide how many rows a round takes)."""
        if not isinstance(x, DeviceArray):
            raise TypeError("SparseOperator.apply takes a DeviceArray (use Regridder for host data)")
        if gradients is not None:
            if x.layout == "sb" or keep_batch_fastest or cf is not None or cf_out is not None:
                raise ValueError("gradients= goes with float32 / float64 fields in the native (B, S) layout and float64 "
                                 "results: no batch-fastest field, no cf / cf_out")
            return self._apply_cols(x, y, gradients, masked, remap_area_min, out_dtype, _flags(flags, skipna=skipna), stream,
                                    scratch_rows, scratch)
        if x.layout == "sb":
            return self.apply_sb(x, y=y, masked=masked, remap_area_min=remap_area_min, out_dtype=out_dtype,
                                 flags=flags, skipna=skipna, stream=stream, keep_batch_fastest=keep_batch_fastest,
                                 cf=cf, cf_out=cf_out)
        if keep_batch_fastest:
            raise ValueError("keep_batch_fastest needs a batch-fastest field (DeviceArray(..., layout='sb'))")
        if x.ndim != 2 or x.shape[1] < self.n_src:
            raise ValueError(f"X must be (B, >= {self.n_src}), got {x.shape}")
        n_batch = x.shape[0]
        y_res = result_dtype(out_dtype, cf_out)
        y = _device_result(y, (n_batch, self.n_dst), y_res[0])
        fl = _flags(flags, masked, skipna)
        return _apply_call("smm_apply", self.handle, x, (x.shape[1],), y,
                           (self.n_dst, n_batch, float(remap_area_min), fl, _stream_handle(stream)), y_res, cf, cf_out)

    def used_sources(self):
        """Ascending 0-based indices of the source cells that carry a link (length n_used_src):
        the row order of a packed batch-fastest field (apply_sb(..., packed=True))."""
        used = np.empty(self.n_used_src, dtype=np.int32)
        _lib.call("smm_operator_used_sources", self.handle, _cptr(used))
        return used

    def prepare_sb(self):
        """Upload the canonical CSR the batch-fastest kernel reads (else done by the first apply_sb)."""
        _lib.call("smm_operator_prepare_sb", self.handle)
        return self

    def apply_sb(self, x, y=None, masked=False, remap_area_min=0.0, packed=False, out_dtype=np.float64,
                 flags=0, stream=None, keep_batch_fastest=False, n_batch=None, skipna=False, cf=None, cf_out=None):
        """The same product for a device-resident field kept batch-fastest: x of shape (S, B) -- or
        (n_used_src, B) with packed=True, rows in `used_sources()` order -- holds the B batch values
        of each source cell contiguously.  Y is (B, D) as `apply` returns it, bit-identical to
        ``apply`` on the transposed field; HBM traffic equals the algorithmic bytes because every
        needed source cell is one contiguous run (smm_apply_sb).  keep_batch_fastest: the result
        stays batch-fastest as well -- Y (D, B), tagged layout "sb" -- which is what a following regrid
        on the target grid consumes without any transpose (SMM_APPLY_SB_Y_SB).  n_batch: batch entries
        when the last axis of x is a padded pitch (cells that start on 128-B lines -- a pitch of a multiple
        of 16 doubles -- are what the cell-staging kernel likes: every 16-entry run is then one line).
        cf: a `CFDecode` for a raw int16 / uint16 field (see `apply`).  cf_out: a `CFEncode` -- the result is raw
        int16 / uint16 (see `apply`); kept batch-fastest it is what a following `apply_sb(..., cf=)` consumes."""
        if not isinstance(x, DeviceArray):
            raise TypeError("SparseOperator.apply_sb takes a DeviceArray")
        rows = self.n_used_src if packed else self.n_src
        if x.ndim != 2 or x.shape[0] != rows:
            raise ValueError(f"X must be ({rows}, B), got {x.shape}")
        ldx = x.shape[1]
        n_batch = ldx if n_batch is None else int(n_batch)
        if not 0 <= n_batch <= ldx:
            raise ValueError(f"n_batch must be within the pitch {ldx}")
        y_shape = (self.n_dst, n_batch) if keep_batch_fastest else (n_batch, self.n_dst)
        y_res = result_dtype(out_dtype, cf_out)
        y = _device_result(y, y_shape, y_res[0], "sb" if keep_batch_fastest else "bs")
        fl = _flags(flags, masked, skipna, sb_packed=packed, y_sb=keep_batch_fastest)
        return _apply_call("smm_apply_sb", self.handle, x, (max(ldx, 1),), y,
                           (max(y_shape[1], 1), n_batch, float(remap_area_min), fl, _stream_handle(stream)), y_res, cf,
                           cf_out)

    def apply_host(self, x, out=None, masked=False, remap_area_min=0.0, out_dtype=np.float64,
                   flags=0, chunk_rows=0, skipna=False, cf=None, cf_out=None, half=False, gradients=None):
        """Same product for a host (numpy) array of shape (B, S): the rows stream through the
        library's double-buffered H2D / kernel / D2H pipeline (smm_apply_host).  Arrays from
        `pinned_empty` are DMA'd without staging copies.  Returns a (B, D) numpy array.
        cf: a `CFDecode` -- x is the raw int16 / uint16 of a CF-packed field: it is staged, packed and shipped as
        2-byte elements and decoded inside the kernels (smm_apply_host_cf).
        cf_out: a `CFEncode` -- the result is encoded inside the kernels and comes back, is staged and copied out as
        raw int16 / uint16: a quarter of the float64 result's bytes over PCIe (smm_apply_host_pk).
        half: a float16 field is shipped as 2-byte cells and widened to float32 inside the kernels (by default it is
        promoted to float64 on the host, as before); a `bfloat16` field always is.  out_dtype float16 / `bfloat16`: the
        result comes back as 2-byte cells.
        gradients: a `GradientRule` -- as for `apply`, for a host field.  This is the first form of that road: a
        synchronous loop over chunks of rows -- H2D copy of the chunk, smm_apply_cols, D2H copy -- which overlaps
        nothing.  A chunk's X, planes and Y stay within 256 MiB and a quarter of the free device memory; chunk_rows > 0
        fixes the rows per chunk."""
        if gradients is not None:
            return self._apply_host_cols(x, out, gradients, masked, remap_area_min, out_dtype, _flags(flags, skipna=skipna),
                                         int(chunk_rows), cf, cf_out, half)
        x = _host_field(x, cf, half)
        if x.ndim != 2 or x.shape[1] != self.n_src:
            raise ValueError(f"X must be (B, {self.n_src}), got {x.shape}")
        if x.strides[1] != x.itemsize or x.strides[0] % x.itemsize or x.strides[0] < self.n_src * x.itemsize:
            x = np.ascontiguousarray(x)
        n_batch = x.shape[0]
        y_res = result_dtype(out_dtype, cf_out)
        if out is None:
            out = result_cache.empty((n_batch, self.n_dst), y_res[0])      # page-locked and recycled when large
        if out.shape != (n_batch, self.n_dst) or not out.flags.c_contiguous:
            raise ValueError(f"out must be a C-contiguous ({n_batch}, {self.n_dst}) array")
        fl = _flags(flags, masked, skipna)
        ldx = x.strides[0] // x.itemsize if n_batch > 1 else max(self.n_src, 1)
        return _apply_call("smm_apply_host", self.handle, x, (ldx,), out,
                           (self.n_dst, n_batch, float(remap_area_min), fl, int(chunk_rows)), y_res, cf, cf_out, "out")

    def _apply_host_cols(self, x, out, rule, masked, remap_area_min, out_dtype, flags, chunk_rows, cf, cf_out, half):
        """`apply_host(..., gradients=rule)`: the synchronous chunk loop."""
        if cf is not None or cf_out is not None or half:
            raise ValueError("gradients= goes with float32 / float64 fields and float64 results: no cf / cf_out / half")
        if np.dtype(out_dtype) != np.dtype(np.float64):
            raise ValueError("gradients= produces float64 results")
        self._check_rule(rule)
        x = _host_field(x, None, False)
        if x.dtype not in (np.float32, np.float64):      # `bfloat16`, which the other host entries ship as it is
            x = x.astype(np.float64)
        if x.ndim != 2 or x.shape[1] != self.n_src:
            raise ValueError(f"X must be (B, {self.n_src}), got {x.shape}")
        x = np.ascontiguousarray(x)
        n_batch = x.shape[0]
        if out is None:
            out = result_cache.empty((n_batch, self.n_dst), np.float64)
        if out.shape != (n_batch, self.n_dst) or not out.flags.c_contiguous or out.dtype != np.float64:
            raise ValueError(f"out must be a C-contiguous float64 ({n_batch}, {self.n_dst}) array")
        if n_batch == 0:
            return out
        if chunk_rows <= 0:      # X, planes and Y of a chunk: 256 MiB and a quarter of the free memory, as _grib.host_chunks
            from .device import mem_info
            per_row = self.n_src * x.itemsize + rule.n_planes * self.n_src * 8 + self.n_dst * 8
            budget = min(256 << 20, mem_info()[0] // 4)
            chunk_rows = max(1, budget // max(per_row, 1))
        chunk_rows = min(int(chunk_rows), n_batch)
        dx = DeviceArray((chunk_rows, self.n_src), x.dtype)
        dy = DeviceArray((chunk_rows, self.n_dst), np.float64)
        scratch = DeviceArray((chunk_rows * rule.n_planes * self.n_src * 8,), np.uint8)
        for r0 in range(0, n_batch, chunk_rows):
            r1 = min(n_batch, r0 + chunk_rows)
            xc, yc = dx.rows(0, r1 - r0), dy.rows(0, r1 - r0)
            xc.copy_from_host(x[r0:r1])
            self._apply_cols(xc, yc, rule, masked, remap_area_min, np.float64, flags, None, None, scratch=scratch)
            yc.to_host(out=out[r0:r1])      # a blocking copy on the default stream: the chunk is done
        return out

    def apply_grib(self, x, rows, x_bytes=None, y=None, masked=False, remap_area_min=0.0, flags=0, stream=None,
                   bitmaps=None, skipna=False, ccsds=None, cpx=None, cpx_missing=None, coded=None):
        """Y = epilogue(fill(decode(X)) . W) for GRIB simple-packed fields resident in HBM as they are on disk
        (smm_apply_grib).  x: a `DeviceArray` of uint8 -- or a raw device pointer with x_bytes -- holding the packed
        bit streams (4-byte aligned; the array -- or the allocation behind a raw pointer -- must cover x_bytes rounded
        up to 4, the kernel reads whole 32-bit words: a shorter DeviceArray is a ValueError); rows: one `GRIB_ROW_DTYPE`
        record per batch row (where its values start in x, its reference value, 2^E, 10^D, its bit width).  The bits
        are unpacked in the kernel's gather; the float64 result is bit-identical to `apply` on the float32 field a
        host decode gives.  Returns a (B, D) DeviceArray.
        bitmaps: one `GRIB_BITMAP_DTYPE` record per row (smm_apply_grib_bm) -- where the row's bitmap lies in x, or
        `GRIB_NO_BITMAP`, and how many values its stream holds.  A cell whose bit is 0 is NaN, as the host decode has
        it; the cell's rank in the stream is looked up in a table built on the device ahead of the gather.
        skipna: renormalise over the valid source values of each row (smm_apply_grib_na) -- the bits of
        `apply(..., skipna=True, flags=APPLY_KERNEL_SELL)` on the decoded float32 field, NaN where the bitmap is 0.
        ccsds: one `GRIB_AEC_DTYPE` record per row -- x holds the CCSDS streams of GRIB-2 template 5.42 (a record with
        block_size 0: that row is simple-packed).  One device step ahead of the gather turns them into simple-packed
        streams (smm_grib_aec_unpack); the result has the bits of the same call on the simple-packed integers.
        cpx: one `GRIB_CPX_DTYPE` record per row -- x holds the complex-packed streams of templates 5.2 / 5.3 (a record
        whose order is GRIB_CPX_SIMPLE: that row is simple-packed).  The same, through smm_grib_cpx_unpack; rows' nbits of
        such a row is not read.  It does not go with ccsds.
        cpx_missing: beside cpx, one uint8 per row -- the row's missing value management (section 5's octet 23): 1 or 2
        means missing values are codes inside the groups.  The device step (smm_grib_cpx_unpack_mv) turns them into a
        bitmap and the present integers, and the gather runs as with bitmaps=: the bits of the same call on the
        simple-packed integers with that bitmap.  Such a row cannot have a bitmap of its own as well.
        coded: what the three keywords say as one `CodedRows` (`GribField.coded`), in their place."""
        rows, rows_p = _grib.grib_rows(rows)
        coded = _grib.CodedRows.of(rows.size, ccsds, cpx, cpx_missing, coded=coded)
        if coded is not None:      # what is refused about the records comes before the device is looked at
            if bitmaps is not None:
                bitmaps, _ = _grib.grib_bitmaps(bitmaps, rows.size)
            idx, total = coded.streams(rows, bitmaps)
        x_ptr, n_bytes = _grib.packed_bytes(x, x_bytes, "apply_grib", raw=coded is None)
        if coded is not None:
            # bitmaps and simple-packed rows stay where they are in x: then x travels along in front of the new streams
            plain = rows["nbits"] != 0
            plain[idx] = False
            keep = bitmaps is not None or bool(plain.any())
            base = _grib.align4(n_bytes) if keep else 0
            both = DeviceArray((max(base + total, 4),), np.uint8)
            if keep and base:
                _lib.call("smm_memcpy_d2d", ctypes.c_void_p(both.ptr), x_ptr, base, _stream_handle(stream))
            dst = DeviceArray((total,), np.uint8, ptr=both.ptr + base, base=both)
            rows, bitmaps = _grib.unpack(coded, x, n_bytes, dst, base, rows, idx, stream, bitmaps, self.n_src)
            return self.apply_grib(both, rows, x_bytes=base + total, y=y, masked=masked, remap_area_min=remap_area_min,
                                   flags=flags, stream=stream, bitmaps=bitmaps, skipna=skipna)
        n_batch = rows.size
        y = _grib.float64_result(y, (n_batch, self.n_dst), DeviceArray, "Y")
        _grib.call_grib("smm_apply_grib", self.handle, x_ptr, n_bytes, rows_p, bitmaps, n_batch, skipna, _ptr(y), _lib.SMM_F64,
                        self.n_dst, n_batch, float(remap_area_min), _flags(flags, masked), _stream_handle(stream))
        return y

    def _apply_host_grib_coded(self, buf, rows, out, bitmaps, coded, chunk_rows, **apply_kw):
        """`apply_host_grib(ccsds=)` and `apply_host_grib(cpx=)`: a synchronous loop over chunks of consecutive rows
        (`_grib.host_chunks`), each chunk's Y copied back."""
        out = _grib.float64_result(out, (rows.size, self.n_dst), result_cache.empty, "out")
        for r0, r1, y, _ in _grib.host_chunks(self, buf, rows, bitmaps, coded, chunk_rows, **apply_kw):
            y.to_host(out=out[r0:r1])
        return out

    def _apply_host_grib_out_coded(self, buf, rows, grib_out, bitmaps, coded, chunk_rows, **apply_kw):
        """`apply_host_grib(grib_out=GribEncode(..., ccsds=...))` and `(..., cpx=...)`, by the codec of grib_out: the
        chunks of `_grib.host_chunks`, each chunk's float64 Y packed on the device (smm_grib_pack) and its
        integers coded as CCSDS or complex-packed streams (smm_grib_aec_pack, smm_grib_cpx_pack); one D2H copy of the
        chunk's bitmaps (none when no cell is missing: they are all ones) and one of the bytes its streams use.  Y and
        the simple-packed streams never leave the device.  The chunk budget counts the simple-packed slots and the
        streams' bound, not the bytes used; a width marked `GribEncode.SOURCE_WIDTH` counts as 32 bits there and becomes,
        chunk by chunk, the width smm_grib_cpx_unpack reports for the source row.  The result's buffer is laid out as
        `GribEncode.encode` lays it out: every field's bitmap slot, then the streams back to back."""
        from .griblite import GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribField
        n_batch, D, codec = rows.size, self.n_dst, grib_out.codec
        worst = grib_out.rows_of(0, n_batch, n_batch)
        if worst.has_source_width:
            if coded is None or coded.codec is not _grib.CPX:
                worst._per_field(n_batch)      # the ValueError of an unresolved mark
            worst = worst.resolved(np.full(n_batch, 32, dtype=np.int32))
        offs, total = worst.layout(D, n_batch)
        slot = np.diff(np.append(offs, np.uint64(total))).astype(np.int64)
        bound = worst.coded_bounds(D, n_batch)
        bm_bytes = (D + 7) // 8 + (-((D + 7) // 8)) % 4
        result = np.empty(n_batch * bm_bytes + int(bound.sum()), dtype=np.uint8)      # cut to the bytes used at the end
        head = result[:n_batch * bm_bytes]
        head[:] = 0
        full = np.packbits(np.ones(D, dtype=np.uint8))
        rows_out = np.zeros(n_batch, dtype=GRIB_ROW_DTYPE)
        bitmaps_out = np.zeros(n_batch, dtype=GRIB_BITMAP_DTYPE)
        recs_out = np.zeros(n_batch, dtype=codec.dtype)
        at = n_batch * bm_bytes
        # per row beside Y: its simple-packed slot, the bound of its stream, the coder's scratch
        extra = slot + bound + codec.out_scratch(D)
        for r0, r1, y, rows_in in _grib.host_chunks(self, buf, rows, bitmaps, coded, chunk_rows, extra_cost=extra, **apply_kw):
            enc = grib_out.rows_of(r0, r1, n_batch)
            if enc.has_source_width:
                enc = enc.resolved(rows_in["nbits"])
            packed, rows_c, bm_c = grib_pack(y, enc)
            slot_c = np.diff(np.append(*enc.layout(D, r1 - r0))).astype(np.int64)
            want = _grib.CodedRows(codec, enc.coded_records(r1 - r0, bm_c["n_values"], rows_c["nbits"]))
            streams, rows_c, recs_c = _grib.pack_device("apply_host_grib", packed, rows_c, coded=want)
            missing = np.flatnonzero(bm_c["bitmap_off"] != GRIB_NO_BITMAP)
            h = head[r0 * bm_bytes:r1 * bm_bytes].reshape(r1 - r0, bm_bytes)
            h[:, :full.size] = full
            if missing.size and (slot_c == slot_c[0]).all():      # one strided copy of the chunk's bitmap slots
                _lib.call("smm_memcpy2d_d2h", _cptr(h), bm_bytes, ctypes.c_void_p(packed.ptr), int(slot_c[0]), bm_bytes,
                          r1 - r0, None)
                _lib.call("smm_stream_sync", None)
            else:
                for i in missing:                                     # slots of different sizes: row by row
                    DeviceArray((bm_bytes,), np.uint8, ptr=packed.ptr + int(bm_c["bitmap_off"][i]), base=packed).to_host(out=h[i])
            bm_c["bitmap_off"][missing] = (r0 + missing) * bm_bytes
            if streams.nbytes:
                streams.to_host(out=result[at:at + streams.nbytes])
            rows_c["byte_off"] += np.uint64(at)
            recs_c["byte_off"] += np.uint64(at)
            rows_out[r0:r1], bitmaps_out[r0:r1], recs_out[r0:r1] = rows_c, bm_c, recs_c
            at += streams.nbytes
        return GribField(result[:at], rows_out, (n_batch, D), D, bitmaps=bitmaps_out, **{codec.name: recs_out})

    def apply_host_grib(self, buf, rows, out=None, masked=False, remap_area_min=0.0, flags=0, chunk_rows=0, bitmaps=None,
                        skipna=False, grib_out=None, ccsds=None, cpx=None, cpx_missing=None, coded=None):
        """The host twin (smm_apply_host_grib): buf is a host uint8 array -- typically a whole GRIB file -- and rows as
        for `apply_grib`.  Each row's packed bytes are staged and cross PCIe as they are (2 B per cell at 16 bits), no
        host decode runs.  Returns a float64 (B, D) numpy array, the bits of `apply_host` on the decoded float32 field.
        bitmaps as for `apply_grib` (smm_apply_host_grib_bm): a bitmapped row's bitmap bytes are staged behind its data.
        skipna as for `apply_grib` (smm_apply_host_grib_na): the bits of `apply_host(..., skipna=True)`'s SELL kernel.
        grib_out: a `GribEncode` -- the result comes back GRIB simple-packed (smm_apply_host_grib_pk): a `GribField` of
        shape (B, D) with `bitmaps` set, over `out` (a 1-d uint8 array of at least `grib_out.layout(D, B)` bytes) or a
        fresh buffer; its bytes and records are those of `grib_out.encode` on the float64 result of the same call
        without grib_out.  The float64 result never leaves the device.
        ccsds as for `apply_grib`: the rows' CCSDS streams cross PCIe as they are and are decoded on the device, chunk
        by chunk (a synchronous loop: no copy overlaps a kernel).  It does not go with a simple-packed grib_out.
        grib_out a `GribEncode` with `ccsds` set: the result comes back CCSDS-packed -- a `GribField` with `bitmaps` and
        `ccsds` set, in a buffer of its own, bytewise `grib_out.encode` of the float64 result.  The same synchronous chunk
        loop, with smm_grib_pack and smm_grib_aec_pack behind the gather; the input may be simple-packed or, through
        ccsds=, CCSDS-packed itself.
        cpx as for `apply_grib`: the rows' complex-packed streams cross PCIe as they are and are decoded on the device, in
        the same synchronous chunk loop.  It goes neither with ccsds nor with a simple-packed or CCSDS grib_out.
        grib_out a `GribEncode` with `cpx` set: the result comes back complex-packed (templates 5.2 / 5.3) -- a `GribField`
        with `bitmaps` and `cpx` set, in a buffer of its own, bytewise `grib_out.encode` of the float64 result; its rows
        carry the widths the integers were packed at.  The same synchronous chunk loop, with smm_grib_pack and
        smm_grib_cpx_pack behind the gather; the input may be simple-packed or, through cpx=, complex-packed itself (not
        CCSDS-packed).  Only there a width of `GribEncode.SOURCE_WIDTH` is legal: it becomes, chunk by chunk, the width
        the source row's integers decode to.
        cpx_missing as for `apply_grib`, carried chunk by chunk; a result record never carries it: missing cells of the
        result are bitmapped as ever.  coded as for `apply_grib`."""
        rows, rows_p = _grib.grib_rows(rows)
        buf = np.ascontiguousarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1:
            raise TypeError("apply_host_grib takes the packed bytes as a 1-d uint8 array")
        coded = _grib.CodedRows.of(rows.size, ccsds, cpx, cpx_missing, coded=coded)
        codec_out = None if grib_out is None else grib_out.codec
        if grib_out is not None and coded is not None and (codec_out is None or coded.codec.name not in codec_out.takes):
            raise ValueError(f"{coded.codec.name} does not go with grib_out: decode the field on the host first")
        if codec_out is not None and out is not None:
            raise ValueError(f"a {codec_out.result} result comes in a buffer of its own: its size is known only afterwards")
        n_batch = rows.size
        if coded is not None or codec_out is not None:      # rows decoded or coded on the device: the chunk loop
            apply_kw = dict(masked=masked, remap_area_min=remap_area_min, flags=int(flags), skipna=skipna)
            if codec_out is not None:
                return self._apply_host_grib_out_coded(buf, rows, grib_out, bitmaps, coded, int(chunk_rows), **apply_kw)
            return self._apply_host_grib_coded(buf, rows, out, bitmaps, coded, int(chunk_rows), **apply_kw)
        if grib_out is not None:
            bitmaps, bm_p = (None, None) if bitmaps is None else _grib.grib_bitmaps(bitmaps, n_batch)
            return _grib.host_grib_out("smm_apply_host_grib_pk", self.handle, buf, rows_p, bm_p, grib_out, out,
                                       (n_batch, self.n_dst), n_batch, float(remap_area_min),
                                       _flags(flags, masked, skipna), int(chunk_rows))
        out = _grib.float64_result(out, (n_batch, self.n_dst), result_cache.empty, "out")
        _grib.call_grib("smm_apply_host_grib", self.handle, _cptr(buf), buf.size, rows_p, bitmaps, n_batch, skipna, _cptr(out),
                        _lib.SMM_F64, self.n_dst, n_batch, float(remap_area_min), _flags(flags, masked), int(chunk_rows))
        return out

    def __repr__(self):
        return (f"SparseOperator(S={self.n_src}, D={self.n_dst}, nnz={self.nnz}, "
                f"device={self.device})")


class OperatorGroup(_Handle):
    """Ordered per-level operators applied in one launch (regrid.py:387-418)."""
    _destroy = "smm_group_destroy"

    def __init__(self, operators):
        self.operators = list(operators)
        if not self.operators:
            raise ValueError("OperatorGroup needs at least one operator")
        arr = (ctypes.c_void_p * len(self.operators))(*[op.handle for op in self.operators])
        h = ctypes.c_void_p()
        _lib.call("smm_group_create", arr, len(self.operators), ctypes.byref(h))
        self.handle = h
        self.n_src = self.operators[0].n_src
        self.n_dst = self.operators[0].n_dst

    def __len__(self):
        return len(self.operators)

    def plan_info(self):
        kind, spb = ctypes.c_int(0), ctypes.c_int(0)
        _lib.call("smm_group_plan_info", self.handle, ctypes.byref(kind), ctypes.byref(spb))
        return {"tile_plan": bool(kind.value & 1), "tile_preferred": bool(kind.value & 2),
                "slices_per_block": spb.value}

    def __getitem__(self, i):
        return self.operators[i]

    def _level_args(self, level_index, masked_levels, n_lev=None):
        lev = np.ascontiguousarray(level_index, dtype=np.int32).ravel()
        if n_lev is not None and lev.size != n_lev:
            raise ValueError("level_index must have one entry per data level")
        ml = None
        if masked_levels is not None:
            ml = np.ascontiguousarray(masked_levels, dtype=np.uint8).ravel()
            if ml.size != len(self.operators):
                raise ValueError("masked_levels must have one entry per group member")
        return lev, ml

    def prepare(self, level_index, masked_levels=None):
        """Upload one (level_index, masked_levels) configuration ahead of time: later `apply`
        calls with it allocate nothing and never block (smm_group_prepare)."""
        lev, ml = self._level_args(level_index, masked_levels)
        _lib.call("smm_group_prepare", self.handle, lev.size, _cptr(lev), _cptr(ml))
        return self

    def launch_info(self, n_outer, n_lev, n_inner=1, dtype=np.float64, flags=0):
        """Launch geometry `apply` would use (nothing is launched).  dtype int16 / uint16: a CF-packed field given
        with `cf=` (always the SELL kernel)."""
        code = field_dtype_code(dtype, cf=True) if is_packed_dtype(dtype) else dtype_code(np.dtype(dtype))
        return _launch_info("smm_group_launch_info", self.handle, code,
                            (int(n_outer), int(n_lev), int(n_inner)), flags)

    def apply(self, x, level_index, masked_levels=None, y=None, masked=False, remap_area_min=0.0,
              transpose=True, out_dtype=np.float64, flags=0, stream=None, skipna=False, cf=None, cf_out=None):
        """x: DeviceArray (n_outer, n_lev, n_inner, S) -- or (..., ldx) with a padded row pitch ldx >= S.  Returns
        (n_outer, n_inner, n_lev, D) when transpose (regrid.py:420-427) else
        (n_lev, n_outer, n_inner, D) (the concat order, regrid.py:410).
        cf: a `CFDecode` -- x holds the raw int16 / uint16 of a CF-packed field, decoded inside the kernel with one
        rule for every level (smm_group_apply_cf; bit-identical to applying `cf.decode` first; float64 results only).
        cf_out: a `CFEncode` -- the result is stored as raw int16 / uint16, encoded inside the kernel's stores with one
        rule for every level (smm_group_apply_pk; bit-identical to `cf_out.encode` of the float64 result)."""
        if not isinstance(x, DeviceArray) or x.ndim != 4 or x.shape[3] < self.n_src:
            raise ValueError(f"X must be a DeviceArray (n_outer, n_lev, n_inner, >= {self.n_src})")
        # the last axis may be a padded row pitch (>= S): rows that start on 128-B lines (a multiple
        # of 16 doubles / 32 floats) are staged without straddling lines
        n_outer, n_lev, n_inner, S = x.shape
        lev, ml = self._level_args(level_index, masked_levels, n_lev)
        shape, ys = _level_result(n_outer, n_lev, n_inner, self.n_dst, transpose)
        y_res = result_dtype(out_dtype, cf_out)
        y = _device_result(y, shape, y_res[0])
        xs = (n_lev * n_inner * S, n_inner * S, S)
        fl = _flags(flags, masked, skipna)
        return _apply_call("smm_group_apply", self.handle, x, xs, y,
                           (*ys, n_outer, n_lev, n_inner, _cptr(lev), _cptr(ml), float(remap_area_min), fl,
                            _stream_handle(stream)), y_res, cf, cf_out)

    def apply_sb(self, x, level_index, masked_levels=None, y=None, masked=False, remap_area_min=0.0,
                 transpose=True, out_dtype=np.float64, flags=0, stream=None, keep_batch_fastest=False, n_batch=None,
                 skipna=False, cf=None, cf_out=None):
        """Masked levels for a field kept batch-fastest per level: x is a DeviceArray (n_lev, S, B) --
        per data level the B batch values of each source cell contiguous.  Returns (B, n_lev, D) when
        transpose (regrid.py:420-427) else (n_lev, B, D); bit-identical to `apply` on the transposed field.
        keep_batch_fastest: the result stays batch-fastest per level, (n_lev, D, B) tagged "sb".
        All data levels run in one grouped launch (several for more than 88 levels), ordered on `stream`.
        n_batch: batch entries when the last axis of x is a padded pitch (see SparseOperator.apply_sb).
        cf: a `CFDecode` for a raw int16 / uint16 field (see `apply`; smm_group_apply_sb_cf).
        cf_out: a `CFEncode` -- the result is raw int16 / uint16 (see `apply`; smm_group_apply_sb_pk); kept
        batch-fastest it is what a following `apply_sb(..., cf=)` consumes."""
        if not isinstance(x, DeviceArray) or x.ndim != 3 or x.shape[1] != self.n_src:
            raise ValueError(f"X must be a DeviceArray (n_lev, {self.n_src}, B)")
        n_lev, S, ldx = x.shape
        B = ldx if n_batch is None else int(n_batch)
        if not 0 <= B <= ldx:
            raise ValueError(f"n_batch must be within the pitch {ldx}")
        D = self.n_dst
        lev, ml = self._level_args(level_index, masked_levels, n_lev)
        if keep_batch_fastest:
            shape, ys_lev, ys_b = (n_lev, D, B), D * max(B, 1), max(B, 1)
        else:
            shape = (B, n_lev, D) if transpose else (n_lev, B, D)
            ys_lev, ys_b = (D, n_lev * D) if transpose else (B * D, D)
        y_res = result_dtype(out_dtype, cf_out)
        y = _device_result(y, shape, y_res[0], "sb" if keep_batch_fastest else "bs")
        fl = _flags(flags, masked, skipna, y_sb=keep_batch_fastest)
        return _apply_call("smm_group_apply_sb", self.handle, x, (S * max(ldx, 1), max(ldx, 1)), y,
                           (ys_lev, ys_b, B, n_lev, _cptr(lev), _cptr(ml), float(remap_area_min), fl,
                            _stream_handle(stream)), y_res, cf, cf_out)

    def apply_host(self, x, level_index, masked_levels=None, masked=False, remap_area_min=0.0,
                   transpose=True, out_dtype=np.float64, flags=0, chunk_outer=0, skipna=False, cf=None, cf_out=None,
                   half=False):
        """Host (numpy) variant: x of shape (n_outer, n_lev, n_inner, S); chunks of the outer
        axis stream through the group's H2D / kernel / D2H pipeline (smm_group_apply_host).
        cf: a `CFDecode` -- x is the raw int16 / uint16 of a CF-packed field: it is staged, packed and shipped as
        2-byte elements and decoded inside the kernels (smm_group_apply_host_cf).
        cf_out: a `CFEncode` -- the result is encoded inside the kernels and comes back, is staged and copied out as
        raw int16 / uint16: a quarter of the float64 result's bytes over PCIe (smm_group_apply_host_pk).
        half: a float16 field is shipped as 2-byte cells (see SparseOperator.apply_host); `bfloat16` always is."""
        x = np.ascontiguousarray(_host_field(x, cf, half))
        if x.ndim != 4 or x.shape[3] != self.n_src:
            raise ValueError(f"X must be (n_outer, n_lev, n_inner, {self.n_src}), got {x.shape}")
        n_outer, n_lev, n_inner, _ = x.shape
        lev, ml = self._level_args(level_index, masked_levels, n_lev)
        shape, _ = _level_result(n_outer, n_lev, n_inner, self.n_dst, transpose)
        y_res = result_dtype(out_dtype, cf_out)
        out = result_cache.empty(shape, y_res[0])
        fl = _flags(flags, masked, skipna)
        return _apply_call("smm_group_apply_host", self.handle, x, (), out,
                           (n_outer, n_lev, n_inner, int(bool(transpose)), _cptr(lev), _cptr(ml), float(remap_area_min),
                            fl, int(chunk_outer)), y_res, cf, cf_out, "out")

    def _grib_args(self, rows, bitmaps, level_index, masked_levels, n_inner):
        """rows / bitmaps flat -- then n_lev is len(level_index) and n_inner the keyword -- or shaped
        (n_outer, n_lev, n_inner).  Returns (n_outer, n_lev, n_inner), the two record arrays with their pointers and
        the level arguments."""
        from .griblite import GRIB_ROW_DTYPE
        shaped = np.asarray(rows, dtype=GRIB_ROW_DTYPE)
        if shaped.ndim == 3:
            dims = shaped.shape
        elif shaped.ndim == 1:
            n_lev, n_inner = np.asarray(level_index).size, int(n_inner)
            if n_lev <= 0 or n_inner <= 0 or shaped.size % (n_lev * n_inner):
                raise ValueError(f"{shaped.size} rows are no whole number of (n_lev = {n_lev}) x (n_inner = {n_inner}) blocks")
            dims = (shaped.size // (n_lev * n_inner), n_lev, n_inner)
        else:
            raise ValueError(f"rows must be flat or (n_outer, n_lev, n_inner), got {shaped.shape}")
        lev, ml = self._level_args(level_index, masked_levels, dims[1])
        rows, rows_p = _grib.grib_rows(shaped)
        bm, bm_p = None, None
        if bitmaps is not None:
            if np.ndim(bitmaps) not in (1, 3) or (np.ndim(bitmaps) == 3 and np.shape(bitmaps) != dims):
                raise ValueError(f"bitmaps must be flat or {dims}, got {np.shape(bitmaps)}")
            bm, bm_p = _grib.grib_bitmaps(bitmaps, rows.size)
        return dims, (rows, rows_p), (bm, bm_p), (lev, ml)

    def apply_grib(self, x, rows, level_index, masked_levels=None, bitmaps=None, y=None, x_bytes=None, masked=False,
                   remap_area_min=0.0, transpose=True, flags=0, stream=None, n_inner=1, skipna=False):
        """`apply` for GRIB simple-packed fields resident in HBM as they are on disk (smm_group_apply_grib): x and the
        `GRIB_ROW_DTYPE` / `GRIB_BITMAP_DTYPE` records as for `SparseOperator.apply_grib`, one record per batch row
        (o, l, i) in C order -- rows shaped (n_outer, n_lev, n_inner), or flat with n_lev = len(level_index) and
        `n_inner`.  All levels run in one launch of the grouped GRIB gather.  Returns the float64 DeviceArray `apply`
        returns, (n_outer, n_inner, n_lev, D) when transpose else (n_lev, n_outer, n_inner, D), bit-identical to
        `apply` on the float32 field a host decode gives (NaN where a bitmap bit is 0).
        skipna: every level renormalises over its valid source values (smm_group_apply_grib_na) -- the bits of
        `apply(..., skipna=True, flags=APPLY_KERNEL_SELL)` on that field."""
        (n_outer, n_lev, n_in), (rows, rows_p), (bm, bm_p), (lev, ml) = self._grib_args(rows, bitmaps, level_index,
                                                                                         masked_levels, n_inner)
        x_ptr, n_bytes = _grib.packed_bytes(x, x_bytes, "apply_grib", raw=True)
        shape, ys = _level_result(n_outer, n_lev, n_in, self.n_dst, transpose)
        y = _grib.float64_result(y, shape, DeviceArray, "Y")
        fl = _flags(flags, masked)
        _lib.call("smm_group_apply_grib_na" if skipna else "smm_group_apply_grib", self.handle, x_ptr, n_bytes, rows_p, bm_p, _ptr(y), _lib.SMM_F64, *ys, n_outer,
                  n_lev, n_in, _cptr(lev), _cptr(ml), float(remap_area_min), fl, _stream_handle(stream))
        return y

    def apply_host_grib(self, buf, rows, level_index, masked_levels=None, bitmaps=None, out=None, masked=False,
                        remap_area_min=0.0, transpose=True, flags=0, chunk_outer=0, n_inner=1, skipna=False,
                        grib_out=None):
        """The host twin (smm_group_apply_host_grib): buf is a host uint8 array -- typically a whole GRIB file -- rows
        and bitmaps as for `apply_grib`.  Blocks of the outer axis stream through the group's pipeline; each row's
        packed bytes (a bitmapped row's: its present cells only, and its bitmap) cross PCIe as they are and no host
        decode runs.  Returns the float64 array `apply_host` returns on the decoded float32 field, bit for bit.
        skipna as for `apply_grib` (smm_group_apply_host_grib_na).
        grib_out: a `GribEncode` -- the result comes back GRIB simple-packed (smm_group_apply_host_grib_pk): a
        `GribField` of shape (n_outer, n_lev, n_inner, D) with `bitmaps` set -- one record per batch row in the order
        of `rows` -- over `out` (a 1-d uint8 array of at least `grib_out.layout(D, n_rows)[1]` bytes, pageable or from
        `pinned_empty`) or a fresh buffer; its bytes and records are those of `grib_out.encode` on the float64 result
        of the same call without grib_out, taken in that order.  No float64 array is delivered, so transpose=False is
        a ValueError."""
        (n_outer, n_lev, n_in), (rows, rows_p), (bm, bm_p), (lev, ml) = self._grib_args(rows, bitmaps, level_index,
                                                                                         masked_levels, n_inner)
        buf = np.ascontiguousarray(buf)
        if buf.dtype != np.uint8 or buf.ndim != 1:
            raise TypeError("apply_host_grib takes the packed bytes as a 1-d uint8 array")
        if grib_out is not None:
            if not transpose:
                raise ValueError("grib_out returns the rows in record order (n_outer, n_lev, n_inner): "
                                 "transpose=False does not go with it")
            return _grib.host_grib_out("smm_group_apply_host_grib_pk", self.handle, buf, rows_p, bm_p, grib_out, out,
                                       (n_outer, n_lev, n_in, self.n_dst), n_outer, n_lev, n_in, _cptr(lev), _cptr(ml),
                                       float(remap_area_min), _flags(flags, masked, skipna), int(chunk_outer))
        shape, _ = _level_result(n_outer, n_lev, n_in, self.n_dst, transpose)
        out = _grib.float64_result(out, shape, result_cache.empty, "out")
        fl = _flags(flags, masked)
        _lib.call("smm_group_apply_host_grib_na" if skipna else "smm_group_apply_host_grib", self.handle, _cptr(buf), buf.size, rows_p, bm_p, _cptr(out), _lib.SMM_F64,
                  n_outer, n_lev, n_in, int(bool(transpose)), _cptr(lev), _cptr(ml), float(remap_area_min), fl,
                  int(chunk_outer))
        return out
