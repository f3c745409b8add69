"""What the GRIB calls of `SparseOperator` / `OperatorGroup` and the device wrappers `grib_unpack` / `grib_unpack_cpx` /
`grib_aec_pack` / `grib_cpx_pack` share: the description of a kind of coded row (`CCSDS`, `CPX`), the check of the packed bytes, the
entry dispatch, the result checks, and the chunk loop of the host calls whose rows are decoded or coded on the device --
its plan (`plan_chunks`, host only) apart from its execution (`host_chunks`)."""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib, device
from .device import DeviceArray, _stream_handle, result_cache
from .griblite import (GRIB_AEC_DTYPE, GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_CPX_SIMPLE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE,
                       GribField)


def align4(v):
    return (v + 3) // 4 * 4


def _cast(records, struct):
    return ctypes.cast(records.ctypes.data, ctypes.POINTER(struct))


# ---------------------------------------------------------------------------------------------- kinds of coded rows
# What differs between the kinds of coded rows a call may hold.  arg: the keyword that carries the records; words: what
# messages call them; is_coded(recs, rows): which rows of a call have a coded stream -- the others are simple-packed;
# device_cost(recs, n_val, nbits): the device bytes a coded row costs in a chunk beside its staged stream; bound_entry,
# pack_entry: the way back, simple-packed streams coded as rows of this kind.
Coded = namedtuple("Coded", "arg words dtype struct layout_entry unpack_entry is_coded device_cost bound_entry pack_entry")

# a record with block_size 0 marks a simple-packed row, a row of width 0 has no stream at all; a coded row costs its
# transcoded stream and 4 B per sample of scratch
CCSDS = Coded("ccsds", "CCSDS records", GRIB_AEC_DTYPE, _lib.GribAecStruct, "smm_grib_aec_layout", "smm_grib_aec_unpack",
              lambda recs, rows: (recs["block_size"] != 0) & (rows["nbits"] != 0),
              lambda recs, n_val, nbits: align4((n_val * nbits + 7) // 8) + 4 * n_val,
              "smm_grib_aec_pack_bound", "smm_grib_aec_pack")
# a record whose order is GRIB_CPX_SIMPLE marks a simple-packed row; a coded row costs its slot of 4 B per value and
# 8 B per value plus 16 B per group of scratch; one with missing values inside its groups (`cpx_missing_cost`) also its
# bitmap slot, 8 B more per value -- the integers pass through a second array on their way to their ranks -- and 4 B per
# 256 values
CPX = Coded("cpx", "complex-packing records", GRIB_CPX_DTYPE, _lib.GribCpxStruct, "smm_grib_cpx_layout",
            "smm_grib_cpx_unpack", lambda recs, rows: recs["order"] != GRIB_CPX_SIMPLE,
            lambda recs, n_val, nbits: 12 * n_val + 16 * recs["n_groups"].astype(np.int64) + 256,
            "smm_grib_cpx_pack_bound", "smm_grib_cpx_pack")


def cpx_missing_cost(n_val):
    """Device bytes a complex-packed row with missing values inside its groups costs beside `CPX.device_cost`."""
    return align4((n_val + 7) // 8) + 8 * n_val + 4 * ((n_val + 255) // 256)


# What differs between the kinds of coded results (`apply_host_grib(grib_out=GribEncode(..., ccsds= / cpx=))`).  attr: the
# attribute of `GribEncode` and `GribField` that carries the parameters / the records; records, bounds: the `GribEncode`
# methods that give the wanted records of a chunk and the streams' bounds; pack: the device step behind `grib_pack`;
# scratch(n_dst): the device bytes a row costs beside its streams' bound; takes: the kinds of coded INPUT it goes with.
CodedOut = namedtuple("CodedOut", "attr words dtype records bounds pack scratch takes")
# 8 B per block and 12 B per segment of scratch
CCSDS_OUT = CodedOut("ccsds", "CCSDS-coded", GRIB_AEC_DTYPE, "ccsds_records", "ccsds_bounds", "grib_aec_pack",
                     lambda n_dst: (n_dst // 8 + 1) * 20, (None, CCSDS))
# 8 B per group of at least 8 values and 12 B per 1024 values of scratch
CPX_OUT = CodedOut("cpx", "complex-packed", GRIB_CPX_DTYPE, "cpx_records", "cpx_bounds", "grib_cpx_pack",
                   lambda n_dst: n_dst + 8 + (n_dst // 1024 + 1) * 12, (None, CPX))


def out_kind(grib_out):
    """The kind of coded result a `GribEncode` asks for, or None: simple-packed (or no grib_out at all)."""
    if grib_out is None:
        return None
    return CPX_OUT if getattr(grib_out, "cpx", None) is not None else \
        CCSDS_OUT if getattr(grib_out, "ccsds", None) is not None else None


def one_kind(ccsds, cpx):
    """(kind, records) of the coded rows of a call -- CCSDS or complex packing, not both -- or (None, None)."""
    if ccsds is not None and cpx is not None:
        raise ValueError("cpx does not go with ccsds: a call's coded rows are of one kind")
    return (CPX, cpx) if cpx is not None else (CCSDS, ccsds) if ccsds is not None else (None, None)


def grib_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=GRIB_ROW_DTYPE).ravel()
    return rows, _cast(rows, _lib.GribRowStruct)


def grib_bitmaps(bitmaps, n_batch):
    bitmaps = np.ascontiguousarray(bitmaps, dtype=GRIB_BITMAP_DTYPE).ravel()
    if bitmaps.size != n_batch:
        raise ValueError(f"{bitmaps.size} bitmap records for {n_batch} rows")
    return bitmaps, _cast(bitmaps, _lib.GribBitmapStruct)


def records(kind, recs, rows):
    """The records of `kind`, one per row."""
    recs = np.ascontiguousarray(recs, dtype=kind.dtype).ravel()
    if recs.size != rows.size:
        raise ValueError(f"{recs.size} {kind.words} for {rows.size} rows")
    return recs


def _layout_total(entry, kind, recs, missing=None):
    """Bytes the host-only layout entry (or the encoder's bound) gives for the records; missing: the complex-packed rows'
    missing value management (smm_grib_cpx_layout_mv), or None."""
    total = ctypes.c_uint64(0)
    if missing is not None:
        _lib.call("smm_grib_cpx_layout_mv", _cast(recs, kind.struct), missing.ctypes.data_as(_lib._u8p), recs.size, None, None,
                  ctypes.byref(total))
    else:
        _lib.call(entry, _cast(recs, kind.struct), recs.size, None, ctypes.byref(total))
    return int(total.value)


def missing_of(missing, rows):
    """One uint8 per row: the complex-packed rows' missing value management, or None."""
    if missing is None:
        return None
    missing = np.ascontiguousarray(missing, dtype=np.uint8).ravel()
    if missing.size != rows.size:
        raise ValueError(f"{missing.size} missing-value-management values for {rows.size} rows")
    return missing


def refuse_bitmap_with_missing(bitmaps, missing, coded):
    """A coded row with a bitmap of its own and missing values inside its groups is not composed on the device."""
    if bitmaps is not None and missing is not None and \
            ((bitmaps["bitmap_off"] != GRIB_NO_BITMAP) & (missing != 0) & coded).any():
        raise ValueError("a row has a bitmap and missing values inside its groups: decode it on the host")


def coded_rows(kind, recs, rows, missing=None):
    """(which rows have a coded stream, bytes of their transcoded streams)."""
    idx = np.flatnonzero(kind.is_coded(recs, rows))
    return idx, _layout_total(kind.layout_entry, kind, np.ascontiguousarray(recs[idx]),
                              None if missing is None else np.ascontiguousarray(missing[idx]))


# ---------------------------------------------------------------------------------------------- packed bytes on the device
def packed_bytes(x, x_bytes, who, raw=False):
    """(pointer, n_bytes) of packed bytes resident in HBM: x a uint8 `DeviceArray` that covers x_bytes (default: all of
    it) rounded up to 4 -- the kernels read whole 32-bit words -- or, with raw, a raw device pointer with x_bytes."""
    if isinstance(x, DeviceArray) and x.dtype == np.uint8:
        n_bytes = x.nbytes if x_bytes is None else int(x_bytes)
        if align4(n_bytes) > x.nbytes:
            raise ValueError(f"the array must cover x_bytes rounded up to 4: {n_bytes} bytes in an array of {x.nbytes}")
        return ctypes.c_void_p(x.ptr), n_bytes
    if isinstance(x, DeviceArray) or not raw:
        raise TypeError(f"{who} takes the packed bytes as a uint8 DeviceArray")
    if x_bytes is None:
        raise TypeError("a raw device pointer needs x_bytes")
    return ctypes.c_void_p(int(x)), int(x_bytes)


def transcode_args(who, kind, bound_entry, device_bytes, rows, recs, x_bytes, out, missing=None):
    """What `unpack_device` and `pack_device` check alike: (pointer, n_bytes) of the bytes, the row
    and `kind` records, `out` -- given or fresh -- holding at least what bound_entry says the records need, and
    `missing` as one uint8 per row (or None)."""
    x_ptr, n_bytes = packed_bytes(device_bytes, x_bytes, who)
    rows, _ = grib_rows(rows)
    recs = records(kind, recs, rows)
    missing = missing_of(missing, rows)
    total = _layout_total(bound_entry, kind, recs, missing)
    if out is None:
        out = DeviceArray((max(total, 4),), np.uint8)
    elif not isinstance(out, DeviceArray) or out.dtype != np.uint8 or out.nbytes < total:
        raise ValueError(f"out must be a uint8 DeviceArray of at least {total} bytes")
    return x_ptr, n_bytes, rows, recs, out, missing


def unpack_device(who, kind, device_bytes, rows, recs, x_bytes=None, out=None, stream=None, missing=None, with_bitmaps=False):
    """`grib_unpack` (CCSDS) and `grib_unpack_cpx` (CPX); with_bitmaps: `grib_unpack_cpx_mv` -- missing: the rows' missing
    value management or None --, which returns the rows' bitmap records as well."""
    x_ptr, n_bytes, rows, recs, out, missing = transcode_args(who, kind, kind.layout_entry, device_bytes, rows, recs, x_bytes, out,
                                                              missing)
    rows_out = np.zeros(rows.size, dtype=GRIB_ROW_DTYPE)
    if with_bitmaps:
        bitmaps_out = np.zeros(rows.size, dtype=GRIB_BITMAP_DTYPE)
        _lib.call("smm_grib_cpx_unpack_mv", device.current_device(), x_ptr, n_bytes, _cast(recs, kind.struct),
                  None if missing is None else missing.ctypes.data_as(_lib._u8p), _cast(rows, _lib.GribRowStruct), rows.size,
                  ctypes.c_void_p(out.ptr), out.nbytes, _cast(rows_out, _lib.GribRowStruct),
                  _cast(bitmaps_out, _lib.GribBitmapStruct), _stream_handle(stream))
        return out, rows_out, bitmaps_out
    _lib.call(kind.unpack_entry, device.current_device(), x_ptr, n_bytes, _cast(recs, kind.struct),
              _cast(rows, _lib.GribRowStruct), rows.size, ctypes.c_void_p(out.ptr), out.nbytes,
              _cast(rows_out, _lib.GribRowStruct), _stream_handle(stream))
    return out, rows_out


def pack_device(who, kind, device_bytes, rows, recs, x_bytes=None, out=None, stream=None):
    """`grib_aec_pack` (CCSDS) and `grib_cpx_pack` (CPX): (out cut to the bytes used, the rows with byte_off at their
    streams, the records of the streams written)."""
    x_ptr, n_bytes, rows, recs, out, _ = transcode_args(who, kind, kind.bound_entry, device_bytes, rows, recs, x_bytes, out)
    recs_out = np.zeros(rows.size, dtype=kind.dtype)
    used = ctypes.c_uint64(0)
    _lib.call(kind.pack_entry, device.current_device(), x_ptr, n_bytes, _cast(rows, _lib.GribRowStruct),
              _cast(recs, kind.struct), rows.size, ctypes.c_void_p(out.ptr), out.nbytes, _cast(recs_out, kind.struct),
              ctypes.byref(used), _stream_handle(stream))
    rows_out = rows.copy()
    rows_out["byte_off"] = recs_out["byte_off"]
    return DeviceArray((int(used.value),), np.uint8, ptr=out.ptr, base=out), rows_out, recs_out


def unpack(kind, src, n_bytes, dst, shift, rows, recs, idx, stream, missing=None, bitmaps=None, n_src=0):
    """The coded streams of rows `idx` in src[:n_bytes] become simple-packed streams in dst.  Returns (the row table with
    those rows pointing at `shift` + their place in dst (complex-packed ones with the width their integers were stored
    at), the others as they were; the bitmap table).  missing: None, or the rows' missing value management (complex
    packing): a row with missing != 0 gets the bitmap the device step wrote behind its slot -- offsets shifted like
    byte_off, a table of GRIB_NO_BITMAP over n_src points made first when the call has none -- and the count of its
    present values."""
    if missing is None or not missing[idx].any():
        _, rows_c = unpack_device("apply_grib", kind, src, rows[idx], recs[idx], x_bytes=n_bytes, out=dst, stream=stream)
    else:
        _, rows_c, bm_c = unpack_device("apply_grib", kind, src, rows[idx], recs[idx], x_bytes=n_bytes, out=dst, stream=stream,
                                        missing=missing[idx], with_bitmaps=True)
        if bitmaps is None:
            bitmaps = np.zeros(rows.size, dtype=GRIB_BITMAP_DTYPE)
            bitmaps["bitmap_off"], bitmaps["n_values"] = GRIB_NO_BITMAP, n_src
        else:
            bitmaps = bitmaps.copy()
        written = np.flatnonzero(bm_c["bitmap_off"] != GRIB_NO_BITMAP)
        bm_c["bitmap_off"][written] += np.uint64(shift)
        bitmaps[idx[written]] = bm_c[written]
    rows = rows.copy()
    rows_c["byte_off"] += np.uint64(shift)
    rows[idx] = rows_c
    return rows, bitmaps


# ---------------------------------------------------------------------------------------------- entries and results
def call_grib(entry, handle, x_ptr, n_bytes, rows_p, bitmaps, n_batch, skipna, *rest):
    """`entry`_na under skipna -- without bitmaps its bitmap pointer is null --, `entry`_bm with bitmaps, else `entry`,
    whose argument list has no bitmap pointer."""
    if not skipna and bitmaps is None:
        return _lib.call(entry, handle, x_ptr, n_bytes, rows_p, *rest)
    bitmaps, bm_p = (None, None) if bitmaps is None else grib_bitmaps(bitmaps, n_batch)
    return _lib.call(entry + ("_na" if skipna else "_bm"), handle, x_ptr, n_bytes, rows_p, bm_p, *rest)


def float64_result(out, shape, empty, name):
    """out -- given, or `empty(shape, float64)` -- as a float64 result of `shape`."""
    if out is None:
        out = empty(shape, np.float64)
    if out.shape != shape or out.dtype != np.float64 or not (isinstance(out, DeviceArray) or out.flags.c_contiguous):
        raise ValueError(f"{name} must be a C-contiguous float64 {shape} array")
    return out


def packed_result(out, total):
    """out -- given or fresh -- as the host buffer of a packed result of `total` bytes."""
    if out is None:
        out = result_cache.empty((max(total, 1),), np.uint8)
    if out.dtype != np.uint8 or out.ndim != 1 or out.size < total or not out.flags.c_contiguous:
        raise ValueError(f"out must be a C-contiguous 1-d uint8 array of at least {total} bytes")
    return out


def host_grib_out(entry, handle, buf, rows_p, bm_p, grib_out, out, shape, *tail):
    """`apply_host_grib(grib_out=)` through `entry` (smm_apply_host_grib_pk, smm_group_apply_host_grib_pk): shape is
    the result's, one row of shape[-1] cells per leading index; tail: the entry's arguments behind the records."""
    n_rows, n_dst = int(np.prod(shape[:-1])), shape[-1]
    _, total = grib_out.layout(n_dst, n_rows)
    out = packed_result(out, total)
    rec = grib_out.records(n_rows)
    rows_out = np.zeros(n_rows, dtype=GRIB_ROW_DTYPE)
    bitmaps_out = np.zeros(n_rows, dtype=GRIB_BITMAP_DTYPE)
    _lib.call(entry, handle, buf.ctypes.data_as(ctypes.c_void_p), buf.size, rows_p, bm_p, _cast(rec, _lib.GribEncodeStruct),
              out.ctypes.data_as(ctypes.c_void_p), out.size, _cast(rows_out, _lib.GribRowStruct),
              _cast(bitmaps_out, _lib.GribBitmapStruct), *tail)
    return GribField(out, rows_out, shape, n_dst, bitmaps=bitmaps_out)


# ---------------------------------------------------------------------------------------------- the chunk loop
# One chunk of consecutive rows [r0, r1): pieces -- (staged offset, offset in the caller's buffer, length) of what is
# staged, every piece at a 4-byte-aligned offset --, the staged bytes, the row / coded / bitmap records with byte_off and
# bitmap_off rewritten to the staged offsets (recs: None without a kind, bitmaps: None without bitmaps), the chunk's
# coded rows and the bytes of their transcoded streams.
Chunk = namedtuple("Chunk", "r0 r1 pieces staged_bytes rows recs bitmaps coded_idx coded_bytes missing",
                   defaults=(None,))


def plan_chunks(buf_size, rows, bitmaps, kind, recs, n_src, n_dst, chunk_rows, target, extra_cost=0, missing=None):
    """The chunks of consecutive rows an `apply_host_grib` call with coded rows (kind, recs) or a CCSDS-packed result
    (kind None: every row is simple-packed) goes through, one after the other (an iterator of `Chunk`); host only.  A row
    costs its staged bytes (coded or simple-packed stream, bitmap), for a coded row kind.device_cost, its float64 Y and
    extra_cost (bytes per row, what the caller puts beside them); a chunk takes rows while their cost stays within
    `target` bytes, and at least one; chunk_rows > 0 fixes the rows.  A bitmap several rows of a chunk share is staged
    once in it (and again in the next chunk).  missing: None, or the complex-packed rows' missing value management: a row
    with missing != 0 costs `cpx_missing_cost` more, and the chunk carries its part of the array."""
    n_batch, S = rows.size, n_src
    coded = np.zeros(n_batch, dtype=bool) if kind is None else kind.is_coded(recs, rows)
    has_bm = np.zeros(n_batch, dtype=bool) if bitmaps is None else bitmaps["bitmap_off"] != GRIB_NO_BITMAP
    n_val = np.full(n_batch, S, dtype=np.int64) if bitmaps is None else \
        np.where(has_bm, bitmaps["n_values"], S).astype(np.int64)
    nbits = rows["nbits"].astype(np.int64)
    in_off, in_len, device_cost = rows["byte_off"].astype(np.uint64), (n_val * nbits + 7) // 8, 0
    if kind is not None:
        if (recs["n_values"][coded].astype(np.int64) != n_val[coded]).any():
            raise ValueError("a coded row's record has n_values different from the points its row holds")
        in_off = np.where(coded, recs["byte_off"], in_off).astype(np.uint64)
        in_len = np.where(coded, recs["byte_len"].astype(np.int64), in_len).astype(np.int64)
        device_cost = np.where(coded, kind.device_cost(recs, n_val, nbits), 0)
        if missing is not None:
            refuse_bitmap_with_missing(bitmaps, missing, coded)
            device_cost = device_cost + np.where(coded & (missing != 0), cpx_missing_cost(n_val), 0)
    bm_len = (S + 7) // 8
    if ((in_off.astype(object) + in_len.astype(object)) > buf_size).any() or \
            (has_bm.any() and (bitmaps["bitmap_off"][has_bm].astype(object) + bm_len > buf_size).any()):
        raise ValueError(f"a row's bytes leave the buffer of {buf_size} bytes")
    cost = align4(in_len) + device_cost + n_dst * 8 + np.where(has_bm, align4(bm_len), 0) + extra_cost
    r0 = 0
    while r0 < n_batch:
        r1, used = r0, 0
        while r1 < n_batch and (r1 - r0 < chunk_rows if chunk_rows > 0 else (r1 == r0 or used + int(cost[r1]) <= target)):
            used += int(cost[r1])
            r1 += 1
        rows_c = rows[r0:r1].copy()
        recs_c = None if kind is None else recs[r0:r1].copy()
        bm_c = None if bitmaps is None else bitmaps[r0:r1].copy()
        pieces, at, seen = [], 0, {}
        for i in range(r0, r1):
            (recs_c if coded[i] else rows_c)["byte_off"][i - r0] = at
            pieces.append((at, int(in_off[i]), int(in_len[i])))
            at += align4(int(in_len[i]))
            if has_bm[i]:
                off = int(bitmaps["bitmap_off"][i])
                if off not in seen:
                    seen[off] = at
                    pieces.append((at, off, bm_len))
                    at += align4(bm_len)
                bm_c["bitmap_off"][i - r0] = seen[off]
        miss_c = None if missing is None else missing[r0:r1].copy()
        idx_c, total = (np.zeros(0, dtype=np.intp), 0) if kind is None else coded_rows(kind, recs_c, rows_c, miss_c)
        yield Chunk(r0, r1, pieces, at, rows_c, recs_c, bm_c, idx_c, total, miss_c)
        r0 = r1


def host_chunks(op, buf, rows, bitmaps, kind, recs, chunk_rows, extra_cost=0, missing=None, **apply_kw):
    """The chunks of `plan_chunks`, one after the other: the chunk's bytes staged and copied to the device, its coded rows
    unpacked behind them into the same buffer (kind.unpack_entry), the device gather (`op.apply_grib` with apply_kw).
    Yields (first row, end row, the chunk's float64 Y on the device, the chunk's row records as the gather took them:
    a complex-packed row with the width its integers were stored at).  A chunk stays within 256 MiB and a quarter of the
    free device memory."""
    if bitmaps is not None:
        bitmaps, _ = grib_bitmaps(bitmaps, rows.size)
    if kind is not None:
        recs = records(kind, recs, rows)
        missing = missing_of(missing, rows)
        coded_rows(kind, recs, rows, missing)      # the layout entry refuses a malformed record ahead of all device work
        refuse_bitmap_with_missing(bitmaps, missing, kind.is_coded(recs, rows))
    free, _ = device.mem_info()
    target = min(256 << 20, max(free // 4, 1))
    for c in plan_chunks(buf.size, rows, bitmaps, kind, recs, op.n_src, op.n_dst, chunk_rows, target, extra_cost, missing):
        staged = np.zeros(max(c.staged_bytes, 4), dtype=np.uint8)
        for a, off, n in c.pieces:
            staged[a:a + n] = buf[off:off + n]
        at, rows_c, bm_c = c.staged_bytes, c.rows, c.bitmaps
        both = DeviceArray((max(at + c.coded_bytes, 4),), np.uint8)
        src = DeviceArray((staged.size,), np.uint8, ptr=both.ptr, base=both).copy_from_host(staged)
        if c.coded_idx.size:
            dst = DeviceArray((c.coded_bytes,), np.uint8, ptr=both.ptr + at, base=both)
            rows_c, bm_c = unpack(kind, src, at, dst, at, rows_c, c.recs, c.coded_idx, None, c.missing, bm_c, op.n_src)
        yield c.r0, c.r1, op.apply_grib(both, rows_c, x_bytes=at + c.coded_bytes, bitmaps=bm_c, **apply_kw), rows_c
