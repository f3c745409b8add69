"""What the GRIB calls of `SparseOperator` / `OperatorGroup` and the device wrappers `grib_unpack` / `grib_unpack_cpx` /
`grib_aec_pack` / `grib_cpx_pack` share: the check of the packed bytes, the two device steps between coded and
simple-packed streams, the entry dispatch, the result checks, and the chunk loop of the host calls whose rows are decoded
or coded on the device -- its plan (`plan_chunks`, host only) apart from its execution (`host_chunks`).  What follows from
the kind of coded row (CCSDS, complex packing) stands in the codec table of `griblite` (`CCSDS`, `CPX`); a call's coded rows
travel as one `CodedRows` -- the codec, its records and the rows' missing value management -- or None."""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib, device
from .device import DeviceArray, _stream_handle, result_cache
from .griblite import CCSDS, CPX, cpx_missing_cost  # noqa: F401  the codec table, read through this module too
from .griblite import GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CodedRows, GribField, _cast, align4


def grib_rows(rows):
    rows = np.ascontiguousarray(rows, dtype=GRIB_ROW_DTYPE).ravel()
    return rows, _cast(rows, _lib.GribRowStruct)


def grib_bitmaps(bitmaps, n_batch):
    bitmaps = np.ascontiguousarray(bitmaps, dtype=GRIB_BITMAP_DTYPE).ravel()
    if bitmaps.size != n_batch:
        raise ValueError(f"{bitmaps.size} bitmap records for {n_batch} rows")
    return bitmaps, _cast(bitmaps, _lib.GribBitmapStruct)


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


def transcode_args(who, device_bytes, rows, x_bytes, out, coded, total_of, **keywords):
    """What `unpack_device` and `pack_device` check alike: (pointer, n_bytes) of the bytes, the row records, the coded
    rows -- given, or built from the wrappers' keywords --, and `out` -- given or fresh -- holding at least the
    total_of(coded) bytes their streams need."""
    x_ptr, n_bytes = packed_bytes(device_bytes, x_bytes, who)
    rows, _ = grib_rows(rows)
    coded = coded or CodedRows.of(rows.size, **keywords)
    if coded is None:
        raise TypeError(f"{who} takes one record per field")
    return x_ptr, n_bytes, rows, coded, device.packed_out(out, total_of(coded))


def unpack_device(who, device_bytes, rows, x_bytes=None, out=None, stream=None, coded=None, **keywords):
    """`grib_unpack` (ccsds=), `grib_unpack_cpx` (cpx=) and `grib_unpack_cpx_mv` (cpx=, cpx_missing=): (out, the rows of
    the streams written, their bitmap records -- None for a call without missing value management)."""
    x_ptr, n_bytes, rows, coded, out = transcode_args(who, device_bytes, rows, x_bytes, out, coded, CodedRows.nbytes, **keywords)
    return (out,) + coded.codec.unpack(device.current_device(), x_ptr, n_bytes, coded.recs, coded.missing, rows,
                                       ctypes.c_void_p(out.ptr), out.nbytes, _stream_handle(stream))


def pack_device(who, device_bytes, rows, x_bytes=None, out=None, stream=None, coded=None, **keywords):
    """`grib_aec_pack` (ccsds=) and `grib_cpx_pack` (cpx=): (out cut to the bytes used, the rows with byte_off at their
    streams, the records of the streams written)."""
    x_ptr, n_bytes, rows, want, out = transcode_args(who, device_bytes, rows, x_bytes, out, coded, CodedRows.bound, **keywords)
    used, recs_out = want.codec.pack(device.current_device(), x_ptr, n_bytes, rows, want.recs, ctypes.c_void_p(out.ptr),
                                     out.nbytes, _stream_handle(stream))
    rows_out = rows.copy()
    rows_out["byte_off"] = recs_out["byte_off"]
    return DeviceArray((used,), np.uint8, ptr=out.ptr, base=out), rows_out, recs_out


def unpack(coded, src, n_bytes, dst, shift, rows, idx, stream, bitmaps=None, n_src=0):
    """The coded streams of rows `idx` in src[:n_bytes] become simple-packed streams in dst.  Returns (the row table with
    those rows pointing at `shift` + their place in dst (complex-packed ones with the width their integers were stored
    at), the others as they were; the bitmap table).  A row with missing values inside its stream gets the bitmap the
    device step wrote behind its slot -- offsets shifted like byte_off, a table of GRIB_NO_BITMAP over n_src points made
    first when the call has none -- and the count of its present values."""
    _, rows_c, bm_c = unpack_device("apply_grib", src, rows[idx], x_bytes=n_bytes, out=dst, stream=stream, coded=coded[idx])
    written = np.flatnonzero(bm_c["bitmap_off"] != GRIB_NO_BITMAP) if bm_c is not None else ()
    if len(written):
        if bitmaps is None:
            bitmaps = np.zeros(rows.size, dtype=GRIB_BITMAP_DTYPE)
            bitmaps["bitmap_off"], bitmaps["n_values"] = GRIB_NO_BITMAP, n_src
        else:
            bitmaps = bitmaps.copy()
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
# staged, every piece at a 4-byte-aligned offset --, the staged bytes, the row / bitmap records and the coded rows with
# byte_off and bitmap_off rewritten to the staged offsets (bitmaps: None without bitmaps, coded: None without coded
# rows), the chunk's coded rows and the bytes of their transcoded streams.
class Chunk(namedtuple("Chunk", "r0 r1 pieces staged_bytes rows bitmaps coded coded_idx coded_bytes")):
    recs = property(lambda c: c.coded and c.coded.recs)
    missing = property(lambda c: c.coded and c.coded.missing)


def plan_chunks(buf_size, rows, bitmaps, coded, n_src, n_dst, chunk_rows, target, extra_cost=0):
    """The chunks of consecutive rows an `apply_host_grib` call with coded rows (`coded`, a `CodedRows`) or a coded
    result (coded None: every row is simple-packed) goes through, one after the other (an iterator of `Chunk`); host
    only.  A row costs its staged bytes (coded or simple-packed stream, bitmap), for a coded row `coded.device_cost`
    (one with missing values inside its stream `cpx_missing_cost` more), its float64 Y and extra_cost (bytes per row,
    what the caller puts beside them); a chunk takes rows while their cost stays within `target` bytes, and at least
    one; chunk_rows > 0 fixes the rows.  A bitmap several rows of a chunk share is staged once in it (and again in the
    next chunk).  A row with a bitmap and missing values inside its stream is refused ahead of the first chunk."""
    n_batch, S = rows.size, n_src
    is_coded = np.zeros(n_batch, dtype=bool) if coded is None else coded.is_coded(rows)
    has_bm = np.zeros(n_batch, dtype=bool) if bitmaps is None else bitmaps["bitmap_off"] != GRIB_NO_BITMAP
    n_val = np.full(n_batch, S, dtype=np.int64) if bitmaps is None else \
        np.where(has_bm, bitmaps["n_values"], S).astype(np.int64)
    nbits = rows["nbits"].astype(np.int64)
    in_off, in_len, device_cost = rows["byte_off"].astype(np.uint64), (n_val * nbits + 7) // 8, 0
    if coded is not None:
        recs = coded.recs
        if (recs["n_values"][is_coded].astype(np.int64) != n_val[is_coded]).any():
            raise ValueError("a coded row's record has n_values different from the points its row holds")
        in_off = np.where(is_coded, recs["byte_off"], in_off).astype(np.uint64)
        in_len = np.where(is_coded, recs["byte_len"].astype(np.int64), in_len).astype(np.int64)
        coded.refuse_bitmaps(bitmaps, is_coded)
        device_cost = coded.device_cost(is_coded, n_val, nbits)
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
        coded_c = None if coded is None else coded[r0:r1]
        bm_c = None if bitmaps is None else bitmaps[r0:r1].copy()
        pieces, at, seen = [], 0, {}
        for i in range(r0, r1):
            (coded_c.recs if is_coded[i] else rows_c)["byte_off"][i - r0] = at
            pieces.append((at, int(in_off[i]), int(in_len[i])))
            at += align4(int(in_len[i]))
            if has_bm[i]:
                off = int(bitmaps["bitmap_off"][i])
                if off not in seen:
                    seen[off] = at
                    pieces.append((at, off, bm_len))
                    at += align4(bm_len)
                bm_c["bitmap_off"][i - r0] = seen[off]
        idx_c = np.flatnonzero(is_coded[r0:r1])
        total = coded_c[idx_c].nbytes() if idx_c.size else 0
        yield Chunk(r0, r1, pieces, at, rows_c, bm_c, coded_c, idx_c, total)
        r0 = r1


def host_chunks(op, buf, rows, bitmaps, coded, chunk_rows, extra_cost=0, **apply_kw):
    """The chunks of `plan_chunks`, one after the other: the chunk's bytes staged and copied to the device, its coded rows
    unpacked behind them into the same buffer (`unpack`), the device gather (`op.apply_grib` with apply_kw).
    Yields (first row, end row, the chunk's float64 Y on the device, the chunk's row records as the gather took them:
    a complex-packed row with the width its integers were stored at).  A chunk stays within 256 MiB and a quarter of the
    free device memory."""
    if bitmaps is not None:
        bitmaps, _ = grib_bitmaps(bitmaps, rows.size)
    if coded is not None:
        coded.streams(rows, bitmaps)      # a malformed record, a bitmap beside missing values: refused ahead of all device work
    free, _ = device.mem_info()
    target = min(256 << 20, max(free // 4, 1))
    for c in plan_chunks(buf.size, rows, bitmaps, coded, op.n_src, op.n_dst, chunk_rows, target, extra_cost):
        staged = np.zeros(max(c.staged_bytes, 4), dtype=np.uint8)
        for a, off, n in c.pieces:
            staged[a:a + n] = buf[off:off + n]
        at, rows_c, bm_c = c.staged_bytes, c.rows, c.bitmaps
        both = DeviceArray((max(at + c.coded_bytes, 4),), np.uint8)
        src = DeviceArray((staged.size,), np.uint8, ptr=both.ptr, base=both).copy_from_host(staged)
        if c.coded_idx.size:
            dst = DeviceArray((c.coded_bytes,), np.uint8, ptr=both.ptr + at, base=both)
            rows_c, bm_c = unpack(c.coded, src, at, dst, at, rows_c, c.coded_idx, None, bm_c, op.n_src)
        yield c.r0, c.r1, op.apply_grib(both, rows_c, x_bytes=at + c.coded_bytes, bitmaps=bm_c, **apply_kw), rows_c
