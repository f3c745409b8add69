"""Minimal GRIB reader (editions 1 and 2): grid-point fields in simple packing on lon/lat, regular Gaussian and
reduced Gaussian grids, laid out as cfgrib lays them out for xarray.

The reference's own tests read one GRIB file, `tests/data/lsm-ifs.grb` (identity2d_test.py:22-27, util_test.py:57: an
IFS land-sea mask on the octahedral reduced Gaussian grid O96), through `xarray.open_mfdataset` + cfgrib / ecCodes, and hand the
file name to `cdo` for the weights.  Neither is on this image, so the field and its grid are decoded here from the
published WMO FM 92 GRIB edition-1 layout (sections 0-5; ECMWF local table 128 for the variable names):

    section 0  'GRIB', total length (3 octets), edition
    section 1  product definition: parameter, level, reference time, decimal scale factor D
    section 2  grid description: representation type (0 lon/lat, 4 Gaussian), Ni, Nj, first / last point, N,
               scanning mode, and for reduced grids the list PL of points per row
    section 3  optional bitmap of the points that carry a value
    section 4  binary data: binary scale factor E, reference value R (IBM hexadecimal float), bits per value, X
               value = (R + X * 2^E) / 10^D

Conventions of cfgrib kept: variable names (`lsm`, `t2m`, ...), dimensions (`latitude`, `longitude`) for rectangular
grids and (`values`,) with `latitude(values)` / `longitude(values)` for reduced ones, `time` / level dimensions only
when a file holds more than one of them, missing points as NaN, float32 fields.

Edition 2 (WMO FM 92 GRIB edition 2; what newer IFS / ICON output comes in) is decoded for the same family: sections
0 - 8, grid definition templates 3.0 (lon/lat) and 3.40 (Gaussian, regular or with the list of points per row),
product definition templates 4.0 / 4.1 / 4.8 / 4.11 (the leading octets they share), data representation templates 5.0
(simple packing, IEEE reference value) and 5.42 (CCSDS packing: the same rule on integers that an adaptive entropy
coder compressed; decoded by the library's host decoder, smm_grib_aec_decode_host), 5.2 and 5.3 (complex packing, plain
and with spatial differencing -- what NCEP writes; the same rule on integers coded in groups of their own widths,
smm_grib_cpx_decode_host; missing value management 1 and 2 -- missing values coded inside the groups, wgrib2's way
for undefined points -- with `cpx_missing=True`, smm_grib_cpx_decode_host_mv, else refused), bitmap section, several fields per message (repeated
sections 2 - 7).

Anything else in a GRIB file (spherical harmonics, GRIB-1 second-order / JPEG / PNG packing, rotated or projected
grids) raises GribUnsupported naming the feature.
"""
import ctypes
from collections import namedtuple

import numpy as np

from . import _lib
from .xrlite import DataArray, Dataset


class GribUnsupported(NotImplementedError):
    pass


# smm_grib_row_t, field for field: one record per GRIB field of a variable kept raw (open_grib(path, decode=False))
GRIB_ROW_DTYPE = np.dtype({"names": ["byte_off", "ref", "bscale", "ddiv", "nbits", "reserved"],
                           "formats": ["<u8", "<f8", "<f8", "<f8", "<i4", "<i4"],
                           "offsets": [0, 8, 16, 24, 32, 36], "itemsize": 40})


# smm_grib_bitmap_t, field for field: one record per GRIB field of a raw-kept variable some of whose messages carry a
# bitmap -- where the bitmap's bytes start in the file (GRIB_NO_BITMAP: the message has none) and how many values the
# message's packed stream holds (the set bits; the grid's points without a bitmap)
GRIB_BITMAP_DTYPE = np.dtype({"names": ["bitmap_off", "n_values"], "formats": ["<u8", "<u8"], "offsets": [0, 8],
                              "itemsize": 16})
GRIB_NO_BITMAP = 2 ** 64 - 1

# smm_grib_encode_t, field for field: how one result row is packed (GribEncode)
GRIB_ENCODE_DTYPE = np.dtype({"names": ["ddiv", "nbits", "reserved"], "formats": ["<f8", "<i4", "<i4"],
                              "offsets": [0, 8, 12], "itemsize": 16})


# smm_grib_aec_t, field for field: one record per GRIB field of a raw-kept variable some of whose messages are CCSDS-packed
# (template 5.42) -- where the message's coded stream lies in the file, how many integers it codes and with which
# parameters.  block_size == 0: the field is simple-packed, its row record says it all
GRIB_AEC_DTYPE = np.dtype({"names": ["byte_off", "byte_len", "n_values", "nbits", "block_size", "rsi", "flags", "reserved"],
                           "formats": ["<u8", "<u8", "<u8", "<i4", "<i4", "<i4", "<u4", "<u8"],
                           "offsets": [0, 8, 16, 24, 28, 32, 36, 40], "itemsize": 48})
# ccsdsFlags (libaec's AEC_* bits): the preprocessor switch is honoured, the two container bits say nothing about the
# stream, the others are refused
_AEC_PREPROCESS = 8
_AEC_REFUSED = {1: "AEC_DATA_SIGNED (signed samples)", 16: "AEC_RESTRICTED (the restricted code set)",
                32: "AEC_PAD_RSI (byte-padded reference sample intervals)"}


def aec_decode(buf, rec, histogram=None):
    """The unsigned integers (uint32) of one CCSDS stream: `rec` a GRIB_AEC_DTYPE record over the bytes `buf`, decoded
    by the library on the host (smm_grib_aec_decode_host; no GPU involved).  histogram: a uint64 array of 7 counters the
    coding options taken are added to (`_lib.GRIB_AEC_OPTIONS`).  A stream that does not end ok is a ValueError."""
    rec = np.ascontiguousarray(rec, dtype=GRIB_AEC_DTYPE).reshape(1)
    raw = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf)
    out = np.empty(int(rec["n_values"][0]), dtype=np.uint32)
    status = ctypes.c_int(0)
    hist = None if histogram is None else histogram.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    _lib.call("smm_grib_aec_decode_host", ctypes.c_void_p(raw.ctypes.data if raw.size else None), raw.size,
              CCSDS.cast(rec), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), hist, ctypes.byref(status))
    if status.value != _lib.GRIB_AEC_OK:
        raise ValueError("CCSDS stream " + ("ends before its values do" if status.value == _lib.GRIB_AEC_EXHAUSTED
                                            else "is invalid"))
    return out


# smm_grib_cpx_t, field for field: one record per GRIB field of a raw-kept variable some of whose messages are complex-packed
# (templates 5.2 / 5.3) -- where section 7's bytes lie in the file, how many integers they code, and section 5's group
# parameters.  order == GRIB_CPX_SIMPLE (-1): the field is simple-packed, its row record says it all
GRIB_CPX_DTYPE = np.dtype({"names": ["byte_off", "byte_len", "n_values", "n_groups", "nbits", "width_ref", "width_bits",
                                     "length_ref", "length_inc", "length_last", "length_bits", "order", "n_oct", "reserved"],
                           "formats": ["<u8", "<u8", "<u8", "<u4", "<i4", "<u4", "<i4", "<u4", "<u4", "<u4", "<i4", "<i4", "<i4",
                                       "<u8"],
                           "offsets": [0, 8, 16, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64], "itemsize": 72})
GRIB_CPX_SIMPLE = -1


def cpx_decode(buf, rec):
    """The integers X (uint32) of one complex-packed stream: `rec` a GRIB_CPX_DTYPE record over the bytes `buf`, decoded
    by the library on the host (smm_grib_cpx_decode_host; no GPU involved).  A row that does not end ok is a
    ValueError."""
    rec = np.ascontiguousarray(rec, dtype=GRIB_CPX_DTYPE).reshape(1)
    raw = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf)
    out = np.empty(int(rec["n_values"][0]), dtype=np.uint32)
    status = ctypes.c_int(0)
    _lib.call("smm_grib_cpx_decode_host", ctypes.c_void_p(raw.ctypes.data if raw.size else None), raw.size,
              CPX.cast(rec), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(status))
    if status.value != _lib.GRIB_CPX_OK:
        raise ValueError("complex-packed stream " + ("ends before its tables or its groups' bits do"
                                                     if status.value == _lib.GRIB_CPX_EXHAUSTED else "is invalid"))
    return out


def cpx_decode_mv(buf, rec, mvm):
    """(the P present integers X (uint32), present: a bool per coded position) of one complex-packed stream whose
    missing value management (section 5's octet 23) is `mvm` -- 1 or 2: missing values are codes inside the groups, by
    the rule of smm_grib_cpx.hpp; 0: every position is present.  Decoded by the library on the host
    (smm_grib_cpx_decode_host_mv; no GPU involved).  A row that does not end ok is a ValueError."""
    rec = np.ascontiguousarray(rec, dtype=GRIB_CPX_DTYPE).reshape(1)
    raw = np.frombuffer(buf, dtype=np.uint8) if not isinstance(buf, np.ndarray) else np.ascontiguousarray(buf)
    n = int(rec["n_values"][0])
    out, present = np.empty(n, dtype=np.uint32), np.empty(n, dtype=np.uint8)
    status, count, m = ctypes.c_int(0), ctypes.c_uint64(0), ctypes.c_uint8(int(mvm))
    _lib.call("smm_grib_cpx_decode_host_mv", ctypes.c_void_p(raw.ctypes.data if raw.size else None), raw.size,
              CPX.cast(rec), ctypes.byref(m), out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
              present.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)),
              ctypes.byref(count), ctypes.byref(status))
    if status.value != _lib.GRIB_CPX_OK:
        raise ValueError("complex-packed stream " + ("ends before its tables or its groups' bits do"
                                                     if status.value == _lib.GRIB_CPX_EXHAUSTED else "is invalid"))
    return out[:int(count.value)].copy(), present.astype(bool)


def aec_encode(values, record, histogram=None):
    """The CCSDS stream (a uint8 array) of the unsigned integers `values`, coded by the library on the host
    (smm_grib_aec_encode_host; no GPU involved) by THE RULE OF THIS ENCODER of smm_grib_aec.hpp -- the oracle of
    smm_grib_aec_pack.  record: a GRIB_AEC_DTYPE record whose nbits, block_size, rsi and flags say how to code (n_values
    is set from `values`, byte_off and byte_len are not read).  histogram: a uint64 array of 7 counters the coding options
    taken are added to (`_lib.GRIB_AEC_OPTIONS`)."""
    v = np.ascontiguousarray(values, dtype=np.uint32).ravel()
    rec = np.array(record, dtype=GRIB_AEC_DTYPE).reshape(1)
    rec["n_values"], rec["byte_off"], rec["byte_len"] = v.size, 0, 0
    bound = int(CCSDS.bounds(rec)[0])
    out = np.zeros(max(bound, 1), dtype=np.uint8)
    used = ctypes.c_uint64(0)
    hist = None if histogram is None else histogram.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    _lib.call("smm_grib_aec_encode_host", v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), v.size, CCSDS.cast(rec),
              ctypes.c_void_p(out.ctypes.data), bound, ctypes.byref(used), hist)
    return out[:int(used.value)].copy()


def cpx_encode(values, rec):
    """(stream: a uint8 array, its GRIB_CPX_DTYPE record with byte_off 0) of the unsigned integers `values`, coded as a
    complex-packed stream by the library on the host (smm_grib_cpx_encode_host; no GPU involved) by THE RULE OF THIS
    ENCODER of smm_grib_cpx.hpp -- the oracle of smm_grib_cpx_pack.  rec: a GRIB_CPX_DTYPE record whose nbits (the width
    of the integers), order (wanted, 0..2) and length_ref (the group length: 8, 16, 32 or 64) say how to code; n_values
    is set from `values`, nothing else is read.  Integers of width 0 are not coded: no bytes, and a record whose order is
    GRIB_CPX_SIMPLE."""
    v = np.ascontiguousarray(values, dtype=np.uint32).ravel()
    rec = np.array(rec, dtype=GRIB_CPX_DTYPE).reshape(1)
    rec["n_values"] = v.size
    bound = int(CPX.bounds(rec)[0])
    out = np.zeros(max(bound, 1), dtype=np.uint8)
    used = ctypes.c_uint64(0)
    rec_out = np.zeros(1, dtype=GRIB_CPX_DTYPE)
    _lib.call("smm_grib_cpx_encode_host", v.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), v.size, CPX.cast(rec),
              ctypes.c_void_p(out.ctypes.data), bound, ctypes.byref(used), CPX.cast(rec_out))
    return out[:int(used.value)].copy(), rec_out[0]


def cpx_want(nbits, order, group_len, n_values=0):
    """The wanted GRIB_CPX_DTYPE record(s) of `cpx_encode` / `device.grib_cpx_pack`: integers of nbits bits coded at
    `order` in groups of group_len values.  Scalars give one record, arrays one per entry."""
    shape = np.broadcast(nbits, order, group_len, n_values).shape
    rec = np.zeros(shape, dtype=GRIB_CPX_DTYPE)
    rec["nbits"], rec["order"], rec["length_ref"], rec["n_values"] = nbits, order, group_len, n_values
    return rec


# ---------------------------------------------------------------------------------------------- the codec table
def align4(v):
    return (v + 3) // 4 * 4


def _cast(records, struct):
    return ctypes.cast(records.ctypes.data, ctypes.POINTER(struct))


class Codec(namedtuple("Codec", "name noun packing packed stream result dtype struct layout_entry unpack_entry bound_entry pack_entry "
                                "mv_entries is_coded device_cost missing_cost out_scratch takes default params_of wanted "
                                "encode decode")):
    """One way GRIB codes a field's integers beside simple packing, for both directions: coded rows regridded raw
    (`ccsds=`, `cpx=`) and results coded on their way out (`GribEncode(..., ccsds= / cpx=)`).  Everything that follows
    from the kind of coded row stands here; a further codec is a further entry of `CODECS`.
    name: the keyword and attribute that carries its records; noun, packing, packed, stream, result: what messages call it.
    dtype, struct: its record, one per row; layout_entry, unpack_entry, bound_entry, pack_entry: the C entries behind
    `layout`, `unpack`, `bounds` and `pack`; mv_entries: the layout and unpack entries that take the rows' missing value
    management and give bitmaps, for a call that carries one (None: the codec has no missing values inside its streams).
    is_coded(recs, rows): which rows have a coded stream -- the others are simple-packed.
    device_cost(recs, n_val, nbits): the device bytes a coded row costs in a chunk beside its staged stream;
    missing_cost(n_val): what a row with missing values inside its stream costs more.
    out_scratch(n_dst): the device bytes a result row costs beside its stream's bound; takes: the names of the codecs
    the input of a call may be coded with when its result is coded this way (simple-packed input always goes).
    default, params_of(rec), wanted(*params): the parameters `True` stands for, those of a record, and the record that
    asks for them (a ValueError when they are not valid).
    encode(q, rec) -> (stream, the stream's record) and decode(buf, rec, mvm) -> (q, present or None): the host coder
    and decoder; a field of width 0 has no stream, and the coder marks its record simple-packed."""
    __slots__ = ()

    def cast(self, recs):
        return _cast(recs, self.struct)

    def params(self, want):
        """Records with the wanted parameters set, from True, one tuple of parameters, a list of them or records."""
        if want is True:
            want = self.default
        if isinstance(want, np.ndarray) and want.dtype == self.dtype:
            par = [self.params_of(r) for r in want.ravel()]
        else:
            par = [tuple(want)] if np.ndim(want[0]) == 0 else [tuple(c) for c in want]
        rec = np.zeros(len(par), dtype=self.dtype)
        for i, p in enumerate(par):
            rec[i] = self.wanted(*p)
        return rec

    def layout(self, recs, missing=None):
        """Bytes the simple-packed streams (and bitmaps) the records' streams unpack to take; host only, and a malformed
        record is refused.  missing: the rows' missing value management, or None."""
        total = ctypes.c_uint64(0)
        if missing is None:
            _lib.call(self.layout_entry, self.cast(recs), recs.size, None, ctypes.byref(total))
        else:
            _lib.call(self.mv_entries[0], self.cast(recs), missing.ctypes.data_as(_lib._u8p), recs.size, None, None,
                      ctypes.byref(total))
        return int(total.value)

    def bounds(self, recs):
        """Bytes the coded stream of each wanted record takes at most (int64); host only."""
        offs, total = np.zeros(recs.size + 1, dtype=np.uint64), ctypes.c_uint64(0)
        _lib.call(self.bound_entry, self.cast(recs), recs.size, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)),
                  ctypes.byref(total))
        offs[recs.size] = total.value
        return np.diff(offs).astype(np.int64)

    def unpack(self, dev, x_ptr, n_bytes, recs, missing, rows, out_ptr, out_bytes, stream):
        """The device step from coded to simple-packed streams.  Returns (the rows of the streams written, their bitmap
        records -- None for a call without missing value management)."""
        rows_out = np.zeros(rows.size, dtype=GRIB_ROW_DTYPE)
        tail = (_cast(rows, _lib.GribRowStruct), rows.size, out_ptr, out_bytes, _cast(rows_out, _lib.GribRowStruct))
        if missing is None:
            _lib.call(self.unpack_entry, dev, x_ptr, n_bytes, self.cast(recs), *tail, stream)
            return rows_out, None
        bitmaps_out = np.zeros(rows.size, dtype=GRIB_BITMAP_DTYPE)
        _lib.call(self.mv_entries[1], dev, x_ptr, n_bytes, self.cast(recs), missing.ctypes.data_as(_lib._u8p), *tail,
                  _cast(bitmaps_out, _lib.GribBitmapStruct), stream)
        return rows_out, bitmaps_out

    def pack(self, dev, x_ptr, n_bytes, rows, recs, out_ptr, out_bytes, stream):
        """The device step from simple-packed to coded streams.  Returns (bytes used, the records of the streams)."""
        recs_out, used = np.zeros(rows.size, dtype=self.dtype), ctypes.c_uint64(0)
        _lib.call(self.pack_entry, dev, x_ptr, n_bytes, _cast(rows, _lib.GribRowStruct), self.cast(recs), rows.size,
                  out_ptr, out_bytes, self.cast(recs_out), ctypes.byref(used), stream)
        return int(used.value), recs_out


def _aec_wanted(block, rsi, pre):
    if int(block) not in (8, 16, 32, 64) or not 1 <= int(rsi) <= 4096:
        raise ValueError(f"CCSDS block size {block} / reference sample interval {rsi}: 8, 16, 32 or 64 and 1..4096")
    return (0, 0, 0, 0, int(block), int(rsi), 0x06 | (_AEC_PREPROCESS if pre else 0), 0)


def _aec_code(q, rec):
    if int(rec["nbits"]) == 0:
        rec = rec.copy()
        rec["block_size"] = 0
        return np.zeros(0, dtype=np.uint8), rec
    return aec_encode(q, rec), rec


def _cpx_wanted(order, group_len):
    if int(order) not in (0, 1, 2) or int(group_len) not in (8, 16, 32, 64):
        raise ValueError(f"complex packing of order {order} in groups of {group_len}: 0, 1 or 2 and 8, 16, 32 or 64")
    return cpx_want(0, int(order), int(group_len))


def cpx_missing_cost(n_val):
    """Device bytes a complex-packed row with missing values inside its groups costs beside `CPX.device_cost`: its
    bitmap slot, 8 B more per value -- the integers pass through a second array on their way to their ranks -- and 4 B
    per 256 values."""
    return align4((n_val + 7) // 8) + 8 * n_val + 4 * ((n_val + 255) // 256)


# a record with block_size 0 marks a simple-packed row, a row of width 0 has no stream at all; a coded row costs its
# transcoded stream and 4 B per sample of scratch; a result row 8 B per block and 12 B per segment of scratch
CCSDS = Codec(
    "ccsds", "CCSDS", "CCSDS packing", "CCSDS-packed", "CCSDS stream", "CCSDS-coded", GRIB_AEC_DTYPE, _lib.GribAecStruct,
    "smm_grib_aec_layout", "smm_grib_aec_unpack", "smm_grib_aec_pack_bound", "smm_grib_aec_pack", mv_entries=None,
    is_coded=lambda recs, rows: (recs["block_size"] != 0) & (rows["nbits"] != 0),
    device_cost=lambda recs, n_val, nbits: align4((n_val * nbits + 7) // 8) + 4 * n_val, missing_cost=None,
    out_scratch=lambda n_dst: (n_dst // 8 + 1) * 20, takes=("ccsds",), default=(32, 128, True),
    params_of=lambda r: (int(r["block_size"]), int(r["rsi"]), bool(int(r["flags"]) & _AEC_PREPROCESS)),
    wanted=_aec_wanted, encode=_aec_code, decode=lambda buf, rec, mvm: (aec_decode(buf, rec), None))
# a record whose order is GRIB_CPX_SIMPLE marks a simple-packed row; a coded row costs its slot of 4 B per value and
# 8 B per value plus 16 B per group of scratch; a result row 8 B per group of at least 8 values and 12 B per 1024 values
# of scratch
CPX = Codec(
    "cpx", "complex-packing", "complex packing", "complex-packed", "complex-packed stream", "complex-packed",
    GRIB_CPX_DTYPE, _lib.GribCpxStruct,
    "smm_grib_cpx_layout", "smm_grib_cpx_unpack", "smm_grib_cpx_pack_bound", "smm_grib_cpx_pack",
    mv_entries=("smm_grib_cpx_layout_mv", "smm_grib_cpx_unpack_mv"),
    is_coded=lambda recs, rows: recs["order"] != GRIB_CPX_SIMPLE,
    device_cost=lambda recs, n_val, nbits: 12 * n_val + 16 * recs["n_groups"].astype(np.int64) + 256,
    missing_cost=cpx_missing_cost, out_scratch=lambda n_dst: n_dst + 8 + (n_dst // 1024 + 1) * 12, takes=("cpx",),
    default=(2, 32), params_of=lambda r: (int(r["order"]), int(r["length_ref"])), wanted=_cpx_wanted, encode=cpx_encode,
    decode=lambda buf, rec, mvm: cpx_decode_mv(buf, rec, mvm) if mvm else (cpx_decode(buf, rec), None))
CODECS = (CCSDS, CPX)


def one_codec(why, **given):
    """(codec, what its keyword holds) for the one keyword of a codec (ccsds=, cpx=) that is not None, or (None, None)."""
    given = [(c, given[c.name]) for c in CODECS if given.get(c.name) is not None]
    if len(given) > 1:
        raise ValueError(f"{given[1][0].name} does not go with {given[0][0].name}: {why}")
    return given[0] if given else (None, None)


class CodedRows:
    """The coded rows of a call or of a `GribField`: the codec, its records -- one per row -- and the rows' missing value
    management (one uint8 per row; None when no row has missing values inside its stream)."""

    def __init__(self, codec, recs, missing=None):
        self.codec, self.recs, self.missing = codec, recs, missing

    @classmethod
    def of(cls, n_rows, ccsds=None, cpx=None, cpx_missing=None, what="rows", coded=None):
        """From the public keywords -- or `coded`, a `CodedRows` that stands in their place --, checked against the
        call's `n_rows`; None when nothing is given."""
        if coded is not None:
            if ccsds is not None or cpx is not None or cpx_missing is not None or coded.recs.size != n_rows:
                raise ValueError(f"coded stands in place of ccsds, cpx and cpx_missing, with a record for each of {n_rows} {what}")
            return coded
        codec, recs = one_codec("a call's coded rows are of one kind", ccsds=ccsds, cpx=cpx)
        if cpx_missing is not None and codec is not CPX:
            raise ValueError("cpx_missing goes with cpx")
        if codec is None:
            return None
        recs = np.ascontiguousarray(recs, dtype=codec.dtype).ravel()
        if recs.size != n_rows:
            raise ValueError(f"{recs.size} {codec.noun} records for {n_rows} {what}")
        if cpx_missing is not None:
            cpx_missing = np.ascontiguousarray(cpx_missing, dtype=np.uint8).ravel()
            if cpx_missing.size != n_rows:
                raise ValueError(f"{cpx_missing.size} missing-value-management values for {n_rows} {what}")
        return cls(codec, recs, cpx_missing)

    def __getitem__(self, rows):
        """The coded rows of a slice or an index array of the rows, as a copy: records and missing values stay together."""
        return CodedRows(self.codec, np.array(self.recs[rows]), None if self.missing is None else np.array(self.missing[rows]))

    def is_coded(self, rows):
        return self.codec.is_coded(self.recs, rows)

    def has_missing(self, is_coded):
        return False if self.missing is None else is_coded & (self.missing != 0)

    def streams(self, rows, bitmaps=None):
        """(which rows have a coded stream, bytes of their transcoded streams).  A coded row with a bitmap of its own and
        missing values inside its stream is refused: the two are not composed on the device."""
        is_coded = self.is_coded(rows)
        self.refuse_bitmaps(bitmaps, is_coded)
        idx = np.flatnonzero(is_coded)
        return idx, self[idx].nbytes()

    def refuse_bitmaps(self, bitmaps, is_coded):
        if bitmaps is not None and np.any((bitmaps["bitmap_off"] != GRIB_NO_BITMAP) & self.has_missing(is_coded)):
            raise ValueError("a row has a bitmap and missing values inside its groups: decode it on the host")

    def nbytes(self):
        return self.codec.layout(self.recs, self.missing)

    def bound(self):
        return int(self.codec.bounds(self.recs).sum())

    def device_cost(self, is_coded, n_val, nbits):
        """The device bytes each row costs in a chunk beside its staged stream (0 for a simple-packed row)."""
        cost = np.where(is_coded, self.codec.device_cost(self.recs, n_val, nbits), 0)
        if self.missing is not None:
            cost = cost + np.where(self.has_missing(is_coded), self.codec.missing_cost(n_val), 0)
        return cost


class GribField:
    """The fields of one GRIB variable kept as the file has them: `buf`, the file's bytes (one uint8 array shared by
    every variable of the file), and `rows`, a GRIB_ROW_DTYPE record per field in (time, level) order that says where
    the field's simple-packed values start in `buf` and how they decode -- value = (ref + q * bscale) / ddiv in float64,
    stored as float32.  It stands where the decoded float32 array stands (`shape`, `dtype`, `np.asarray`), and
    `Regridder(packed=True)` hands buf and rows to the GPU as they are (smm_apply_host_grib): the bits are unpacked in
    the kernel, with the results of regridding `decode()`.  `bitmaps` is None, or a GRIB_BITMAP_DTYPE record per field
    (open_grib(path, decode=False, bitmaps=True) on a variable with bitmapped messages): the stream of a bitmapped
    field holds its present points only, the others are NaN (smm_apply_host_grib_bm).  `ccsds` is None, or a
    GRIB_AEC_DTYPE record per field (a variable with CCSDS-packed messages, template 5.42): such a field's q are what
    its coded stream decodes to -- on the GPU for `Regridder(packed=True)` (smm_grib_aec_unpack ahead of the gather),
    on the host for `decode()`; a record with block_size 0 marks a simple-packed field among them.  `cpx` is None, or a
    GRIB_CPX_DTYPE record per field (a variable with complex-packed messages, templates 5.2 / 5.3): such a field's q are
    the integers its groups decode to (smm_grib_cpx_unpack ahead of the gather on the GPU, smm_grib_cpx_decode_host for
    `decode()`), and its row's nbits is the width of the group references, not of q; a record whose order is
    GRIB_CPX_SIMPLE marks a simple-packed field among them.  `cpx_missing` is None, or one uint8 per field beside `cpx`:
    the field's missing value management (1 or 2: missing values are codes inside its groups -- they become NaN;
    smm_grib_cpx_unpack_mv on the GPU, smm_grib_cpx_decode_host_mv for `decode()`).  The three are views of `coded`,
    the `CodedRows` built from them (None for a variable of simple-packed fields only), which the calls take whole."""

    dtype = np.dtype(np.float32)

    def __init__(self, buf, rows, shape, n_points, bitmaps=None, ccsds=None, cpx=None, cpx_missing=None):
        """n_points: grid points of one field -- the product of the trailing (horizontal) axes of `shape`."""
        self.buf = buf
        self.rows = np.ascontiguousarray(rows, dtype=GRIB_ROW_DTYPE).ravel()
        self.bitmaps = None if bitmaps is None else np.ascontiguousarray(bitmaps, dtype=GRIB_BITMAP_DTYPE).ravel()
        if self.bitmaps is not None and self.bitmaps.size != self.rows.size:
            raise ValueError(f"{self.bitmaps.size} bitmap records for {self.rows.size} GRIB fields")
        if ccsds is not None and cpx is not None:
            raise ValueError("a GribField holds CCSDS records or complex-packing records, not both")
        self.coded = CodedRows.of(self.rows.size, ccsds, cpx, cpx_missing, what="GRIB fields")
        self.shape = tuple(int(n) for n in shape)
        self.n_points = int(n_points)
        if self.rows.size * self.n_points != int(np.prod(self.shape)):
            raise ValueError(f"{self.rows.size} GRIB fields of {self.n_points} points for a variable of shape {self.shape}")

    def _coded_as(self, codec):
        return self.coded is not None and self.coded.codec is codec

    ccsds = property(lambda self: self.coded.recs if self._coded_as(CCSDS) else None)
    cpx = property(lambda self: self.coded.recs if self._coded_as(CPX) else None)
    cpx_missing = property(lambda self: self.coded.missing if self._coded_as(CPX) else None)

    @property
    def ndim(self):
        return len(self.shape)

    @property
    def size(self):
        return int(np.prod(self.shape))

    def decode(self):
        """The float32 array `open_grib(path)` gives for this variable, bit for bit."""
        out = np.empty((self.rows.size, self.n_points), dtype=np.float32)
        is_coded = None if self.coded is None else self.coded.is_coded(self.rows)
        for i, r in enumerate(self.rows):
            rule = (int(r["byte_off"]), float(r["ref"]), float(r["bscale"]), float(r["ddiv"]), int(r["nbits"]))
            bm = None
            if self.bitmaps is not None and int(self.bitmaps[i]["bitmap_off"]) != GRIB_NO_BITMAP:
                bm = (int(self.bitmaps[i]["bitmap_off"]), int(self.bitmaps[i]["n_values"]))
            coded = self.coded[i:i + 1] if is_coded is not None and is_coded[i] else None
            out[i] = _decode_rule(self.buf, rule, self.n_points, bm, coded)
        return out.reshape(self.shape)

    def __array__(self, dtype=None, copy=None):
        a = self.decode()
        return a if dtype is None else a.astype(dtype, copy=False)

    def __repr__(self):
        n_bm = 0 if self.bitmaps is None else int((self.bitmaps["bitmap_off"] != GRIB_NO_BITMAP).sum())
        n_coded = 0 if self.coded is None else int(self.coded.is_coded(self.rows).sum())
        return (f"<GribField {self.shape} float32, {self.rows.size} packed fields, widths "
                f"{sorted(set(self.rows['nbits'].tolist()))}" + (f", {n_coded} {self.coded.codec.packed}" if n_coded else "")
                + (f" ({int((self.cpx_missing != 0).sum())} with missing values inside the groups)"
                   if self.cpx_missing is not None else "")
                + (f", {n_bm} with a bitmap>" if n_bm else ">"))


_FLT_MAX = float(np.finfo(np.float32).max)


class GribEncode:
    """How regrid results go back into GRIB simple packing: a bit width and a decimal scale factor D per field (scalars,
    or one entry per field).  The reference value and the binary scale of a field follow from the field's own minimum
    and maximum by the rule of smm_grib_codec.hpp, which `encode` states in numpy -- the oracle of smm_grib_pack:
        t = v * 10^D; present iff v finite and |t| <= FLT_MAX; R = the largest float32 <= min t; ref = R + 0.0;
        range = max t - ref; E = the smallest integer with range * 2^-E <= 2^nbits - 1 (at least -1022);
        q = rint(ldexp(t - ref, -E)); a constant or empty field has width 0 and no data bits.
    The result decodes with `GribField.decode` (value = (ref + q * 2^E) / 10^D).
    ccsds: None, True or (block_size, rsi, preprocess) -- or one such tuple per field: the q of every field are coded as
    a CCSDS stream (template 5.42) by THE RULE OF THIS ENCODER of smm_grib_aec.hpp instead of stored at their width;
    `encode` is then the host oracle of smm_grib_pack followed by smm_grib_aec_pack.  True means block size 32, a
    reference sample interval of 128 blocks and the preprocessor on, with ccsdsFlags 0x0e -- ecCodes' defaults as
    recalled, not pinned against an ecCodes file (like the section-5 octets).
    cpx: None, True or (order, group_len) -- or one such tuple per field: the q of every field are coded as a
    complex-packed stream (templates 5.2 / 5.3) by THE RULE OF THIS ENCODER of smm_grib_cpx.hpp; `encode` is then the host
    oracle of smm_grib_pack followed by smm_grib_cpx_pack.  True means second-order differencing in groups of 32.  It does
    not go with ccsds.
    A width of `SOURCE_WIDTH` marks a field whose width is the one its complex-packed source row's integers decode to:
    only `apply_host_grib(cpx=..., grib_out=)` can resolve it (`resolved`); everything else refuses the mark."""

    CCSDS_DEFAULT, CPX_DEFAULT = CCSDS.default, CPX.default
    SOURCE_WIDTH = -(1 << 15)      # no width: every other value outside 1..32 is refused

    def __init__(self, nbits, decimal_scale=0, ccsds=None, cpx=None):
        nb, ds = np.asarray(nbits), np.asarray(decimal_scale)
        if nb.ndim > 1 or ds.ndim > 1:
            raise ValueError("nbits and decimal_scale are scalars or one entry per field")
        if not (np.issubdtype(nb.dtype, np.integer) and np.issubdtype(ds.dtype, np.integer)):
            raise ValueError("nbits and decimal_scale are integers")
        if nb.ndim == 1 and ds.ndim == 1 and nb.size != ds.size:
            raise ValueError(f"{nb.size} widths for {ds.size} decimal scale factors")
        self.n_fields = None if nb.ndim == 0 and ds.ndim == 0 else int(max(nb.size if nb.ndim else 0, ds.size if ds.ndim else 0))
        n = 1 if self.n_fields is None else self.n_fields
        self.nbits = np.broadcast_to(nb.astype(np.int32), (n,)).copy()
        self.decimal_scale = np.broadcast_to(ds.astype(np.int64), (n,)).copy()
        if (((self.nbits < 1) | (self.nbits > 32)) & (self.nbits != self.SOURCE_WIDTH)).any():
            raise ValueError("GRIB output widths are 1..32 bits")
        self.codec, want = one_codec("a result is coded one way", ccsds=ccsds, cpx=cpx)
        self.ddiv = np.array([10.0 ** int(d) if abs(int(d)) < 309 else np.inf for d in self.decimal_scale], dtype=np.float64)
        if not (np.isfinite(self.ddiv) & (self.ddiv > 0)).all():
            raise ValueError("10^D must be finite and positive")
        self.params = None if self.codec is None else self.codec.params(want)
        if self.params is not None and self.params.size > 1:
            if self.n_fields is None:      # scalars beside one parameter set per field
                self.n_fields = self.params.size
                self.nbits, self.decimal_scale, self.ddiv = (np.repeat(a, self.n_fields) for a in
                                                              (self.nbits, self.decimal_scale, self.ddiv))
            elif self.params.size != self.n_fields:
                raise ValueError(f"{self.params.size} {self.codec.noun} parameter sets for {self.n_fields} fields")

    def _params(self, codec):
        return self.params if self.codec is codec else None

    ccsds = property(lambda self: self._params(CCSDS))
    cpx = property(lambda self: self._params(CPX))

    @property
    def has_source_width(self):
        return bool((self.nbits == self.SOURCE_WIDTH).any())

    def resolved(self, widths):
        """This rule with every `SOURCE_WIDTH` mark replaced by the entry of `widths` (one per field: what
        smm_grib_cpx_unpack reports for the source rows).  A width of 0 there -- a constant source row -- becomes the
        largest width of the resolved fields, or 16 if all are 0, as `from_field` has it for a constant row."""
        widths = np.asarray(widths, dtype=np.int32).ravel()
        nbits, _ = self._per_field(widths.size, marks=True)
        nbits = np.where(nbits == self.SOURCE_WIDTH, widths, nbits).astype(np.int32)
        top = int(nbits.max()) if nbits.size and nbits.max() > 0 else 16
        return self._like(np.where(nbits == 0, top, nbits).astype(np.int32),
                          np.broadcast_to(self.decimal_scale, nbits.shape).copy(), self.params)

    @classmethod
    def from_field(cls, field, ccsds=None, cpx=None):
        """Each source row's own width and D.  A width of 0 (a constant field) becomes the variable's largest width,
        or 16 if all are 0.  ccsds=True: the result is CCSDS-coded, each field with its source field's own block size,
        interval and preprocessor switch where the source is CCSDS-packed, with the defaults where it is not."""
        if ccsds is True and getattr(field, "ccsds", None) is not None:
            ccsds = [CCSDS.params_of(r) if int(r["block_size"]) else cls.CCSDS_DEFAULT for r in field.ccsds]
        nbits = field.rows["nbits"].astype(np.int32)
        marked = np.zeros(nbits.size, dtype=bool)
        if cpx is True:
            # a complex-packed source row keeps its order and gets groups of 32; its row's nbits is octet 20, the width of
            # its group references, not of its integers: the width is the one the device decode will report
            src = getattr(field, "cpx", None)
            if src is not None:
                marked = src["order"] != GRIB_CPX_SIMPLE
                cpx = [(int(r["order"]), cls.CPX_DEFAULT[1]) if m else cls.CPX_DEFAULT for r, m in zip(src, marked)]
        live = nbits[~marked]
        top = int(live.max()) if live.size and live.max() > 0 else 16
        nbits = np.where(marked, cls.SOURCE_WIDTH, np.where(nbits == 0, top, nbits)).astype(np.int32)
        ddiv = field.rows["ddiv"].astype(np.float64)
        if not (np.isfinite(ddiv) & (ddiv > 0)).all():
            raise ValueError("a source row's ddiv is not finite and positive")
        dec = np.rint(np.log10(ddiv)).astype(np.int64)
        for d, want in zip(dec, ddiv):
            if 10.0 ** int(d) != want:
                raise ValueError(f"ddiv {want!r} is not 10.0 ** D for an integer D")
        return cls(nbits, dec, ccsds=ccsds, cpx=cpx)

    def _like(self, nbits, decimal_scale, params):
        return GribEncode(nbits, decimal_scale, **({} if self.codec is None else {self.codec.name: params}))

    def rows_of(self, r0, r1, n_fields):
        """The GribEncode of fields [r0, r1) of n_fields (`SOURCE_WIDTH` marks stay)."""
        nbits, _ = self._per_field(n_fields, marks=True)
        par = None if self.codec is None else self.coded_records(n_fields, marks=True)[r0:r1]
        return self._like(nbits[r0:r1].copy(), np.broadcast_to(self.decimal_scale, (int(n_fields),))[r0:r1].copy(), par)

    def coded_records(self, n_fields, n_values=0, nbits=0, marks=False, codec=None):
        """The wanted records of n_fields fields for the pack step of this rule's codec (smm_grib_aec_pack,
        smm_grib_cpx_pack): the parameters of this rule, n_values and nbits (the stored widths) as given."""
        codec = codec or self.codec
        self._per_field(n_fields, marks=marks)
        par = self._params(codec)
        rec = np.zeros(int(n_fields), dtype=codec.dtype)
        rec[:] = par if par.size > 1 else par[0]
        rec["n_values"], rec["nbits"] = n_values, nbits
        return rec

    def coded_bounds(self, n_points, n_fields, codec=None):
        """Bytes the coded stream of each of n_fields fields of n_points points takes at most (int64; the codec's
        pack_bound entry)."""
        nbits, _ = self._per_field(n_fields)
        return (codec or self.codec).bounds(self.coded_records(n_fields, int(n_points), nbits, codec=codec))

    def cpx_records(self, n_fields, n_values=0, nbits=0, marks=False):
        """`coded_records` of a rule with `cpx` (smm_grib_cpx_t: order and group length of this rule)."""
        return self.coded_records(n_fields, n_values, nbits, marks, CPX)

    def cpx_bound(self, n_points, n_fields):
        """Bytes the coded streams of n_fields fields of n_points points take at most (smm_grib_cpx_pack_bound)."""
        return int(self.coded_bounds(n_points, n_fields, CPX).sum())

    def cpx_bounds(self, n_points, n_fields):
        """The same field by field (int64)."""
        return self.coded_bounds(n_points, n_fields, CPX)

    def ccsds_records(self, n_fields, n_values=0, nbits=0):
        """`coded_records` of a rule with `ccsds` (smm_grib_aec_t: block size, interval and flags of this rule)."""
        return self.coded_records(n_fields, n_values, nbits, codec=CCSDS)

    def ccsds_bound(self, n_points, n_fields):
        """Bytes the coded streams of n_fields fields of n_points points take at most (smm_grib_aec_pack_bound)."""
        return int(self.coded_bounds(n_points, n_fields, CCSDS).sum())

    def ccsds_bounds(self, n_points, n_fields):
        """The same field by field (int64)."""
        return self.coded_bounds(n_points, n_fields, CCSDS)

    def _per_field(self, n_fields, marks=False):
        n_fields = int(n_fields)
        if self.n_fields is not None and self.n_fields != n_fields:
            raise ValueError(f"a GribEncode of {self.n_fields} fields for {n_fields} fields")
        if not marks and self.has_source_width:
            raise ValueError("a width of GribEncode.SOURCE_WIDTH is the width of a complex-packed source row: only "
                             "apply_host_grib(cpx=..., grib_out=) resolves it")
        return np.broadcast_to(self.nbits, (n_fields,)), np.broadcast_to(self.ddiv, (n_fields,))

    def records(self, n_fields):
        """The smm_grib_encode_t records of n_fields fields."""
        nbits, ddiv = self._per_field(n_fields)
        rec = np.zeros(int(n_fields), dtype=GRIB_ENCODE_DTYPE)
        rec["ddiv"], rec["nbits"] = ddiv, nbits
        return rec

    def layout(self, n_points, n_fields):
        """(byte offset of every field's slot, total bytes): a slot is align4(ceil(n_points / 8)) bitmap bytes and
        align4(ceil(n_points * nbits / 8)) stream bytes, slots back to back in field order."""
        n_points = int(n_points)
        if n_points < 0 or n_points >= 2 ** 31:
            raise ValueError("n_points must be within [0, 2^31)")
        nbits, _ = self._per_field(n_fields)
        sizes = np.array([align4((n_points + 7) // 8) + align4((n_points * int(w) + 7) // 8) for w in nbits], dtype=np.uint64)
        offs = np.zeros(int(n_fields), dtype=np.uint64)
        if offs.size:
            offs[1:] = np.cumsum(sizes)[:-1]
        return offs, int(sizes.sum())

    def encode(self, values):
        """values: float64, (..., n_points) -- every leading index is one field.  Returns a `GribField` of that shape
        over a fresh buffer in the layout of `layout`, `bitmaps` set."""
        v = np.ascontiguousarray(values, dtype=np.float64)
        if v.ndim < 1:
            raise ValueError("encode takes at least one axis of points")
        shape, n = v.shape, int(v.shape[-1])
        v = v.reshape(-1, n)
        nf = v.shape[0]
        nbits, ddiv = self._per_field(nf)
        offs, total = self.layout(n, nf)
        buf = np.zeros(total, dtype=np.uint8)
        rows = np.zeros(nf, dtype=GRIB_ROW_DTYPE)
        bitmaps = np.zeros(nf, dtype=GRIB_BITMAP_DTYPE)
        bm_bytes = align4((n + 7) // 8)
        for b in range(nf):
            w, dd, off = int(nbits[b]), float(ddiv[b]), int(offs[b])
            with np.errstate(over="ignore", invalid="ignore"):
                t = v[b] * dd
                present = np.isfinite(v[b]) & (np.abs(t) <= _FLT_MAX)
            nv = int(present.sum())
            buf[off:off + (n + 7) // 8] = np.packbits(present)
            ref, E, width = 0.0, 0, 0
            if nv:
                tp = t[present]
                tmin, tmax = float(tp.min()), float(tp.max())
                R = np.float32(tmin)
                if float(R) > tmin:
                    R = np.nextafter(R, np.float32(-np.inf))
                ref = float(R) + 0.0
                rng = tmax - ref
                if rng != 0.0:
                    m, e = np.frexp(rng)
                    E = int(e) - w if float(np.ldexp(m, w)) <= float(2 ** w - 1) else int(e) - w + 1
                    E = max(E, -1022)
                    width = w
                    q = np.rint(np.ldexp(tp - ref, -E)).astype(np.uint64)
                    bits = ((q[:, None] >> np.arange(w - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
                    packed = np.packbits(bits.ravel())
                    buf[off + bm_bytes:off + bm_bytes + packed.size] = packed
            rows[b] = (off + bm_bytes, ref, float(np.ldexp(1.0, E)), dd, width, 0)
            bitmaps[b] = (GRIB_NO_BITMAP if nv == n else off, nv)
        if self.codec is not None:
            return self._encode_coded(buf, rows, bitmaps, shape, n)
        return GribField(buf, rows, shape, n, bitmaps=bitmaps)

    def _encode_coded(self, buf, rows, bitmaps, shape, n):
        """The simple-packed fields of `encode` with their integers coded as CCSDS or complex-packed streams.  The buffer:
        every field's bitmap slot (align4(ceil(n_points / 8)) bytes, written whether the field has missing points or not)
        in field order, then the streams back to back in field order, each at a 4-byte-aligned offset.  A field of width 0
        has no stream (block_size 0; order GRIB_CPX_SIMPLE).  The rows keep the widths of the integers."""
        nf, bm_bytes = rows.size, align4((n + 7) // 8)
        rec = self.coded_records(nf, bitmaps["n_values"], rows["nbits"])
        streams, at = [], nf * bm_bytes
        head = np.zeros(at, dtype=np.uint8)
        rows, bitmaps = rows.copy(), bitmaps.copy()
        for b in range(nf):
            w, nv, off = int(rows["nbits"][b]), int(bitmaps["n_values"][b]), int(rows["byte_off"][b])
            head[b * bm_bytes:(b + 1) * bm_bytes] = buf[off - bm_bytes:off]
            if int(bitmaps["bitmap_off"][b]) != GRIB_NO_BITMAP:
                bitmaps["bitmap_off"][b] = b * bm_bytes
            q = _unpack_bits(bytes(memoryview(buf)[off:off + (nv * w + 7) // 8]), w, nv).astype(np.uint32)
            # the record of the stream written (marked simple-packed, without bytes, at width 0)
            st, rec[b] = self.codec.encode(q, rec[b])
            rec["byte_off"][b] = rows["byte_off"][b] = at
            rec["byte_len"][b] = st.size
            streams.append(np.concatenate([st, np.zeros(align4(st.size) - st.size, dtype=np.uint8)]))
            at += align4(st.size)
        return GribField(np.concatenate([head] + streams), rows, shape, n, bitmaps=bitmaps, **{self.codec.name: rec})

    def __repr__(self):
        return f"<GribEncode widths {sorted(set(self.nbits.tolist()))}, D {sorted(set(self.decimal_scale.tolist()))}>"


# ECMWF table 128 entries that turn up in climate work -> (cfgrib variable name, long name, units)
_TABLE_128 = {
    31: ("siconc", "Sea ice area fraction", "(0 - 1)"), 34: ("sst", "Sea surface temperature", "K"),
    129: ("z", "Geopotential", "m**2 s**-2"), 130: ("t", "Temperature", "K"),
    131: ("u", "U component of wind", "m s**-1"), 132: ("v", "V component of wind", "m s**-1"),
    133: ("q", "Specific humidity", "kg kg**-1"), 134: ("sp", "Surface pressure", "Pa"),
    151: ("msl", "Mean sea level pressure", "Pa"), 164: ("tcc", "Total cloud cover", "(0 - 1)"),
    165: ("u10", "10 metre U wind component", "m s**-1"), 166: ("v10", "10 metre V wind component", "m s**-1"),
    167: ("t2m", "2 metre temperature", "K"), 168: ("d2m", "2 metre dewpoint temperature", "K"),
    172: ("lsm", "Land-sea mask", "(0 - 1)"), 228: ("tp", "Total precipitation", "m"),
}
_LEVEL_DIMS = {100: "isobaricInhPa", 109: "hybrid", 105: "heightAboveGround", 111: "depthBelowLand",
               160: "depthBelowSea"}


# GRIB-2 (discipline, category, number) -> (cfgrib variable name, long name, units); WMO code table 4.2
_TABLE_G2 = {
    (0, 0, 0): ("t", "Temperature", "K"), (0, 0, 6): ("d", "Dew point temperature", "K"),
    (0, 1, 0): ("q", "Specific humidity", "kg kg**-1"), (0, 1, 8): ("tp", "Total precipitation", "kg m**-2"),
    (0, 2, 2): ("u", "U component of wind", "m s**-1"), (0, 2, 3): ("v", "V component of wind", "m s**-1"),
    (0, 3, 0): ("sp", "Pressure", "Pa"), (0, 3, 1): ("msl", "Pressure reduced to MSL", "Pa"),
    (0, 3, 4): ("z", "Geopotential", "m**2 s**-2"), (0, 3, 5): ("gh", "Geopotential height", "gpm"),
    (0, 6, 1): ("tcc", "Total cloud cover", "%"), (2, 0, 0): ("lsm", "Land-sea mask", "(0 - 1)"),
    (10, 3, 0): ("sst", "Sea surface temperature", "K"), (10, 2, 0): ("siconc", "Sea ice area fraction", "(0 - 1)"),
}
# near-surface fields get cfgrib's own names: (name above, height above ground in m) -> name
_G2_NEAR_SURFACE = {("t", 2.0): "t2m", ("d", 2.0): "d2m", ("u", 10.0): "u10", ("v", 10.0): "v10"}
_LEVEL_DIMS_G2 = {100: "isobaricInhPa", 105: "hybrid", 103: "heightAboveGround", 106: "depthBelowLandLayer",
                  160: "depthBelowSea"}


def _uint(b):
    return int.from_bytes(b, "big")


def _sint(b):
    """GRIB-1 signed integers are sign-and-magnitude."""
    v = _uint(b)
    top = 1 << (8 * len(b) - 1)
    return -(v & (top - 1)) if v & top else v


def _ibm_float(b):
    """IBM System/360 single precision: sign, 7-bit excess-64 exponent of 16, 24-bit fraction."""
    v = _uint(b)
    sign = -1.0 if v >> 31 else 1.0
    return sign * (v & 0xFFFFFF) / float(1 << 24) * 16.0 ** (((v >> 24) & 0x7F) - 64)


def gaussian_latitudes(n):
    """The 2N Gaussian latitudes, north to south: arcsin of the roots of the Legendre polynomial of degree 2N."""
    x, _ = np.polynomial.legendre.leggauss(2 * n)
    return np.degrees(np.arcsin(x))[::-1]


def _unpack_bits(raw, nbits, count):
    """`count` unsigned big-endian integers of `nbits` bits each from the byte string `raw`."""
    if nbits == 0:
        return np.zeros(count, dtype=np.float64)
    if nbits in (8, 16, 32):
        return np.frombuffer(raw, dtype={8: ">u1", 16: ">u2", 32: ">u4"}[nbits], count=count).astype(np.float64)
    if nbits == 24:
        b = np.frombuffer(raw, dtype=np.uint8, count=3 * count).reshape(count, 3).astype(np.uint32)
        return ((b[:, 0] << 16) | (b[:, 1] << 8) | b[:, 2]).astype(np.float64)
    bits = np.unpackbits(np.frombuffer(raw, dtype=np.uint8))[:nbits * count].reshape(count, nbits)
    return bits.astype(np.uint64) @ (np.uint64(1) << np.arange(nbits - 1, -1, -1, dtype=np.uint64))


def _decode_rule(buf, rule, count, bitmap=None, coded=None):
    """The float64 values of one message from its rule (file offset of the packed values, R, 2^E, 10^D, bit width):
    the statement the message classes evaluate, on the message's own bytes only.  bitmap: None, or (file offset of the
    bitmap's bytes, values in the stream) -- the values go to the points whose bit is set, the others are NaN.
    coded: None, or the one-row `CodedRows` of a CCSDS- or complex-packed message -- its integers come out of the coded
    stream (missing values coded inside it become NaN; such a message has no bitmap here)."""
    off, ref, scale, ddiv, nbits = rule
    n = count if bitmap is None else bitmap[1]
    if coded is not None:
        rec, mvm = coded.recs[0], 0 if coded.missing is None else int(coded.missing[0])
        if int(rec["n_values"]) != n:
            raise ValueError(f"{coded.codec.stream} of {int(rec['n_values'])} values for {n} points")
        q, there = coded.codec.decode(buf, rec, mvm)
        if there is not None:
            values = np.full(n, np.nan)
            values[there] = (ref + q.astype(np.float64) * scale) / ddiv
            return values
        q = q.astype(np.float64)
    else:
        q = _unpack_bits(bytes(memoryview(buf)[off:off + (n * nbits + 7) // 8]), nbits, n)
    packed = (ref + q * scale) / ddiv
    if bitmap is None:
        return packed
    present = np.unpackbits(np.frombuffer(bytes(memoryview(buf)[bitmap[0]:bitmap[0] + (count + 7) // 8]),
                                          dtype=np.uint8))[:count].astype(bool)
    values = np.full(count, np.nan)
    values[present] = packed
    return values


_POPCOUNT8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def _count_bits(raw, n):
    """Set bits among the first n of the byte string `raw` (MSB first), without unpacking them."""
    if len(raw) * 8 < n:
        raise ValueError(f"GRIB bitmap of {len(raw)} bytes for {n} grid points")
    b = np.frombuffer(bytes(raw[:(n + 7) // 8]), dtype=np.uint8)
    total = int(_POPCOUNT8[b].sum(dtype=np.int64))
    if n % 8:
        total -= int(_POPCOUNT8[int(b[-1]) & (0xFF >> (n % 8))])
    return total


class _Field:
    """Grid and coordinates shared by the fields of both editions.  `values` is None for a message read with
    keep_raw (only its `raw_rule` was recorded, and with keep_bitmaps the `raw_bitmap` of a message that has one: file
    offset of the bitmap's bytes and values in the stream); `field_values` decodes it on demand."""
    raw_bitmap = None
    raw_aec = None        # the GRIB_AEC_DTYPE fields of a CCSDS-packed message (edition 2, template 5.42)
    raw_cpx = None        # the GRIB_CPX_DTYPE fields of a complex-packed message (edition 2, templates 5.2 / 5.3)
    raw_mvm = 0           # ... its missing value management (1 or 2: missing values are codes inside the groups)

    def field_values(self, buf):
        if self.values is not None:
            return self.values
        coded = CodedRows.of(1, None if self.raw_aec is None else np.array(self.raw_aec, dtype=GRIB_AEC_DTYPE),
                             None if self.raw_cpx is None else np.array(self.raw_cpx, dtype=GRIB_CPX_DTYPE),
                             None if self.raw_cpx is None else [self.raw_mvm])
        return _decode_rule(buf, self.raw_rule, self.npoints, self.raw_bitmap, coded)

    def _set_grid(self, rep, ni, nj, la1, lo1, la2, lo2, n_gauss, scan, pl, tol):
        if scan & 0x20:
            raise GribUnsupported("scanning mode with consecutive points along j")
        if scan & 0x10:
            raise GribUnsupported("scanning mode with alternating row direction")
        self.rep, self.nj = rep, nj
        self.pl = pl
        if pl is not None and pl.size != nj:
            raise ValueError("reduced grid: the list of points per row is shorter than Nj")
        if rep == 4:
            lat = gaussian_latitudes(n_gauss)
            if lat.size != nj:                       # a band of a Gaussian grid: rows from La1 to La2
                first = int(np.abs(lat - max(la1, la2)).argmin())
                lat = lat[first:first + nj]
            if abs(lat[0] - max(la1, la2)) > tol:
                raise ValueError(f"Gaussian latitude {lat[0]:.4f} does not match the file's first row {max(la1, la2)}")
            if scan & 0x40:
                lat = lat[::-1]
        else:
            lat = np.linspace(la1, la2, nj)
        self.lat = lat
        if pl is None:
            if lo2 < lo1:
                lo2 += 360.0
            lon = np.linspace(lo1, lo2, ni)
            self.lon = lon[::-1] if scan & 0x80 else lon
            self.ni, self.npoints = ni, ni * nj
        else:
            if scan & 0x80:
                raise GribUnsupported("reduced grid scanned east to west")
            self.lon = None
            self.ni, self.npoints = None, int(pl.sum())

    def point_coordinates(self):
        """latitude / longitude of every point of a reduced grid, in the order of the values: PL[j] points per row,
        evenly spaced from 0 east (the full circle divided by PL[j])."""
        lat = np.repeat(self.lat, self.pl)
        lon = np.concatenate([np.arange(p) * (360.0 / p) for p in self.pl])
        return lat, lon

    @property
    def grid_key(self):
        return (self.rep, self.nj, self.ni, None if self.pl is None else self.pl.tobytes(), self.lat.tobytes())


class _Message(_Field):
    """One decoded GRIB-1 message: metadata + values in the file's scanning order (NaN where the bitmap says so)."""
    edition = 1

    def __init__(self, buf, start, keep_raw=False, keep_bitmaps=False):
        if buf[start:start + 4] != b"GRIB":
            raise ValueError("not a GRIB message")
        if buf[start + 7] != 1:
            raise GribUnsupported(f"GRIB edition {buf[start + 7]}")
        self.length = _uint(buf[start + 4:start + 7])
        if buf[start + self.length - 4:start + self.length] != b"7777":
            raise ValueError("GRIB message does not end in 7777 (truncated file?)")
        pos = start + 8
        pds = buf[pos:pos + _uint(buf[pos:pos + 3])]
        pos += len(pds)
        self.table, self.centre, self.param = pds[3], pds[4], pds[8]
        self.level_type = pds[9]
        self.level = _uint(pds[10:12]) if self.level_type in (100, 105, 109, 111, 160, 103, 107, 113, 115, 117, 119, 125) \
            else pds[10]
        century = pds[24] if len(pds) > 24 else 21
        year = (century - 1) * 100 + pds[12]
        self.time = np.datetime64(f"{year:04d}-{max(pds[13], 1):02d}-{max(pds[14], 1):02d}T{pds[15]:02d}:{pds[16]:02d}")
        unit_hours = {0: 1 / 60.0, 1: 1.0, 2: 24.0, 10: 3.0, 11: 6.0, 12: 12.0, 254: 1 / 3600.0}.get(pds[17])
        tri = pds[20]
        p1, p2 = pds[18], pds[19]
        step = {0: p1, 1: 0, 10: (p1 << 8) | p2}.get(tri, p2)
        self.step_hours = float(step) * unit_hours if unit_hours is not None else 0.0
        self.decimal_scale = _sint(pds[26:28]) if len(pds) >= 28 else 0
        has_gds, has_bms = bool(pds[7] & 0x80), bool(pds[7] & 0x40)
        if not has_gds:
            raise GribUnsupported("GRIB-1 message without a grid description section (predefined grid numbers)")
        gds = buf[pos:pos + _uint(buf[pos:pos + 3])]
        pos += len(gds)
        self._grid(gds)
        bitmap = None
        if has_bms:
            bms = buf[pos:pos + _uint(buf[pos:pos + 3])]
            pos += len(bms)
            if _uint(bms[4:6]) != 0:
                raise GribUnsupported("predefined GRIB-1 bitmaps")
            if keep_raw and keep_bitmaps:
                # kept raw with its bitmap: where the bitmap lies and how many bits it sets, nothing unpacked
                self._keep_bitmapped(buf, pos, (pos - len(bms) + 6, _count_bits(bms[6:], self.npoints)))
                return
            bitmap = np.unpackbits(np.frombuffer(bms[6:], dtype=np.uint8))[:self.npoints].astype(bool)
        bds = buf[pos:pos + _uint(buf[pos:pos + 3])]
        flag = bds[3]
        if flag & 0x80:
            raise GribUnsupported("spherical harmonic coefficients")
        if flag & 0x40:
            raise GribUnsupported("second-order (complex) packing")
        if flag & 0x10:
            raise GribUnsupported("GRIB-1 binary data section with additional flags (matrix of values)")
        scale = 2.0 ** _sint(bds[4:6])
        ref = _ibm_float(bds[6:10])
        nbits = bds[10]
        count = self.npoints if bitmap is None else int(bitmap.sum())
        avail = ((len(bds) - 11) * 8 - (flag & 0x0F)) // nbits if nbits else count
        if avail < count:
            raise ValueError(f"GRIB data section holds {avail} values, the grid needs {count}")
        # where the packed values lie in the file and how they decode (open_grib(decode=False)); None with a bitmap
        self.raw_rule = None if bitmap is not None else (pos + 11, ref, scale, 10.0 ** self.decimal_scale, nbits)
        if keep_raw and bitmap is None:
            self.values = None               # nothing is unpacked: the rule is all a raw-kept variable needs
            return
        x = _unpack_bits(bds[11:], nbits, count)
        packed = (ref + x * scale) / 10.0 ** self.decimal_scale
        if bitmap is None:
            self.values = packed
        else:
            self.values = np.full(self.npoints, np.nan)
            self.values[bitmap] = packed

    def _keep_bitmapped(self, buf, pos, raw_bitmap):
        """The binary data section at `pos` of a message whose bitmap is `raw_bitmap`: the rule, no value unpacked."""
        bds = buf[pos:pos + _uint(buf[pos:pos + 3])]
        flag = bds[3]
        if flag & 0x80:
            raise GribUnsupported("spherical harmonic coefficients")
        if flag & 0x40:
            raise GribUnsupported("second-order (complex) packing")
        if flag & 0x10:
            raise GribUnsupported("GRIB-1 binary data section with additional flags (matrix of values)")
        nbits, count = bds[10], raw_bitmap[1]
        avail = ((len(bds) - 11) * 8 - (flag & 0x0F)) // nbits if nbits else count
        if avail < count:
            raise ValueError(f"GRIB data section holds {avail} values, the grid needs {count}")
        self.raw_rule = (pos + 11, _ibm_float(bds[6:10]), 2.0 ** _sint(bds[4:6]), 10.0 ** self.decimal_scale, nbits)
        self.raw_bitmap = raw_bitmap
        self.values = None

    def _grid(self, gds):
        nv, pvpl, rep = gds[3], gds[4], gds[5]
        if rep not in (0, 4):
            raise GribUnsupported(f"GRIB-1 data representation type {rep} (lon/lat = 0 and Gaussian = 4 are decoded)")
        ni, nj = _uint(gds[6:8]), _uint(gds[8:10])
        la1, lo1 = _sint(gds[10:13]) / 1000.0, _sint(gds[13:16]) / 1000.0
        la2, lo2 = _sint(gds[17:20]) / 1000.0, _sint(gds[20:23]) / 1000.0
        pl = None
        if pvpl != 255 and ni == 0xFFFF:
            off = pvpl - 1 + 4 * nv
            pl = np.frombuffer(bytes(gds[off:off + 2 * nj]), dtype=">u2").astype(np.int64)
        self._set_grid(rep, ni, nj, la1, lo1, la2, lo2, _uint(gds[25:27]), gds[27], pl, tol=2e-3)


def _ccsds_template(sec5):
    """Data representation template 5.42 (CCSDS packing) from section 5: (R, 2^E, D, bits per value, ccsdsFlags,
    ccsdsBlockSize, ccsdsRsi).  Octets 12 - 20 are those of template 5.0 (R, E, D, bits per value; 21 = type of the
    original values), 22 = ccsdsFlags, 23 = ccsdsBlockSize, 24 - 25 = ccsdsRsi -- taken from the WMO table; no file
    written by ecCodes was at hand to pin them.  A flag the decoder does not take raises GribUnsupported naming it."""
    if len(sec5) < 25:
        raise GribUnsupported(f"GRIB-2 data representation template 5.42 (CCSDS packing) in a section 5 of {len(sec5)} "
                              "octets: the template takes 25")
    ref = float(np.frombuffer(bytes(sec5[11:15]), dtype=">f4")[0])
    scale, decimal, nbits = 2.0 ** _sint(sec5[15:17]), _sint(sec5[17:19]), sec5[19]
    flags, block, rsi = sec5[21], sec5[22], _uint(sec5[23:25])
    for bit, what in _AEC_REFUSED.items():
        if flags & bit:
            raise GribUnsupported(f"CCSDS packing with ccsdsFlags {what}")
    if flags & ~0x3F:
        raise GribUnsupported(f"CCSDS packing with ccsdsFlags {flags:#x}: bits outside the flag table")
    if nbits > 32:
        raise GribUnsupported(f"CCSDS packing of {nbits} bits per value")
    if nbits and (block not in (8, 16, 32, 64) or not 1 <= rsi <= 4096):
        raise GribUnsupported(f"CCSDS packing with block size {block} and reference sample interval {rsi} "
                              "(8 / 16 / 32 / 64 and 1..4096 are decoded)")
    return ref, scale, decimal, nbits, flags, block, rsi


def _complex_template(sec5, drt, n_values, cpx_missing=False):
    """Data representation templates 5.2 (complex packing) and 5.3 (with spatial differencing) from section 5: (R, 2^E, D,
    width of the group references, then the fields of GRIB_CPX_DTYPE from n_groups to n_oct).  Octets 12 - 20 are those
    of template 5.0, 21 = type of the original values, 22 = group splitting method, 23 = missing value management,
    24 - 31 the two substitutes, 32 - 35 NG, 36 / 37 reference and bits of the group widths, 38 - 41 / 42 reference and
    increment of the group lengths, 43 - 46 true length of the last group, 47 bits of the scaled group lengths; 5.3:
    48 order of spatial differencing, 49 octets per extra descriptor -- taken from the WMO table; no file written by
    NCEP's tools or ecCodes was at hand to pin them.  What the decoder does not take raises GribUnsupported naming it."""
    what = f"GRIB-2 data representation template 5.{drt} (complex packing" + (" with spatial differencing)" if drt == 3 else ")")
    need = 49 if drt == 3 else 47
    if len(sec5) < need:
        raise GribUnsupported(f"{what} in a section 5 of {len(sec5)} octets: the template takes {need}")
    ref = float(np.frombuffer(bytes(sec5[11:15]), dtype=">f4")[0])
    scale, decimal, nbits = 2.0 ** _sint(sec5[15:17]), _sint(sec5[17:19]), sec5[19]
    mvm = sec5[22]
    if mvm > 2 or (mvm != 0 and not cpx_missing):
        raise GribUnsupported(f"{what} with missing value management {mvm} (missing values coded inside the groups; "
                              "1 and 2 are decoded by open_dataset(..., cpx_missing=True))")
    n_groups, width_ref, width_bits = _uint(sec5[31:35]), sec5[35], sec5[36]
    length_ref, length_inc, length_last, length_bits = _uint(sec5[37:41]), sec5[41], _uint(sec5[42:46]), sec5[46]
    order, n_oct = (sec5[47], sec5[48]) if drt == 3 else (0, 0)
    if order > 2:
        raise GribUnsupported(f"{what} of order {order}: orders 0, 1 and 2 are decoded")
    if order > 0 and not 1 <= n_oct <= 4:
        raise GribUnsupported(f"{what} with {n_oct} octets per extra descriptor: 1..4 are decoded")
    if nbits > 32:
        raise GribUnsupported(f"{what} with group references of {nbits} bits")
    if width_bits > 32 or length_bits > 32:
        raise GribUnsupported(f"{what} with group widths stored in {width_bits} bits and group lengths in {length_bits}: "
                              "at most 32 are decoded")
    if n_values > 0 and n_groups == 0:
        raise GribUnsupported(f"{what} of {n_values} values in no group")
    if 0 < n_values <= order:
        raise GribUnsupported(f"{what} of order {order} on {n_values} values")
    if n_values >= 2 ** 31:
        raise GribUnsupported(f"{what} of {n_values} values: fewer than 2^31 are decoded")
    return ref, scale, decimal, nbits, (n_groups, nbits, width_ref, width_bits, length_ref, length_inc, length_last, length_bits,
                                        order, n_oct if order else 0), mvm


class _Field2(_Field):
    """One field of a GRIB-2 message (a message may repeat sections 2 - 7 / 3 - 7 / 4 - 7 for further fields)."""
    edition = 2

    def __init__(self, discipline, sec1, sec3, sec4, sec5, sec6, sec7, prev_bitmap, data_pos=None, keep_raw=False,
                 bitmap_pos=None, prev_raw_bitmap=None, cpx_missing=False):
        """data_pos: file offset of section 7 (its packed values follow 5 octets later).  bitmap_pos: file offset of
        section 6 when bitmapped fields are kept raw too (its bits follow 6 octets later); prev_raw_bitmap: the
        `raw_bitmap` of the field before, for a field that reuses its bitmap."""
        self.centre = _uint(sec1[5:7])
        self.time = np.datetime64(f"{_uint(sec1[12:14]):04d}-{max(sec1[14], 1):02d}-{max(sec1[15], 1):02d}"
                                  f"T{sec1[16]:02d}:{sec1[17]:02d}:{sec1[18]:02d}")
        # --- section 3: grid
        if sec3[5] != 0:
            raise GribUnsupported("GRIB-2 grid defined by reference to a predefined grid")
        n_points, n_oct, template = _uint(sec3[6:10]), sec3[10], _uint(sec3[12:14])
        if template not in (0, 40):
            raise GribUnsupported(f"GRIB-2 grid definition template 3.{template} (3.0 lon/lat and 3.40 Gaussian are decoded)")
        ni, nj = _uint(sec3[30:34]), _uint(sec3[34:38])
        basic, sub = _uint(sec3[38:42]), _uint(sec3[42:46])
        unit = 1e-6 if basic in (0, 0xFFFFFFFF) or sub in (0, 0xFFFFFFFF) else basic / float(sub)
        la1, lo1 = _sint(sec3[46:50]) * unit, _sint(sec3[50:54]) * unit
        la2, lo2 = _sint(sec3[55:59]) * unit, _sint(sec3[59:63]) * unit
        pl = None
        if n_oct:
            pl = np.array([_uint(sec3[72 + i * n_oct:72 + (i + 1) * n_oct]) for i in range(nj)], dtype=np.int64)
            ni = None
        elif ni == 0xFFFFFFFF:
            raise ValueError("GRIB-2 reduced grid without its list of points per row")
        self._set_grid(4 if template == 40 else 0, ni, nj, la1, lo1, la2, lo2, _uint(sec3[67:71]), sec3[71], pl, tol=1e-4)
        if self.npoints != n_points:
            raise ValueError(f"GRIB-2 grid of {self.npoints} points in a section that announces {n_points}")
        # --- section 4: product
        pdt = _uint(sec4[7:9])
        if pdt not in (0, 1, 8, 11):
            raise GribUnsupported(f"GRIB-2 product definition template 4.{pdt}")
        self.table = f"g2:{discipline}"
        self.param = (discipline, sec4[9], sec4[10])
        unit_hours = {0: 1 / 60.0, 1: 1.0, 2: 24.0, 10: 3.0, 11: 6.0, 12: 12.0, 13: 1 / 3600.0}.get(sec4[17])
        self.step_hours = float(_uint(sec4[18:22])) * unit_hours if unit_hours is not None else 0.0
        self.level_type = sec4[22]
        factor, scaled = sec4[23], _uint(sec4[24:28])
        level = 0.0 if scaled == 0xFFFFFFFF or factor == 0xFF else _sint(sec4[24:28]) * 10.0 ** -_sint(sec4[23:24])
        self.level = level / 100.0 if self.level_type == 100 else level          # Pa -> hPa, as cfgrib's isobaricInhPa
        # --- section 5 / 6 / 7: packed values
        n_coded, drt = _uint(sec5[5:9]), _uint(sec5[9:11])
        if drt not in (0, 2, 3, 42):
            names = {40: "JPEG 2000 packing", 41: "PNG packing", 50: "spherical harmonics", 51: "spherical harmonics"}
            raise GribUnsupported(f"GRIB-2 data representation template 5.{drt} ({names.get(drt, 'not simple packing')})")
        aec = None         # CCSDS: (ccsdsFlags, ccsdsBlockSize, ccsdsRsi); a constant field (0 bits) has no stream
        cpx = None         # complex packing: GRIB_CPX_DTYPE's fields from n_groups to n_oct
        mvm = 0            # ... its missing value management (octet 23): 1 or 2 with cpx_missing
        if drt == 42:
            ref, scale, decimal, nbits, *aec = _ccsds_template(sec5)
            aec = tuple(aec) if nbits else None
        elif drt in (2, 3):
            ref, scale, decimal, nbits, cpx, mvm = _complex_template(sec5, drt, n_coded, cpx_missing)
        else:
            ref = float(np.frombuffer(bytes(sec5[11:15]), dtype=">f4")[0])
            scale, decimal, nbits = 2.0 ** _sint(sec5[15:17]), _sint(sec5[17:19]), sec5[19]
        if aec is not None and data_pos is not None:
            self.raw_aec = (data_pos + 5, len(sec7) - 5, n_coded, nbits, aec[1], aec[2], aec[0], 0)
        if cpx is not None and data_pos is not None:
            self.raw_cpx = (data_pos + 5, len(sec7) - 5, n_coded) + cpx + (0,)
            self.raw_mvm = mvm
        indicator = sec6[5] if sec6 is not None else 255
        # a bitmap and codes inside the groups on one message: decoded on the host, the bitmap first, the codes inside it
        both = mvm != 0 and indicator in (0, 254)
        if keep_raw and bitmap_pos is not None and data_pos is not None and indicator in (0, 254) and not both:
            # kept raw with its bitmap: where the bitmap lies and how many bits it sets, nothing unpacked
            if indicator == 254 and prev_raw_bitmap is None:
                raise ValueError("GRIB-2 field refers to a previous bitmap that does not exist")
            self.raw_bitmap = (bitmap_pos + 6, _count_bits(sec6[6:], self.npoints)) if indicator == 0 else prev_raw_bitmap
            self.bitmap = None
            if n_coded != self.raw_bitmap[1]:
                raise ValueError(f"GRIB-2 data section codes {n_coded} values, grid and bitmap need {self.raw_bitmap[1]}")
            if nbits and aec is None and cpx is None and (len(sec7) - 5) * 8 < n_coded * nbits:
                raise ValueError("GRIB-2 data section is shorter than its values")
            self.raw_rule = (data_pos + 5, ref, scale, 10.0 ** decimal, nbits)
            self.values = None
            return
        if indicator == 0:
            self.bitmap = np.unpackbits(np.frombuffer(bytes(sec6[6:]), dtype=np.uint8))[:self.npoints].astype(bool)
        elif indicator == 254:
            if prev_bitmap is None:
                raise ValueError("GRIB-2 field refers to a previous bitmap that does not exist")
            self.bitmap = prev_bitmap
        elif indicator == 255:
            self.bitmap = None
        else:
            raise GribUnsupported("predefined GRIB-2 bitmaps")
        count = self.npoints if self.bitmap is None else int(self.bitmap.sum())
        if n_coded != count:
            raise ValueError(f"GRIB-2 data section codes {n_coded} values, grid and bitmap need {count}")
        if nbits and aec is None and cpx is None and (len(sec7) - 5) * 8 < count * nbits:
            raise ValueError("GRIB-2 data section is shorter than its values")
        self.raw_rule = None if (self.bitmap is not None or data_pos is None) else \
            (data_pos + 5, ref, scale, 10.0 ** decimal, nbits)
        if keep_raw and self.raw_rule is not None:
            self.values = None
            return
        if cpx is not None and mvm != 0:      # codes inside the groups: the present positions, then the bitmap around them
            rec = np.array((0, len(sec7) - 5, count) + cpx + (0,), dtype=GRIB_CPX_DTYPE)
            q, there = cpx_decode_mv(bytes(sec7[5:]), rec, mvm)
            coded = np.full(count, np.nan)
            coded[there] = (ref + q.astype(np.float64) * scale) / 10.0 ** decimal
            if self.bitmap is None:
                self.values = coded
            else:
                self.values = np.full(self.npoints, np.nan)
                self.values[self.bitmap] = coded
            return
        if cpx is not None:       # the message's own groups, decoded on the host
            q = cpx_decode(bytes(sec7[5:]), np.array((0, len(sec7) - 5, count) + cpx + (0,), dtype=GRIB_CPX_DTYPE)).astype(np.float64)
        elif aec is not None:     # the message's own stream, decoded on the host
            q = aec_decode(bytes(sec7[5:]), np.array((0, len(sec7) - 5, count, nbits, aec[1], aec[2], aec[0], 0),
                                                     dtype=GRIB_AEC_DTYPE)).astype(np.float64)
        else:
            q = _unpack_bits(bytes(sec7[5:]), nbits, count)
        packed = (ref + q * scale) / 10.0 ** decimal
        if self.bitmap is None:
            self.values = packed
        else:
            self.values = np.full(self.npoints, np.nan)
            self.values[self.bitmap] = packed


def _fields_of_message2(buf, start, keep_raw=False, keep_bitmaps=False, cpx_missing=False):
    """The fields of the GRIB-2 message at `start`, and the message's length."""
    discipline, total = buf[start + 6], _uint(buf[start + 8:start + 16])
    if buf[start + total - 4:start + total] != b"7777":
        raise ValueError("GRIB message does not end in 7777 (truncated file?)")
    pos, end = start + 16, start + total - 4
    sec, sec6_pos = {}, None
    fields, bitmap, raw_bitmap = [], None, None
    while pos < end:
        length, number = _uint(buf[pos:pos + 4]), buf[pos + 4]
        if length < 5 or pos + length > end:
            raise ValueError("GRIB-2 section runs past the end of its message")
        sec[number] = buf[pos:pos + length]
        if number == 3:                       # a new grid: sections 4 - 7 follow again
            sec.pop(6, None)
        if number == 6 and sec[6][5] == 0:    # a bitmap of its own: a later "same as before" (254) means this one
            sec6_pos = pos
        if number == 7:
            for need in (1, 3, 4, 5):
                if need not in sec:
                    raise ValueError(f"GRIB-2 message without section {need}")
            f = _Field2(discipline, sec[1], sec[3], sec[4], sec[5], sec.get(6), sec[7], bitmap, data_pos=pos, keep_raw=keep_raw,
                        bitmap_pos=sec6_pos if keep_bitmaps else None, prev_raw_bitmap=raw_bitmap, cpx_missing=cpx_missing)
            bitmap, raw_bitmap = f.bitmap, f.raw_bitmap
            fields.append(f)
        pos += length
    return fields, total


def read_messages(path):
    with open(path, "rb") as f:
        return _messages_of(f.read(), path)


def _messages_of(buf, path, keep_raw=False, keep_bitmaps=False, cpx_missing=False):
    """The messages of a file's bytes.  keep_raw: those without a bitmap are not unpacked (`values` is None, `raw_rule`
    says how to); with keep_bitmaps neither are those with one (`raw_bitmap` says where it lies)."""
    out, pos = [], 0
    while True:
        pos = buf.find(b"GRIB", pos)
        if pos < 0:
            break
        edition = buf[pos + 7] if pos + 8 <= len(buf) else 0
        if edition == 2:
            fields, length = _fields_of_message2(buf, pos, keep_raw, keep_bitmaps, cpx_missing)
            out.extend(fields)
            pos += length
            continue
        if edition != 1:
            raise GribUnsupported(f"GRIB edition {edition}")
        m = _Message(buf, pos, keep_raw, keep_bitmaps)
        out.append(m)
        pos += m.length
    if not out:
        raise ValueError(f"{path} holds no GRIB message")
    return out


def open_grib(path, decode=True, bitmaps=False, cpx_missing=False):
    """Dataset of the fields of a GRIB file, one variable per parameter.  All messages must share one grid.
    decode=False keeps every variable whose (time, level) slots are all filled by messages without a bitmap as a
    `GribField` -- the file's bytes and one decode rule per field, which `Regridder(packed=True)` ships to the GPU as
    they are; `np.asarray` of it is the decoded float32 array.  Any other variable is decoded as with decode=True.
    bitmaps=True (with decode=False) keeps messages with a bitmap section raw as well (edition 1 section 3; edition 2
    section 6 with its own bitmap or the previous field's): the reader records where the bitmap lies and how many bits
    it sets, `GribField.bitmaps` holds one record per field, and a variable may mix messages with and without one.
    CCSDS-packed messages (edition 2, template 5.42) are decoded on the host with decode=True and kept raw like the
    others with decode=False: `GribField.ccsds` holds one record per field, simple-packed fields may stand among them.
    Complex-packed messages (templates 5.2 / 5.3) likewise: `GribField.cpx` holds one record per field, simple-packed
    fields may stand among them; a variable that mixes CCSDS-packed and complex-packed messages is decoded.
    cpx_missing=True reads complex-packed messages whose missing value management (section 5's octet 23) is 1 or 2 --
    missing values coded inside the groups, what wgrib2 writes for undefined points -- instead of refusing them: decoded
    on the host with decode=True (smm_grib_cpx_decode_host_mv; a section-6 bitmap on the same message is honoured: the
    bitmap first, the codes inside it), kept raw with decode=False -- `GribField.cpx_missing` holds the octet per field.
    A variable with a message that has both a bitmap and such codes is decoded."""
    with open(path, "rb") as f:
        file_bytes = f.read()
    msgs = _messages_of(file_bytes, path, keep_raw=not decode, keep_bitmaps=bool(bitmaps) and not decode,
                        cpx_missing=bool(cpx_missing))
    shared = np.frombuffer(file_bytes, dtype=np.uint8) if not decode else None
    if len({m.grid_key for m in msgs}) != 1:
        raise GribUnsupported("GRIB file with fields on several grids")
    g = msgs[0]
    ds = Dataset(attrs={"GRIB_edition": int(g.edition), "GRIB_centre": {98: "ecmf"}.get(g.centre, str(g.centre)),
                        "Conventions": "CF-1.7", "institution": "European Centre for Medium-Range Weather Forecasts"
                        if g.centre == 98 else str(g.centre)})
    if g.pl is None:
        hdims, hshape = ("latitude", "longitude"), (g.nj, g.ni)
        coords = {"latitude": DataArray(g.lat, dims=("latitude",), attrs={"units": "degrees_north",
                                                                         "standard_name": "latitude"}),
                  "longitude": DataArray(g.lon, dims=("longitude",), attrs={"units": "degrees_east",
                                                                           "standard_name": "longitude"})}
        grid_type = "regular_ll" if g.rep == 0 else "regular_gg"
    else:
        lat, lon = g.point_coordinates()
        hdims, hshape = ("values",), (g.npoints,)
        coords = {"latitude": DataArray(lat, dims=("values",), attrs={"units": "degrees_north",
                                                                     "standard_name": "latitude"}),
                  "longitude": DataArray(lon, dims=("values",), attrs={"units": "degrees_east",
                                                                      "standard_name": "longitude"})}
        grid_type = "reduced_gg" if g.rep == 4 else "reduced_ll"
    by_param = {}
    for m in msgs:
        by_param.setdefault((m.table, m.param, m.level_type), []).append(m)
    for (table, param, level_type), group in by_param.items():
        if isinstance(param, tuple):             # edition 2: (discipline, category, number)
            tag = "p" + "_".join(str(v) for v in param)
            name, long_name, units = _TABLE_G2.get(param, (tag, f"parameter {param}", "unknown"))
            heights = {m.level for m in group}
            if level_type == 103 and len(heights) == 1:
                name = _G2_NEAR_SURFACE.get((name, float(next(iter(heights)))), name)
            param_id = param[0] * 1000000 + param[1] * 1000 + param[2]
        else:
            name, long_name, units = _TABLE_128.get(param, (f"p{param}", f"parameter {param}", "unknown")) \
                if table == 128 else (f"p{param}", f"parameter {param} of table {table}", "unknown")
            param_id = int(param)
        if name in ds.data_vars:
            name = f"{name}_{level_type}"
        times = sorted({m.time + np.timedelta64(int(round(m.step_hours * 3600)), "s") for m in group})
        levels = sorted({m.level for m in group})
        slots = [(times.index(m.time + np.timedelta64(int(round(m.step_hours * 3600)), "s")), levels.index(m.level))
                 for m in group]
        rows = np.zeros((len(times), len(levels)), dtype=GRIB_ROW_DTYPE)
        filled = np.zeros((len(times), len(levels)), dtype=bool)
        bms = np.zeros((len(times), len(levels)), dtype=GRIB_BITMAP_DTYPE)
        bms["bitmap_off"], bms["n_values"] = GRIB_NO_BITMAP, g.npoints
        aecs = np.zeros((len(times), len(levels)), dtype=GRIB_AEC_DTYPE)
        cpxs = np.zeros((len(times), len(levels)), dtype=GRIB_CPX_DTYPE)
        cpxs["order"] = GRIB_CPX_SIMPLE
        mvms = np.zeros((len(times), len(levels)), dtype=np.uint8)
        for m, slot in zip(group, slots):
            if m.raw_rule is not None:
                rows[slot] = m.raw_rule + (0,)
                filled[slot] = True
                if m.raw_bitmap is not None:
                    bms[slot] = m.raw_bitmap
                if m.raw_aec is not None:
                    aecs[slot] = m.raw_aec
                if m.raw_cpx is not None:
                    cpxs[slot] = m.raw_cpx
                    mvms[slot] = m.raw_mvm
        # raw: every (time, level) slot filled by a message without a bitmap (a missing slot is NaN, which only a
        # decoded array holds).  Such a variable is never unpacked here; any other is decoded as with decode=True
        raw_ok = not decode and all(m.raw_rule is not None for m in group) and bool(filled.all())
        has_aec, has_cpx = any(m.raw_aec is not None for m in group), any(m.raw_cpx is not None for m in group)
        raw_ok = raw_ok and not (has_aec and has_cpx)      # one kind of coded record per variable
        arr = None
        if not raw_ok:
            arr = np.full((len(times), len(levels)) + hshape, np.nan, dtype=np.float32)
            for m, slot in zip(group, slots):
                arr[slot] = m.field_values(file_bytes).reshape(hshape)
        dims, vcoords = [], dict(coords)
        level_dim = (_LEVEL_DIMS_G2 if isinstance(param, tuple) else _LEVEL_DIMS).get(level_type, "level")
        if len(times) > 1:
            dims.append("time")
            vcoords["time"] = DataArray(np.array(times, dtype="datetime64[s]").astype(np.float64), dims=("time",),
                                        attrs={"units": "seconds since 1970-01-01", "standard_name": "time"})
        elif arr is not None:
            arr = arr[0:1]
        if len(levels) > 1:
            dims.append(level_dim)
            vcoords[level_dim] = DataArray(np.array(levels, dtype=np.float64), dims=(level_dim,))
        shape = tuple(n for n, keep in ((len(times), len(times) > 1), (len(levels), len(levels) > 1)) if keep) + hshape
        if raw_ok:
            if len(times) == 1:
                rows, bms, aecs, cpxs, mvms = rows[0:1], bms[0:1], aecs[0:1], cpxs[0:1], mvms[0:1]
            arr = GribField(shared, rows, shape, int(np.prod(hshape)),
                            bitmaps=bms if any(m.raw_bitmap is not None for m in group) else None,
                            ccsds=aecs if has_aec else None, cpx=cpxs if has_cpx else None,
                            cpx_missing=mvms if mvms.any() else None)
        else:
            arr = arr.reshape(shape)
        ds[name] = DataArray(arr, dims=tuple(dims) + hdims, coords=vcoords, name=name,
                             attrs={"long_name": long_name, "units": units, "GRIB_paramId": param_id,
                                    "GRIB_gridType": grid_type, "GRIB_shortName": name})
    for k, c in coords.items():
        ds.coords[k] = c
    return ds
