"""The synthetic workloads of the tools/*_bench.py tools: every field, stream, row table and record they time is built
here, and nowhere else.  The inputs are the workload -- a changed seed or gap changes every recorded ratio -- so the
seeds are arguments whose defaults are the constants the recorded figures were taken with, and
tests/test_bench_tools.py holds a digest of what every builder returns.  Nothing here needs a device but `padded_upload`.

The gaps.  A message-after-message buffer (`make_streams`, `make_bitmap_streams`, `make_level_streams`) and the coded
input tables put 117 zero bytes in front of every stream, "as sections 0 - 3 would leave": an odd number, so the streams
start at odd byte offsets and the gathers run their unaligned reads.  The `source` of the result tools uses 116, a
multiple of 4, and rounds the buffer itself up to 4 bytes: its streams are aligned and it is uploaded as it is -- there
the input is not what is measured.  The bitmapped layouts put 11 bytes between a bitmap and its values.

Two layouts, on purpose.  `stream_table` lays DISTINCT streams out once and lets the rows point at them in turn (the
coded-input tables, `source`).  `make_streams`, `make_bitmap_streams` and `make_level_streams` write one message per ROW
-- a buffer of rows x stream bytes, no gap behind the last message, and for the bitmapped ones bitmap + 11 bytes + values
per message -- because the host-to-host figures taken with them ship that many bytes; sending them through
`stream_table` would change the bytes and with them every recorded figure, so they keep their own loops.
"""
import numpy as np

DISTINCT = 4        # distinct rows; the batch points at them (or tiles them) in turn
MISSING = 0.3       # share of the cells the bitmapped workloads leave out
NBITS, BLOCK, RSI = 16, 32, 128
FLAGS = 8 | 4 | 2   # AEC_DATA_PREPROCESS | AEC_DATA_MSB | AEC_DATA_3BYTE: ecCodes' ccsdsFlags
GROUP, N_OCT = 32, 3
SEEDS = {"ccsds": 20261019, "cpx": 20261020}     # of the coded-input and the coded-result tools, by codec name


# ------------------------------------------------------------------------------------------------ bits
def pack16(q):
    return q.astype(">u2").tobytes()


def pack12(q):
    """Two 12-bit values in three bytes, big-endian bit order (q.size even)."""
    a, b = q[0::2].astype(np.uint16), q[1::2].astype(np.uint16)
    out = np.empty((a.size, 3), dtype=np.uint8)
    out[:, 0] = a >> 4
    out[:, 1] = ((a & 15) << 4) | (b >> 8)
    out[:, 2] = b & 255
    return out.tobytes()


def _bit_length(v):
    """bit lengths of non-negative integers below 2^53"""
    return np.where(v > 0, np.frexp(np.maximum(v, 1).astype(np.float64))[1], 0).astype(np.int64)


def _pack(values, widths):
    """values[i] in widths[i] bits, big-endian, back to back, padded to an octet"""
    start = np.cumsum(widths) - widths
    bits = np.zeros(int(widths.sum()), dtype=np.uint8)
    for b in range(int(widths.max()) if widths.size else 0):
        sel = np.flatnonzero(widths > b)
        bits[start[sel] + b] = (values[sel] >> (widths[sel] - 1 - b)) & 1
    return np.packbits(bits)


def _sm(v, n_oct):
    return (abs(int(v)) | ((1 << (8 * n_oct - 1)) if v < 0 else 0)).to_bytes(n_oct, "big")


def padded(buf):
    """buf in a zeroed array rounded up to 4 bytes: what the device entries read in words"""
    out = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
    out[:buf.size] = buf
    return out


def padded_upload(buf):
    from smmregrid_amd import to_device
    return to_device(padded(buf))


# ------------------------------------------------------------------------------------------------ the encoders
def encode_ccsds(x, nbits=NBITS, J=BLOCK, rsi=RSI):
    """A CCSDS 121.0-B stream of the unsigned integers x with the preprocessor on, vectorised over blocks: per block
    the shortest of the split-sample options and the uncompressed one (no zero-block, no second extension -- a valid
    stream, not the shortest one; not the grouping of `griblite.aec_encode`).  Returns uint8 bytes."""
    x = np.asarray(x, dtype=np.int64)
    n = x.size
    pad = (-n) % J
    if pad:
        x = np.concatenate([x, np.full(pad, x[-1])])
    xmax = (1 << nbits) - 1
    idl = 5 if nbits > 16 else 4 if nbits > 8 else 3
    id_raw = (1 << idl) - 1
    prev = np.concatenate([x[:1], x[:-1]])
    delta, theta = x - prev, np.minimum(prev, xmax - prev)
    d = np.where((delta >= 0) & (delta <= theta), 2 * delta,
                 np.where((delta < 0) & (-delta <= theta), -2 * delta - 1, theta + np.abs(delta)))
    d = d.reshape(-1, J)
    nblk = d.shape[0]
    ref = (np.arange(nblk) % rsi) == 0
    refval = x.reshape(-1, J)[:, 0]
    d[ref, 0] = 0
    nc = J - ref.astype(np.int64)
    ks = np.arange(0, min(id_raw - 2, nbits - 1) + 1)
    lens = np.stack([(d >> k).sum(axis=1) + nc * (k + 1) for k in ks], axis=1)
    best = lens.argmin(axis=1)
    split_len = lens[np.arange(nblk), best]
    raw = split_len >= nc * nbits
    k = np.where(raw, 0, ks[best])
    ids = np.where(raw, id_raw, k + 1)
    body = np.where(raw, nc * nbits, split_len)
    head = idl + ref * nbits
    start = np.concatenate([[0], np.cumsum(head + body)])
    bits = np.zeros(int(start[-1]), dtype=np.uint8)
    start = start[:-1]
    for j in range(idl):
        bits[start + j] = (ids >> (idl - 1 - j)) & 1
    rb = np.flatnonzero(ref)
    for j in range(nbits):
        bits[start[rb] + idl + j] = (refval[rb] >> (nbits - 1 - j)) & 1
    at = start + head                                     # first bit of the coded part
    coded = np.ones_like(d, dtype=bool)
    coded[ref, 0] = False
    # split-sample: the terminating ones of the fundamental sequences, then the k-bit remainders
    sp = np.flatnonzero(~raw)
    q = (d[sp] >> k[sp, None]) + 1
    q[~coded[sp]] = 0
    ends = at[sp, None] + np.cumsum(q, axis=1) - 1
    bits[ends[coded[sp]]] = 1
    fs_len = q.sum(axis=1)
    slot = np.cumsum(coded[sp], axis=1) - 1                 # the sample's place among the coded ones
    for kk in np.unique(k[sp]):
        if kk == 0:
            continue
        m = k[sp] == kk
        rows_, pos = sp[m], (at[sp][m] + fs_len[m])[:, None] + slot[m] * kk
        for j in range(kk):
            bits[(pos + j)[coded[rows_]]] = ((d[rows_] >> (kk - 1 - j)) & 1)[coded[rows_]]
    # uncompressed: the coded samples as they are (the reference stands in front of them already)
    rw = np.flatnonzero(raw)
    slot_r = np.cumsum(coded[rw], axis=1) - 1
    for j in range(nbits):
        pos = at[rw, None] + slot_r * nbits + j
        bits[pos[coded[rw]]] = ((d[rw] >> (nbits - 1 - j)) & 1)[coded[rw]]
    return np.packbits(bits)


def _second_differences(x):
    """(z = second difference - g with the two placeholders 0, g) of int64 x: what order 2 codes"""
    d = np.zeros(x.size, dtype=np.int64)
    d[2:] = x[2:] - 2 * x[1:-1] + x[:-2]
    g = int(d[2:].min())
    z = d - g
    z[:2] = 0
    return z, g


def _complex_stream(x, g, ref, w, stored, n, nbits, group, n_oct):
    """(stream, the fields of a GRIB_CPX_DTYPE record from n_groups to n_oct) of template 5.3, order 2, groups of `group`
    positions with references ref and widths w, n positions holding `stored` (padded to whole groups)"""
    ng = ref.size
    width_ref = int(w.min())
    width_bits = int(_bit_length(w.max() - width_ref))
    stream = _sm(x[0], n_oct) + _sm(x[1], n_oct) + _sm(g, n_oct) + _pack(ref, np.full(ng, nbits)).tobytes() + \
        _pack(w - width_ref, np.full(ng, width_bits)).tobytes() + _pack(stored.ravel()[:n], np.repeat(w, group)[:n]).tobytes()
    return np.frombuffer(stream, dtype=np.uint8), (ng, nbits, width_ref, width_bits, group, 1, n - (ng - 1) * group, 0, 2, n_oct)


def encode_complex(q, group=GROUP, n_oct=N_OCT):
    """(stream, the fields of a GRIB_CPX_DTYPE record from n_groups to n_oct) for the unsigned integers q: template 5.3,
    order 2, groups of `group` values (the last one shorter), every group with its own minimal width (a valid stream,
    not the grouping of `griblite.cpx_encode`)."""
    x = np.asarray(q, dtype=np.int64)
    n = x.size
    z, g = _second_differences(x)
    ng = (n + group - 1) // group
    zz = np.concatenate([z, np.full(ng * group - n, z[-1])]).reshape(ng, group)
    ref = zz.min(axis=1)
    w = _bit_length(zz.max(axis=1) - ref)
    return _complex_stream(x, g, ref, w, zz - ref[:, None], n, int(_bit_length(ref.max())), group, n_oct)


def encode_complex_mv(q, present, group=GROUP, n_oct=N_OCT, mvm=1):
    """(stream, the fields of a GRIB_CPX_DTYPE record from n_groups to n_oct) of a row of present.size positions under
    missing value management `mvm`: the present ones hold the integers q in order (order 2 over them), a missing one
    holds 2^w - 1 of its group, every group wide enough to keep its values below the `mvm` codes at the top."""
    x = np.asarray(q, dtype=np.int64)
    zc, g = _second_differences(x)
    n = present.size
    ng = (n + group - 1) // group
    there = np.concatenate([present, np.zeros(ng * group - n, dtype=bool)]).reshape(ng, group)
    z = np.zeros(ng * group, dtype=np.int64)
    z[np.flatnonzero(there.ravel())] = zc
    z = z.reshape(ng, group)
    if not there.any(axis=1).all():
        raise SystemExit("a group without a present position: the tool's encoder does not write those")
    ref = np.where(there, z, np.iinfo(np.int64).max).min(axis=1)
    w = _bit_length(np.where(there, z, 0).max(axis=1) - ref + mvm)          # span < 2^w - mvm
    stored = np.where(there, z - ref[:, None], (np.int64(1) << w)[:, None] - 1)
    return _complex_stream(x, g, ref, w, stored, n, int(_bit_length(ref.max() + mvm)), group, n_oct)


# what the coded-input tools need of a codec beside its `griblite.CODECS` entry, by the entry's name: the encoder as
# (stream, the record's fields between n_values and the reserved one)
CODERS = {"ccsds": lambda q: (encode_ccsds(q), (NBITS, BLOCK, RSI, FLAGS)), "cpx": encode_complex}


def coded_record(codec, byte_off, stream, n_values, params):
    return np.array((byte_off, stream.size, n_values) + params + (0,), dtype=codec.dtype)


# ------------------------------------------------------------------------------------------------ fields
def smooth_field(S, i, rng):
    """16-bit integers of a smooth field: a few waves over the index, noise of a few counts."""
    t = np.arange(S) / S
    f = 32768 + 18000 * np.sin(2 * np.pi * (3 + i) * t) * np.cos(2 * np.pi * 41 * t) + 4000 * np.sin(2 * np.pi * 977 * t)
    return np.clip(np.rint(f + rng.normal(0.0, 3.0, S)), 0, 65535).astype(np.uint32)


def int16_rows(rows, n_src, seed=20261016):
    """ERA5-like int16 rows: full range, -32768 as _FillValue on ~3 % of the cells (16 distinct rows, tiled)."""
    rng = np.random.default_rng(seed)
    blk = rng.integers(-32767, 32768, size=(16, n_src)).astype(np.int16)
    blk[rng.random(blk.shape) < 0.03] = -32768
    return np.ascontiguousarray(np.tile(blk, ((rows + 15) // 16, 1))[:rows])


def int16_levels(masks, n_steps, seed=20261016):
    """(n_steps, n_lev, 1, S) int16: full range over the ocean, -32768 (_FillValue) where the level's mask is 0;
    4 distinct time steps, tiled."""
    rng = np.random.default_rng(seed)
    n_lev, S = masks.shape
    blk = rng.integers(-32767, 32768, size=(4, n_lev, 1, S)).astype(np.int16)
    blk[:, masks[:, None, :] == 0] = -32768
    return np.ascontiguousarray(np.tile(blk, ((n_steps + 3) // 4, 1, 1, 1))[:n_steps])


def half_fields(shape, seed=20261018):
    """The same values as float32, float16 and bfloat16 (16 distinct rows, tiled along the first axis)."""
    from smmregrid_amd import to_bfloat16
    rng = np.random.default_rng(seed)
    blk = (250.0 + 30.0 * rng.standard_normal((16,) + tuple(shape[1:]))).astype(np.float32)
    x32 = np.ascontiguousarray(np.tile(blk, ((shape[0] + 15) // 16,) + (1,) * (len(shape) - 1))[:shape[0]])
    return {"f32": x32, "f16": x32.astype(np.float16), "bf16": to_bfloat16(x32)}


def class_fields(shape, n_classes, seed=20261021):
    """{"u16": uint16, "f32": float32} fields of `shape` holding class codes 1 .. n_classes in patches (a smooth field cut
    into n_classes bands along its last axis, so neighbouring cells mostly share a class, as land cover does) with about
    2 % of the cells missing: 65535 / NaN"""
    rng = np.random.default_rng(seed)
    n = shape[-1]
    t = np.linspace(0.0, 40.0 * np.pi, n)
    smooth = np.sin(t)[None, :] + 0.6 * np.sin(2.3 * t + rng.uniform(0, 6, size=(int(np.prod(shape[:-1])), 1)))
    codes = 1 + np.minimum(((smooth + 1.6) / 3.2 * n_classes).astype(np.int64), n_classes - 1)
    hole = rng.random(codes.shape) < 0.02
    u16 = np.where(hole, 65535, codes).astype(np.uint16).reshape(shape)
    f32 = np.where(hole, np.nan, codes).astype(np.float32).reshape(shape)
    return {"u16": u16, "f32": f32}


def seeded_block(n_src, dtype, nan, rows=16, seed=20261016):
    """`rows` rows around 250 +- 30, with ~3 % NaN when asked for"""
    rng = np.random.default_rng(seed)
    blk = (250.0 + 30.0 * rng.standard_normal((rows, n_src))).astype(dtype)
    if nan:
        blk[rng.random(blk.shape) < 0.03] = np.nan
    return blk


def thinned(masks, seed=20261019):
    """the levels' bitmaps under skipna: each level's source mask with a further MISSING of the cells cleared"""
    rng = np.random.default_rng(seed)
    return np.stack([(m != 0) & (rng.random(m.size) >= MISSING) for m in masks]).astype(masks.dtype)


def _grib1_sm(value, nbytes):
    return ((1 << (8 * nbytes - 1)) | -value if value < 0 else value).to_bytes(nbytes, "big")


def _ibm32(x):
    """a float as IBM hexadecimal single precision (exactly representable inputs only)"""
    if x == 0:
        return bytes(4)
    sign = 0x80 if x < 0 else 0
    x, e = abs(x), 64
    while x >= 1.0:
        x, e = x / 16.0, e + 1
    while x < 1.0 / 16.0:
        x, e = x * 16.0, e - 1
    return bytes([sign | e]) + int(round(x * (1 << 24))).to_bytes(3, "big")


def grib1_message(values, ni, nj, date, nbits=16, param=167):
    """A GRIB-1 message of a global lon/lat field (north to south, from 0 E) in simple packing, written from the section
    layout (WMO FM 92, edition 1): what the file block of grib_bench.py opens."""
    scaled = np.asarray(values, dtype=np.float64).ravel()
    ref = float(np.floor(scaled.min() * 16.0) / 16.0)
    span = scaled.max() - ref
    e = 0 if span == 0 else int(np.ceil(np.log2(span / ((1 << nbits) - 1))))
    x = np.round((scaled - ref) / 2.0 ** e).astype(np.uint64)
    bits = ((x[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).ravel()
    pad = (-bits.size) % 16
    data = np.packbits(np.r_[bits, np.zeros(pad, np.uint8)]).tobytes()
    y, mo, d, h = date
    pds = bytearray(28)
    pds[0:3] = (28).to_bytes(3, "big")
    pds[3:9] = 128, 98, 1, 255, 0x80, param
    pds[9] = 1
    pds[12:18] = y % 100 or 100, mo, d, h, 0, 1
    pds[24] = (y - 1) // 100 + 1
    gds = bytearray(32)
    gds[0:3] = (32).to_bytes(3, "big")
    gds[4] = 255
    gds[6:8], gds[8:10] = ni.to_bytes(2, "big"), nj.to_bytes(2, "big")
    gds[10:13], gds[13:16] = _grib1_sm(90000, 3), _grib1_sm(0, 3)
    gds[16] = 0x80
    gds[17:20], gds[20:23] = _grib1_sm(-90000, 3), _grib1_sm(int(round((360.0 - 360.0 / ni) * 1000)), 3)
    gds[23:25] = (0xFFFF).to_bytes(2, "big")
    gds[25:27] = int(180000 // (nj - 1)).to_bytes(2, "big")
    bds = (11 + len(data)).to_bytes(3, "big") + bytes([pad & 0x0F]) + _grib1_sm(e, 2) + _ibm32(ref) + bytes([nbits]) + data
    body = bytes(pds) + bytes(gds) + bds + b"7777"
    return b"GRIB" + (8 + len(body)).to_bytes(3, "big") + b"\x01" + body


def lonlat_messages(rows, ni=1440, nj=721, seed=20261018):
    """`rows` 16-bit GRIB-1 messages of one noisy 2-m temperature field, a day apart"""
    rng = np.random.default_rng(seed)
    base = 250.0 + 30.0 * rng.standard_normal((nj, ni))
    return [grib1_message(base + day, ni, nj, (2021, 1 + day // 28, 1 + day % 28, 12)) for day in range(rows)]


# ------------------------------------------------------------------------------------------------ stream tables
def stream_table(blocks, rows, refs, E, nbits=NBITS, gap=117, pad4=False):
    """The distinct streams `blocks` laid out in one zeroed buffer with `gap` bytes in front of each and behind the last
    (pad4: the buffer rounded up to 4 bytes), and a GRIB_ROW_DTYPE table of `rows` rows pointing at them in turn, row r
    with reference refs[r % len(blocks)] and binary scale E.  Returns (buffer, table, the streams' offsets)."""
    from smmregrid_amd import GRIB_ROW_DTYPE
    offs, pos = [], gap
    for b in blocks:
        offs.append(pos)
        pos += b.size + gap
    buf = np.zeros((pos + 3) // 4 * 4 if pad4 else pos, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        buf[o:o + b.size] = b
    table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    for r in range(rows):
        table[r] = (offs[r % len(blocks)], refs[r % len(blocks)], 2.0 ** E, 1.0, nbits, 0)
    return buf, table, offs


def _refs():
    return [float(np.float32(220.0 + i)) for i in range(DISTINCT)]


def source(S, rows, seed):
    """DISTINCT smooth 16-bit fields simple-packed in one buffer, `rows` records pointing at them in turn: the input of
    the coded-result tools (seed: SEEDS of the codec)."""
    rng = np.random.default_rng(seed)
    blocks = [np.frombuffer(pack16(smooth_field(S, i, rng)), dtype=np.uint8) for i in range(DISTINCT)]
    return stream_table(blocks, rows, _refs(), -6, gap=116, pad4=True)[:2]


def make_coded_streams(codec, S, rows, seed=None):
    """For a `griblite.CODECS` entry: (coded buffer, row table, the codec's records), (simple-packed buffer, row table),
    the float32 field, the distinct streams, their record parameters, the references and E.  Every stream is decoded
    back by the library's host decoder first."""
    rng = np.random.default_rng(SEEDS[codec.name] if seed is None else seed)
    E, refs = -6, _refs()
    coded, params, simple, dec = [], [], [], []
    for i in range(DISTINCT):
        q = smooth_field(S, i, rng)
        stream, p = CODERS[codec.name](q)
        if not np.array_equal(codec.decode(stream, coded_record(codec, 0, stream, S, p), 0)[0], q):
            raise SystemExit("the tool's encoder wrote a stream the host decoder reads differently")
        coded.append(stream)
        params.append(p)
        simple.append(np.frombuffer(pack16(q), dtype=np.uint8))
        dec.append(((refs[i] + q.astype(np.float64) * 2.0 ** E) / 1.0).astype(np.float32))
    cbuf, crows, coffs = stream_table(coded, rows, refs, E)
    recs = np.zeros(rows, dtype=codec.dtype)
    for r in range(rows):
        recs[r] = coded_record(codec, coffs[r % DISTINCT], coded[r % DISTINCT], S, params[r % DISTINCT])
    sbuf, srows, _ = stream_table(simple, rows, refs, E)
    field = np.ascontiguousarray(np.stack([dec[r % DISTINCT] for r in range(rows)]))
    return (cbuf, crows, recs), (sbuf, srows), field, coded, params, refs, E


def make_streams(S, rows, D, widths=(16, 12), seed=20261018):
    """The packed streams of `rows` fields of S values at 16 and at 12 bits -- message after message with a gap of 117
    bytes between them, as sections 0 - 3 would leave -- their row tables, and the float32 field griblite decodes from
    them (the parent road's input)."""
    from smmregrid_amd import GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _unpack_bits
    assert S % 2 == 0
    rng = np.random.default_rng(seed)
    out = {}
    for nbits, pack in ((16, pack16), (12, pack12)):
        if nbits not in widths:
            continue
        blocks, refs = [], []
        for i in range(DISTINCT):
            q = rng.integers(0, 1 << nbits, size=S, dtype=np.uint32)
            blocks.append(pack(q))
            refs.append(float(np.float32(220.0 + i)))
        E = -6 if nbits == 16 else -2          # ~ 0.016 K / 0.25 K steps over a 1000-K span
        table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
        pieces, pos = [], 0
        for b in range(rows):
            pieces.append(bytes(117))
            pos += 117
            table[b] = (pos, refs[b % DISTINCT], 2.0 ** E, 10.0 ** D, nbits, 0)
            pieces.append(blocks[b % DISTINCT])
            pos += len(blocks[b % DISTINCT])
        buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        dec = np.empty((DISTINCT, S), dtype=np.float32)
        for i in range(DISTINCT):
            dec[i] = (refs[i] + _unpack_bits(blocks[i], nbits, S) * 2.0 ** E) / 10.0 ** D
        field = np.ascontiguousarray(np.tile(dec, ((rows + DISTINCT - 1) // DISTINCT, 1))[:rows])
        out[nbits] = (buf, table, field, blocks[0], refs[0], E)
    return out


def make_bitmap_streams(S, rows, widths=(16, 12), seed=20261019):
    """Per width: the buffer -- message after message: a gap of 117 bytes, the bitmap, a gap of 11, the packed present
    values -- the row table, the bitmap records, the float32 field griblite decodes (NaN where the bitmap is 0), and the
    rule and bitmap of message 0 for the decode timing."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _decode_rule
    rng = np.random.default_rng(seed)
    masks = []
    for i in range(DISTINCT):
        m = rng.random(S) >= MISSING
        if m.sum() % 2:                       # pack12 writes pairs
            m[np.flatnonzero(~m)[0]] = True
        masks.append(m)
    out = {}
    for nbits, pack in ((16, pack16), (12, pack12)):
        if nbits not in widths:
            continue
        E = -6 if nbits == 16 else -2
        blocks = [pack(rng.integers(0, 1 << nbits, size=int(m.sum()), dtype=np.uint32)) for m in masks]
        bmbytes = [np.packbits(m.astype(np.uint8)).tobytes() for m in masks]
        refs = _refs()
        table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
        bitmaps = np.zeros(rows, dtype=GRIB_BITMAP_DTYPE)
        pieces, pos = [], 0
        for b in range(rows):
            i = b % DISTINCT
            pieces.append(bytes(117))
            pos += 117
            bitmaps[b] = (pos, int(masks[i].sum()))
            pieces.append(bmbytes[i])
            pos += len(bmbytes[i])
            pieces.append(bytes(11))
            pos += 11
            table[b] = (pos, refs[i], 2.0 ** E, 1.0, nbits, 0)
            pieces.append(blocks[i])
            pos += len(blocks[i])
        buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        del pieces
        rule = lambda b: (int(table[b]["byte_off"]), float(table[b]["ref"]), float(table[b]["bscale"]), 1.0, nbits)   # noqa: E731
        bm = lambda b: (int(bitmaps[b]["bitmap_off"]), int(bitmaps[b]["n_values"]))                                  # noqa: E731
        dec = np.empty((DISTINCT, S), dtype=np.float32)
        for i in range(DISTINCT):
            dec[i] = _decode_rule(buf, rule(i), S, bm(i))
        field = np.ascontiguousarray(np.tile(dec, ((rows + DISTINCT - 1) // DISTINCT, 1))[:rows])
        out[nbits] = (buf, table, bitmaps, field, rule(0), bm(0))
    return out


def make_level_streams(masks, n_steps, nbits, seed=20261019):
    """The buffer -- message after message in (step, level) order: a gap of 117 bytes, the level's bitmap, a gap of 11,
    the packed values of its present cells -- the row table and the bitmap records shaped (n_steps, n_lev, 1), the float32
    field (n_steps, n_lev, 1, S) griblite decodes from it (DISTINCT distinct steps, tiled) and the rule and bitmap of
    each level's first message for the decode timing."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _decode_rule
    rng = np.random.default_rng(seed)
    n_lev, S = masks.shape
    pack, E = (pack16, -6) if nbits == 16 else (pack12, -2)
    present = [masks[l] != 0 for l in range(n_lev)]
    bmbytes = [np.packbits(m.astype(np.uint8)).tobytes() for m in present]
    # pack12 writes pairs: an odd count gets one value more, which no row's n_values reaches
    blocks = [[pack(rng.integers(0, 1 << nbits, size=int(m.sum()) + int(m.sum()) % 2, dtype=np.uint32)) for m in present]
              for _ in range(DISTINCT)]
    table = np.zeros((n_steps, n_lev, 1), dtype=GRIB_ROW_DTYPE)
    bitmaps = np.zeros((n_steps, n_lev, 1), dtype=GRIB_BITMAP_DTYPE)
    pieces, pos = [], 0
    for t in range(n_steps):
        for l in range(n_lev):
            pieces.append(bytes(117))
            pos += 117
            bitmaps[t, l, 0] = (pos, int(present[l].sum()))
            pieces.append(bmbytes[l])
            pos += len(bmbytes[l])
            pieces.append(bytes(11))
            pos += 11
            table[t, l, 0] = (pos, float(np.float32(220.0 + l + t % DISTINCT)), 2.0 ** E, 1.0, nbits, 0)
            pieces.append(blocks[t % DISTINCT][l])
            pos += len(blocks[t % DISTINCT][l])
    buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    del pieces
    rule = lambda t, l: (int(table[t, l, 0]["byte_off"]), float(table[t, l, 0]["ref"]), float(table[t, l, 0]["bscale"]), 1.0, nbits)  # noqa: E731
    bm = lambda t, l: (int(bitmaps[t, l, 0]["bitmap_off"]), int(bitmaps[t, l, 0]["n_values"]))                                       # noqa: E731
    dec = np.empty((min(DISTINCT, n_steps), n_lev, 1, S), dtype=np.float32)
    for t in range(dec.shape[0]):
        for l in range(n_lev):
            dec[t, l, 0] = _decode_rule(buf, rule(t, l), S, bm(t, l))
    field = np.ascontiguousarray(np.tile(dec, ((n_steps + DISTINCT - 1) // DISTINCT, 1, 1, 1))[:n_steps])
    return buf, table, bitmaps, field, [(rule(0, l), bm(0, l)) for l in range(n_lev)]


def _slots(streams):
    """The streams back to back, each followed by 4 to 7 zero bytes up to a multiple of 4: (buffer, their offsets)"""
    parts, offs, at = [], [], 0
    for s in streams:
        offs.append(at)
        parts += [np.asarray(s, np.uint8), np.zeros(-s.size % 4 + 4, np.uint8)]
        at += parts[-2].size + parts[-1].size
    return np.concatenate(parts), offs


def make_mv_streams(S, rows, seed=20261020):
    """The smooth fields with MISSING of the cells missing at random, complex-packed both ways in one buffer: with the
    missing values inside the groups (missing value management 1) and compacted beside a bitmap (management 0).  Returns
    the buffer, the row table, the records of the mvm-1 rows, those of the mvm-0 rows and the bitmap records of the
    latter.  Every stream is decoded back by the library's host decoder first."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import CPX, cpx_decode, cpx_decode_mv
    rng = np.random.default_rng(seed)
    streams, pars, counts = [], [], []
    for i in range(DISTINCT):
        present = rng.random(S) >= MISSING
        q = smooth_field(S, i, rng)[present]
        s_mv, p_mv = encode_complex_mv(q, present)
        s_0, p_0 = encode_complex(q)
        got, there = cpx_decode_mv(s_mv, coded_record(CPX, 0, s_mv, S, p_mv), 1)
        if not (np.array_equal(got, q) and np.array_equal(there, present) and
                np.array_equal(cpx_decode(s_0, coded_record(CPX, 0, s_0, q.size, p_0)), q)):
            raise SystemExit("the tool's encoder wrote a stream the host decoder reads differently")
        streams += [s_mv, s_0, np.packbits(present)]
        pars.append((p_mv, p_0))
        counts.append(int(q.size))
    buf, offs = _slots(streams)
    table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    cpx_mv, cpx_0 = np.zeros(rows, dtype=GRIB_CPX_DTYPE), np.zeros(rows, dtype=GRIB_CPX_DTYPE)
    bms = np.zeros(rows, dtype=GRIB_BITMAP_DTYPE)
    for r in range(rows):
        k = r % DISTINCT
        table[r] = (0, 220.0 + k, 2.0 ** -6, 1.0, 16, 0)
        cpx_mv[r] = coded_record(CPX, offs[3 * k], streams[3 * k], S, pars[k][0])
        cpx_0[r] = coded_record(CPX, offs[3 * k + 1], streams[3 * k + 1], counts[k], pars[k][1])
        bms[r] = (offs[3 * k + 2], counts[k])
    return buf, table, cpx_mv, cpx_0, bms


def make_plain_complex_streams(S, rows, seed=20261020):
    """The smooth fields complex-packed with no cell missing, slot after slot: (buffer, records)"""
    from smmregrid_amd import GRIB_CPX_DTYPE
    from smmregrid_amd.griblite import CPX
    rng = np.random.default_rng(seed)
    coded = [encode_complex(smooth_field(S, i, rng)) for i in range(DISTINCT)]
    buf, offs = _slots([s for s, _ in coded])
    cpx = np.zeros(rows, dtype=GRIB_CPX_DTYPE)
    for r in range(rows):
        k = r % DISTINCT
        cpx[r] = coded_record(CPX, offs[k], coded[k][0], S, coded[k][1])
    return buf, cpx
