"""Buffers whose rows lie past 2^31 and 2^32 elements, for the tests that pin the 64-bit address arithmetic of every
entry (tests/test_gpu_far_offsets.py) and for the proof that the checker catches what it is for
(tests/test_far_cases.py).  Plain numpy, no GPU.

A `Layout` is a flat buffer with a handful of short true rows on a huge pitch: the arithmetic stays tiny, only the
addresses are large.  An offset narrowed somewhere on its way into a kernel lands on an ALIAS of the true row:

  elems31   the element offset taken mod 2^31
  elems32   the element offset taken mod 2^32
  bytes32   the byte offset taken mod 2^32
  sext32    the element offset cut to 32 bits and sign-extended

X is filled with decoys (finite values of another mean) before the true rows are copied in, so a wrapped read gives a
finite wrong number; Y is filled with the byte 0x42, and after the call every true row must hold the reference's bits
while each true row's guard band and a row-length window at every alias of every true row still hold 0x42.

Everything takes `modulus` (2^31; "2^32" is twice it) and `guard` (4096), so that the CPU test walks the same code at
2^12 on buffers of a few thousand elements.

The last section places BYTE STREAMS at far byte offsets, for the GRIB transcoders (tests/test_gpu_grib_far_offsets.py):
`StreamLayout`, the alias streams and the slot checks of the output side."""
from collections import namedtuple

import numpy as np

MODULUS = 1 << 31
GUARD = 4096
SENTINEL = 0x42
TRUNCATIONS = ("elems31", "elems32", "bytes32", "sext32")


def truncate(offset, itemsize, kind, modulus=MODULUS):
    """Where an access to element `offset` lands when the offset is narrowed in the way `kind` names (it may be
    negative or beyond the buffer: then a kernel would fault instead of corrupting)."""
    offset = int(offset)
    if kind == "elems31":
        return offset % modulus
    if kind == "elems32":
        return offset % (2 * modulus)
    if kind == "bytes32":
        return (offset * itemsize) % (2 * modulus) // itemsize
    if kind == "sext32":
        v = offset % (2 * modulus)
        return v - 2 * modulus if v >= modulus else v
    raise KeyError(kind)


def aliases(offset, itemsize, buffer_elems, modulus=MODULUS):
    """Every in-buffer element position, other than `offset` itself, where an access to `offset` would land under
    one of the four truncations."""
    hits = {truncate(offset, itemsize, k, modulus) for k in TRUNCATIONS}
    return sorted(a for a in hits if a != offset and 0 <= a < buffer_elems)


class Layout(namedtuple("Layout", "offsets row_len size guard modulus")):
    """offsets: element offset of every true row in a flat buffer of `size` elements; each row has `row_len` elements
    that matter and `guard` elements on both sides that nothing may touch."""

    def crossed(self):
        """(rows at or past `modulus` elements, rows at or past twice that)"""
        return (sum(o >= self.modulus for o in self.offsets), sum(o >= 2 * self.modulus for o in self.offsets))

    def nbytes(self, itemsize):
        return self.size * itemsize


def _round4(n):
    return -(-int(n) // 4) * 4


def pitch(n_rows, row_len, modulus=MODULUS, guard=GUARD):
    """The far pitch of `n_rows` rows: the power of two at which the last rows cross `modulus` and then twice it, plus
    K >= row_len + 2 guard, a multiple of 4 (16-B aligned rows of 4-byte elements stay eligible for LDS-DMA staging).
    5 rows: 2^30 + K (row 2 past 2^31, row 4 past 2^32); 3 rows: 2^31 + K; 33 .. 64 rows: 2^27 + K."""
    if n_rows < 3:
        raise ValueError("a far layout needs at least 3 rows: one below, one past each threshold")
    step = (2 * modulus) >> ((n_rows - 1).bit_length() - 1)
    return step + _round4(row_len + 2 * guard)


def rows_layout(n_rows, row_len, modulus=MODULUS, guard=GUARD, inner=1, inner_stride=None):
    """`n_rows` far rows of `pitch`, each of them `inner` near rows `inner_stride` apart (a second, near stride: the
    inner rows of a level, the levels of an outer step).  Row (r, i) lies at guard + r * pitch + i * inner_stride;
    the offsets are listed r-major.  The standard row-major layout is rows_layout(5, n_src); the batch-fastest one is
    rows_layout(S, B) with S of about 40 source cells: X is (S, ldx) and c * ldx crosses both thresholds."""
    inner_stride = _round4(row_len + 2 * guard) if inner_stride is None else int(inner_stride)
    ld = pitch(n_rows, inner * inner_stride if inner > 1 else row_len, modulus, guard)
    lead = _round4(guard)
    offsets = tuple(lead + r * ld + i * inner_stride for r in range(n_rows) for i in range(inner))
    lay = Layout(offsets, int(row_len), offsets[-1] + row_len + guard, int(guard), int(modulus))
    past1, past2 = lay.crossed()
    assert past2 >= 1 and past1 > past2 and past1 < len(offsets), "rows below, past the first and past the second threshold"
    return lay, ld


def host_rows_layout(n_rows, row_len, guard=GUARD):
    """rows_layout at half the thresholds -- 5 rows on a pitch of 2^29 + K: row 2 past 2^30 elements (2^32 bytes of a
    4-byte type), row 4 past 2^31 elements (2^32 bytes of a 2-byte type) -- for host arrays, whose mapping stays under
    9 GB with float32 and int16.  The aliases are still taken at the real 2^31 / 2^32."""
    lay, ld = rows_layout(n_rows, row_len, MODULUS // 2, guard)
    return lay._replace(modulus=MODULUS), ld


def near_layout(n_rows, row_len, modulus=MODULUS):
    """The ordinary C-contiguous (n_rows, row_len) array as a Layout: the side of a case that stays near."""
    return Layout(tuple(r * int(row_len) for r in range(n_rows)), int(row_len), n_rows * int(row_len), 0, int(modulus))


def windows(layout, itemsize):
    """The regions [start, stop) of a Y buffer that must keep their sentinel bytes: the guard band on both sides of
    every true row and a row-length window at every alias of every true row, merged and clipped to the buffer.
    ValueError if a window overlaps a true row (then the layout cannot tell a wrapped write from a right one)."""
    L, n, g = layout, layout.row_len, layout.guard
    spans = []
    for o in L.offsets:
        spans.append((max(o - g, 0), o))
        spans.append((o + n, min(o + n + g, L.size)))
        for a in aliases(o, itemsize, L.size, L.modulus):
            spans.append((a, min(a + n, L.size)))
    for s, e in spans:
        for o in L.offsets:
            if s < o + n and o < e:
                raise ValueError(f"window [{s}, {e}) overlaps the true row at {o}")
    merged = []
    for s, e in sorted(x for x in spans if x[1] > x[0]):
        if merged and s <= merged[-1][1]:
            merged[-1][1] = max(merged[-1][1], e)
        else:
            merged.append([s, e])
    return [tuple(m) for m in merged]


# ------------------------------------------------------------------ the checks, shared by the CPU and the GPU test

def check_rows(got, want, what=""):
    """Bit equality of the true rows; in float32 / float64 rows a NaN equals a NaN (the kernels and the oracle agree on
    where the NaNs are, not on their payloads), rows of any other type -- raw 2-byte results -- are compared as bits."""
    got, want = np.ascontiguousarray(got), np.ascontiguousarray(want)
    assert got.shape == want.shape and got.dtype.itemsize == want.dtype.itemsize, (what, got.shape, want.shape)
    u = f"u{got.dtype.itemsize}"
    diff = got.view(u) != want.view(u)
    if got.dtype.kind == "f" and want.dtype == got.dtype:
        diff &= ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{what}: {int(diff.sum())} results differ in their bits, first at {np.argwhere(diff)[:3].tolist()}"


def check_windows(read_bytes, layout, itemsize, what=""):
    """read_bytes(start, stop) returns the bytes of elements [start, stop) of the Y buffer: every window must still
    hold the sentinel.  The message names the truncations whose alias was written."""
    for s, e in windows(layout, itemsize):
        raw = np.asarray(read_bytes(s, e)).view(np.uint8).ravel()
        assert raw.size == (e - s) * itemsize
        bad = np.flatnonzero(raw != SENTINEL)
        if bad.size:
            at = s + int(bad[0]) // itemsize
            named = [f"{k} of row {r}" for r, o in enumerate(layout.offsets) for k in TRUNCATIONS
                     if 0 <= at - truncate(o, itemsize, k, layout.modulus) < layout.row_len
                     and truncate(o, itemsize, k, layout.modulus) != o]
            raise AssertionError(f"{what}: element {at} of Y was written ({bad.size} bytes in window [{s}, {e})): "
                                 f"{', '.join(named) or 'a guard band'}")


# ------------------------------------------------------------------ byte streams at far byte offsets
# The GRIB transcoders (tests/test_gpu_grib_far_offsets.py) read coded rows from "one buffer of the whole file" and write
# slots laid back to back.  A row is a byte stream at a 64-bit byte offset, and beside the four narrowings above a bit
# position or a word index may be the thing that is cut to 32 bits:
#
#   bits32    8 * byte_off kept in 32 bits: the stream is read at byte_off mod 2^29
#   words32   byte_off >> 2 kept in 32 bits: the stream is read at byte_off mod 2^34
#
# A narrowed read that lands on decoys gives noise, which a decoder may refuse or turn into integers that look wrong.  The
# dangerous one lands on another valid stream: so one near row of a `StreamLayout` lies exactly where a far row's offset
# lands mod 2^32, and holds a DIFFERENT valid stream of the same record shape (`cpx_alias`, `aec_alias`): the far row's
# record decodes it cleanly, to the wrong integers.

STREAM_TRUNCATIONS = TRUNCATIONS + ("bits32", "words32")


def truncate_stream(byte_off, kind, modulus=MODULUS):
    """Where the read of a stream at byte `byte_off` lands under the narrowing `kind` (2^32 is twice `modulus`)."""
    byte_off = int(byte_off)
    if kind == "bits32":
        return byte_off % (modulus // 4)
    if kind == "words32":
        return byte_off % (8 * modulus)
    return truncate(byte_off, 1, kind, modulus)


def stream_images(byte_off, x_bytes, modulus=MODULUS):
    """{kind: landing byte} for every narrowing that moves a read of `byte_off` and keeps it inside the buffer."""
    out = {}
    for kind in STREAM_TRUNCATIONS:
        at = truncate_stream(byte_off, kind, modulus)
        if at != byte_off and 0 <= at < x_bytes:
            out[kind] = at
    return out


class StreamLayout(namedtuple("StreamLayout", "far alias near x_bytes modulus")):
    """far: byte offsets of three streams just past `modulus`, twice it (an odd offset) and eight times it (2^31, 2^32
    and 2^34 bytes); the last one ends in the buffer's last word.  alias: far[1] taken mod 2^32, where a different stream
    of far[1]'s shape lies.  near: the offsets of the other near streams."""

    def offsets(self):
        """Every stream's offset, in the order far[0], far[1], far[2], alias, near..."""
        return self.far + (self.alias,) + self.near


def stream_layout(far_lens, near_lens, modulus=MODULUS, guard=GUARD):
    """The layout for three far streams of far_lens bytes, the alias of the second (as long as it) and near streams of
    near_lens bytes.  All near offsets, and the far offsets taken mod modulus / 4, lie below modulus / 4 and apart by at
    least `guard`, so every narrowed read of a far row lands on the alias or on `guard` bytes of decoys ahead of them."""
    far_lens, near_lens = [int(n) for n in far_lens], [int(n) for n in near_lens]
    assert len(far_lens) == 3
    a0 = _round4(guard) + 2
    a1 = _round4(a0 + far_lens[0] + guard) + 1
    a2 = _round4(a1 + far_lens[1] + guard)
    at, near = a2 + far_lens[2], []
    for k, n in enumerate(near_lens):
        near.append(_round4(at + guard) + (3, 0, 1, 2)[k % 4])
        at = near[-1] + n
    assert at + guard <= modulus // 4, f"{at} bytes of near streams do not fit below {modulus // 4}"
    far = (modulus + a0, 2 * modulus + a1, 8 * modulus + a2)
    lay = StreamLayout(far, a1, tuple(near), far[2] + far_lens[2], int(modulus))
    spans = sorted(zip(lay.offsets(), far_lens + [far_lens[1]] + near_lens))
    assert all(o + n <= p for (o, n), (p, _) in zip(spans, spans[1:]))
    # far[1] lands on the alias under every narrowing that moves it; no other image of a stream touches a stream
    assert set(stream_images(far[1], lay.x_bytes, modulus).values()) == {a1}
    for off, length in ((far[0], far_lens[0]), (far[2], far_lens[2])):
        for img in stream_images(off, lay.x_bytes, modulus).values():
            assert all(img + length <= o or img >= o + n for o, n in spans), (off, img)
    return lay


def stream_buffer(lay, streams, seed=0):
    """A host buffer of lay.x_bytes rounded up to 4 bytes: random decoy bytes, then `streams` (uint8 arrays, in the order
    of `lay.offsets()`).  For the CPU proof; the GPU test fills a device buffer the same way."""
    buf = np.random.default_rng(seed).integers(0, 256, _round4(lay.x_bytes), dtype=np.uint8)
    for off, s in zip(lay.offsets(), streams):
        buf[off:off + len(s)] = s
    return buf


class AliasRow:
    """A stand-in for a case of tests/complex_cases.py or a fixture of tests/golden/ccsds: other integers in a stream of
    the same length that the same record parameters decode."""

    def __init__(self, of, X, stream):
        self.name, self.of = f"alias_of_{of.name}", of
        self.X = self.values = np.asarray(X)
        self.stream, self.n_values = np.asarray(stream, dtype=np.uint8), int(len(X))
        for k in ("params", "nbits", "block", "rsi", "flags"):
            if hasattr(of, k):
                setattr(self, k, getattr(of, k))
        self.width = int(np.max(X)).bit_length() if len(X) else 0

    def record(self, byte_off):
        return self.of.record(byte_off)

    def __repr__(self):
        return self.name


def cpx_alias(case):
    """A complex-packed stream of the shape of `case` (tests/complex_cases.py) with other integers: at order 1 / 2 every
    seed h_k is one larger, so every integer is; at order 0 the first group's reference is one smaller (or larger).
    Checked with the numpy decoder of the cases: valid, inside [0, 2^32), different."""
    from tests import complex_cases as xc
    p, s = case.params, case.stream.copy()
    if p["order"]:
        for k in range(p["order"]):
            at = (k + 1) * p["n_oct"] - 1                    # the low octet of a sign-magnitude number
            assert s[at] < 255 and not s[k * p["n_oct"]] & 0x80
            s[at] += 1
    else:
        nb = p["nbits"]
        assert 0 < nb <= 32
        bits = np.unpackbits(s[:(nb + 7) // 8])
        ref = int("".join(str(b) for b in bits[:nb]), 2)
        ref = ref - 1 if ref > 0 else ref + 1
        bits[:nb] = [int(c) for c in format(ref, f"0{nb}b")]
        s[:(nb + 7) // 8] = np.packbits(bits)
    X = xc.numpy_decode(s, case.n_values, p)
    assert X.min() >= 0 and X.max() < 2 ** 32 and (X != case.X).any(), case
    return AliasRow(case, X, s)


def aec_alias(fx, tries=32):
    """A CCSDS stream that the record of the fixture `fx` decodes -- no longer than the fixture's own, padded to its
    length -- with one sample changed: coded by the library's host encoder, checked by its host decoder."""
    from smmregrid_amd.griblite import aec_decode, aec_encode
    from tests.ccsds_cases import record
    rec = record(0, fx.stream.size, fx.n_values, fx.nbits, fx.block, fx.rsi, fx.flags)
    for k in range(min(tries, fx.n_values)):
        v = np.asarray(fx.values, dtype=np.uint32).copy()
        v[fx.n_values - 1 - k] ^= 1
        st = aec_encode(v, rec)
        if st.size > fx.stream.size:
            continue
        padded = np.full(fx.stream.size, 0x5A, np.uint8)
        padded[:st.size] = st
        try:
            if np.array_equal(aec_decode(padded, rec), v):
                return AliasRow(fx, v, padded)
        except ValueError:
            pass
    raise AssertionError(f"no alias stream of at most {fx.stream.size} bytes for {fx}")


def check_slots(read_bytes, slots, used, size, what=""):
    """The output side.  read_bytes(start, stop) returns bytes [start, stop) of an output buffer of `size` bytes that was
    filled with the sentinel; slots: (byte offset, wanted bytes) of every checked row; everything from `used` on must
    still hold the sentinel.  A slot written at a narrowed offset leaves sentinel bytes (or another row's) in its place."""
    for k, (off, want) in enumerate(slots):
        want = np.asarray(want, dtype=np.uint8)
        got = np.asarray(read_bytes(off, off + want.size)).view(np.uint8).ravel()
        diff = np.flatnonzero(got != want)
        assert diff.size == 0, (f"{what}: slot {k} at byte {off}: {diff.size} of {want.size} bytes differ, first at "
                                f"{diff[:4].tolist()}" + (" (the slot still holds the sentinel)" if (got == SENTINEL).all() else ""))
    check_guard(read_bytes, used, size, what)


def check_guard(read_bytes, start, stop, what="", step=1 << 28):
    """Bytes [start, stop) still hold the sentinel."""
    for s in range(int(start), int(stop), step):
        raw = np.asarray(read_bytes(s, min(s + step, int(stop)))).view(np.uint8).ravel()
        bad = np.flatnonzero(raw != SENTINEL)
        assert bad.size == 0, f"{what}: byte {s + int(bad[0])} behind the {int(start)} bytes used was written ({bad.size} bytes)"
