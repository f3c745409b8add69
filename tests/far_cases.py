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
2^12 on buffers of a few thousand elements."""
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
