"""Complex-packed GRIB-2 cases whose missing values are coded inside the groups (section 5's octet 23, missing value
management m = 1 or 2), shared by tests/test_grib_complex_mv.py and tests/test_gpu_grib_complex_mv.py.  Plain numpy, no
GPU, nothing of the product's parser; the bit helpers and the message writer are those of tests/complex_cases.py.

THE RULE (the template text, g2c's comunpack as recalled).  N coded positions, groups of width w_g and reference r_g,
stored values s_i; every comparison in 64 bits.
    w_g > 0    position i is missing iff s_i == 2^w_g - 1, or m == 2 and s_i == 2^w_g - 2; else z = r_g + s_i
    w_g == 0   the whole group is missing iff r_g == 2^nbits - 1, or m == 2 and r_g == 2^nbits - 2; else z = r_g
    the present values in order form c_0 .. c_(P-1); spatial differencing is undone over that sequence: the `order`
    placeholders are the first `order` present values; X_0 = h_1, X_1 = h_2 whatever P is.

THE HAND-ASSEMBLED ROW (tests/golden/complex_mv/hand_mvm1.grib2): 5 x 2 cells, m = 1, order 1, n_oct = 1, three groups
of 4, 3 and 3 positions, R = E = D = 0.
    present X          20 23 . 25 | 24 30 . | . . .       positions 2, 6, 7, 8, 9 missing; P = 5
    first differences  3 2 -1 6, so g = -1 and c = (0) 4 3 0 7
    group 0            ref 0, width 3, stored 0 4 7* 3
    group 1            ref 0, width 4, stored 0 7 15*
    group 2            width 0, ref 3 = 2^2 - 1: the whole group is missing
    section 5, octets 20 - 49   02 00 01 01  00000000 00000000  00000003  00 03  00000003 01 00000003 01  01 01
    section 7 from octet 6      14 81 | 0C | 70 00 | 80 | 13 B0 7F
    device bitmap               DC 00
    compacted stream, width 5   A5 F3 8F 00
"""
import os

import numpy as np

from tests.ccsds_cases import _sm, pack_bits
from tests.complex_cases import PARAM_NAMES, _bits, _smooth, _table, bit_length, even, grib2_message, record, section5

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "complex_mv")
S = 2048
HAND_X = np.array([20, 23, 25, 24, 30], dtype=np.int64)
HAND_PRESENT = np.array([1, 1, 0, 1, 1, 1, 0, 0, 0, 0], dtype=bool)
HAND_LENGTHS = [4, 3, 3]
HAND_STREAM = bytes.fromhex("1481" "0C" "7000" "80" "13B07F")
HAND_S5 = bytes.fromhex("02000101" "00000000" "00000000" "00000003" "0003" "00000003" "01" "00000003" "01" "0101")
HAND_BITMAP = bytes.fromhex("DC00")
HAND_COMPACT = bytes.fromhex("A5F38F00")


def encode(X, present, m, order, lengths, n_oct=2, widths=None, nbits=None, kinds=None):
    """(stream: uint8 array, params: dict of PARAM_NAMES) of a row of present.size positions whose present ones hold the
    integers X in order.  A group's width is widened until its largest z - ref stays below the codes it reserves
    (2^w - 1, under m == 2 also 2^w - 2); a group with no present position gets width 0 and a missing reference unless
    `widths` ({group: width}) gives it one.  kinds: per position 1 or 2, which code a missing one carries (2 only under
    m == 2; default: alternating under m == 2).  nbits: the width of the references when not the smallest that keeps a
    present reference off the codes."""
    X, present = np.asarray(X, dtype=np.int64), np.asarray(present, dtype=bool)
    N, P = present.size, int(present.sum())
    assert X.size == P and sum(lengths) == N and m in (1, 2)
    if kinds is None:
        kinds = 1 + (np.arange(N) % 2) * (m == 2)
    kinds = np.asarray(kinds)
    heads, g, zc = [0] * order, 0, np.zeros(P, dtype=np.int64)
    if order == 0:
        zc = X.copy()
    else:
        heads = [int(v) for v in X[:order]] + [0] * max(order - P, 0)
        if P > order:
            d = X[1:] - X[:-1] if order == 1 else X[2:] - 2 * X[1:-1] + X[:-2]
            g = int(d.min())
            zc[order:] = d - g
    z = np.zeros(N, dtype=np.int64)
    z[present] = zc
    ends = np.cumsum(lengths)
    starts = ends - np.asarray(lengths)
    widths = dict(widths or {})
    reserve = 1 if m == 1 else 2
    refs, ws, empty = [], [], []
    for k, (a, b) in enumerate(zip(starts, ends)):
        here = present[a:b]
        if not here.any():
            refs.append(None)
            ws.append(int(widths.get(k, 0)))
            empty.append(k)
            continue
        part = z[a:b][here]
        ref, span = int(part.min()), int(part.max() - part.min())
        w = 0 if span == 0 and here.all() else 1
        while w and span > (1 << w) - 1 - reserve:
            w += 1
        w = max(w, int(widths.get(k, 0)))
        assert w <= 32
        refs.append(ref)
        ws.append(w)
    top = max([r for r in refs if r is not None], default=-1)
    if nbits is None:
        nbits = 1
        while top >= (1 << nbits) - 2:
            nbits += 1
    stored = np.zeros(N, dtype=np.int64)
    for k, (a, b) in enumerate(zip(starts, ends)):
        code = lambda w, kind: (1 << w) - kind          # noqa: E731  (kind 1: 2^w - 1; kind 2: 2^w - 2)
        if refs[k] is None:
            kind = int(kinds[a])
            refs[k] = max(code(nbits, kind), 0) if ws[k] == 0 else 0
            assert ws[k] > 0 or nbits > 0 or kind == 1
        seg = np.where(present[a:b], z[a:b] - refs[k], [code(ws[k], int(q)) for q in kinds[a:b]])
        stored[a:b] = seg if ws[k] else 0
    lengths = [int(v) for v in lengths]
    p = dict(n_groups=len(lengths), order=order, n_oct=n_oct if order else 0, length_inc=1, length_last=lengths[-1], nbits=nbits)
    p["width_ref"] = min(ws)
    p["width_bits"] = bit_length(max(ws) - p["width_ref"])
    inner = lengths[:-1]
    p["length_ref"] = min(inner) if inner else lengths[-1]
    scaled = [v - p["length_ref"] for v in inner] + [0]
    p["length_bits"] = bit_length(max(scaled))
    assert all(abs(v) < 1 << (8 * n_oct - 1) for v in heads + [g]) and bit_length(max(refs)) <= nbits
    head = b"".join(_sm(v, n_oct) for v in heads + [g]) if order else b""
    per_w = np.repeat(np.asarray(ws, dtype=np.int64), lengths)
    data = np.packbits(_bits(stored, per_w, int(per_w.sum()))).tobytes()
    stream = head + _table(refs, nbits) + _table([w - p["width_ref"] for w in ws], p["width_bits"]) + \
        _table(scaled, p["length_bits"]) + data
    return np.frombuffer(stream, dtype=np.uint8).copy(), p


def numpy_decode(stream, n_values, p, m):
    """(the present integers X in order: int64, present: bool per position) of a stream, by THE RULE above."""
    bits = np.unpackbits(np.asarray(stream, dtype=np.uint8))
    ng, order, n_oct = p["n_groups"], p["order"], p["n_oct"]

    def number(at, width):
        v = 0
        for b in bits[at:at + width]:
            v = (v << 1) | int(b)
        return v

    def signed(at):
        v, sign = number(at, 8 * n_oct), 1 << (8 * n_oct - 1)
        return -(v & (sign - 1)) if v & sign else v
    pos = 8 * n_oct * (order + 1) if order else 0
    heads = [signed(8 * n_oct * k) for k in range(order)]
    g = signed(8 * n_oct * order) if order else 0
    tables = []
    for width in (p["nbits"], p["width_bits"], p["length_bits"]):
        tables.append([number(pos + k * width, width) for k in range(ng)])
        pos += (ng * width + 7) // 8 * 8
    refs = tables[0]
    ws = [p["width_ref"] + v for v in tables[1]]
    ls = [p["length_ref"] + p["length_inc"] * v for v in tables[2]]
    ls[-1] = p["length_last"]
    assert sum(ls) == n_values
    present, c = [], []
    for r, w, n in zip(refs, ws, ls):
        for _ in range(n):
            s = number(pos, w)
            pos += w
            v, top = (s, (1 << w) - 1) if w > 0 else (r, (1 << p["nbits"]) - 1)
            gone = v == top or (m == 2 and v == top - 1)
            present.append(not gone)
            if not gone:
                c.append(r + s)
    P = len(c)
    X = np.zeros(P, dtype=np.int64)
    for k in range(P):
        if order == 0:
            X[k] = c[k]
        elif k == 0:
            X[k] = heads[0]
        elif order == 1:
            X[k] = X[k - 1] + c[k] + g
        elif k == 1:
            X[k] = heads[1]
        else:
            X[k] = 2 * X[k - 1] - X[k - 2] + c[k] + g
    return X, np.array(present, dtype=bool)


class Case:
    def __init__(self, name, X, present, m, order, lengths, **kw):
        self.name, self.m, self.order = name, m, order
        self.present = np.asarray(present, dtype=bool)
        self.X = np.asarray(X, dtype=np.int64)
        self.stream, self.params = encode(self.X, self.present, m, order, lengths, **kw)
        self.n_values, self.P = int(self.present.size), int(self.present.sum())
        self.width = bit_length(int(self.X.max())) if self.P else 0
        self.bitmap = np.packbits(self.present.astype(np.uint8))
        self.bitmap_slot = np.concatenate([self.bitmap, np.zeros(-self.bitmap.size % 4, np.uint8)])
        packed = pack_bits(self.X, self.width) if self.P and self.width else np.zeros(0, np.uint8)
        self.packed = np.concatenate([packed, np.zeros(-packed.size % 4, np.uint8)])    # rounded up to 4 with zero bytes

    def record(self, byte_off):
        return record(byte_off, self.stream.size, self.n_values, self.params)

    def __repr__(self):
        return self.name


def _mask(n, frac, seed):
    return np.random.default_rng(seed).random(n) >= frac


def _runs(n, *runs):
    present = np.ones(n, dtype=bool)
    for a, b in runs:
        present[a:b] = False
    return present


_CASES = []


def cases():
    """Every case, built once: 2048 positions unless the name says otherwise, each with m = 1 and m = 2."""
    if _CASES:
        return list(_CASES)
    c = _CASES.append
    n = S
    c(Case("hand_m1", HAND_X, HAND_PRESENT, 1, 1, HAND_LENGTHS, n_oct=1))
    for m in (1, 2):
        t = f"_m{m}"
        rng = np.random.default_rng(40 + m)
        third = _mask(n, 0.3, m)
        c(Case("order0_third" + t, rng.integers(0, 4096, int(third.sum())), third, m, 0, even(n, 64)))
        c(Case("order1_third" + t, _smooth(int(third.sum()), 1, 0.002, 12), third, m, 1, even(n, 40)))
        c(Case("order2_third" + t, _smooth(int(third.sum()), 2, 0.0005, 16), third, m, 2, even(n, 64), n_oct=3))
        c(Case("order2_none_missing" + t, _smooth(n, 3, 0.0005, 16), np.ones(n, bool), m, 2, even(n, 64), n_oct=3))
        c(Case("all_missing_nbits0" + t, [], np.zeros(n, bool), m, 1, even(n, 16), nbits=0, kinds=np.ones(n, int)))
        c(Case("all_missing_nbits5" + t, [], np.zeros(n, bool), m, 2, even(n, 16), nbits=5))
        one = np.zeros(n, bool)
        one[777] = True
        c(Case("order2_P1" + t, [12345], one, m, 2, even(n, 32), n_oct=3))
        two = one.copy()
        two[1500] = True
        c(Case("order2_P2" + t, [12345, 999], two, m, 2, even(n, 32), n_oct=3))
        late = _runs(n, (0, 3))
        c(Case("order2_first3_missing" + t, _smooth(n - 3, 4, 0.0005, 16), late, m, 2, even(n, 64), n_oct=3))
        edges = _runs(n, (250, 261), (1020, 1031))
        c(Case("order1_edge_runs" + t, _smooth(int(edges.sum()), 5, 0.002, 14), edges, m, 1, even(n, 50)))
        # group 3 (32 positions) has no present position and width 1: under m == 2 both stored values are codes
        w1 = _runs(n, (96, 128))
        c(Case("order0_width1_group" + t, rng.integers(0, 500, int(w1.sum())), w1, m, 0, even(n, 64), widths={3: 1}))
        # group 0 is 32 bits wide: its missing positions carry 0xFFFFFFFF (and 0xFFFFFFFE), its present ones up to 2^32 - 3
        w32 = _runs(n, (5, 9), (40, 50))
        big = rng.integers(0, 1000, int(w32.sum()))
        big[:20] = rng.integers(0, 2 ** 32 - 2, 20)
        big[3] = 2 ** 32 - 3
        c(Case("order0_width32_group" + t, big, w32, m, 0, even(n, 64), widths={0: 32}))
        # groups 0 and 1 of width 0: one present (a constant), one missing
        w0 = _runs(n, (32, 64))
        flat = rng.integers(0, 300, int(w0.sum()))
        flat[:32] = 77
        c(Case("order0_width0_present_and_missing" + t, flat, w0, m, 0, even(n, 64)))
        short = _mask(1500, 0.3, 10 + m)
        c(Case("short1500_order2" + t, _smooth(int(short.sum()), 6, 0.001, 16), short, m, 2, even(1500, 47), n_oct=3))
        large = _mask(70000, 0.3, 20 + m)
        c(Case("big70000_order2" + t, _smooth(int(large.sum()), 7, 0.0002, 16), large, m, 2, even(70000, 1500), n_oct=3))
    return list(_CASES)


def case(name):
    return next(k for k in cases() if k.name == name)


def hand_message():
    c = case("hand_m1")
    return grib2_message([dict(cpx=(c.stream, c.params, 10), s5=section5(10, c.params, mvm=1))], 5, 2)


def build(cs, seed=1):
    """The rows `cs` as one call (buf, rows, cpx, missing) and as its simple-packed twin (buf, rows, bitmaps): the
    compacted integers at their own width plus the bitmap.  Streams lie at odd offsets with garbage between them."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE
    from tests.ccsds_cases import rules
    rows = rules(len(cs), seed)
    twin_rows = rows.copy()
    cpx = np.zeros(len(cs), dtype=GRIB_CPX_DTYPE)
    bms = np.zeros(len(cs), dtype=GRIB_BITMAP_DTYPE)
    parts, twin_parts = [], []

    def put(store, data):
        at = sum(p.size for p in store) + 3
        store.extend([np.full(3, 0xA5, np.uint8), np.asarray(data, np.uint8)])
        return at
    for i, c in enumerate(cs):
        rows["nbits"][i], twin_rows["nbits"][i] = c.params["nbits"], c.width
        rows["byte_off"][i] = off = put(parts, c.stream)
        cpx[i] = c.record(off)
        twin_rows["byte_off"][i] = put(twin_parts, c.packed)
        bms["bitmap_off"][i], bms["n_values"][i] = put(twin_parts, c.bitmap), c.P
    missing = np.array([c.m for c in cs], dtype=np.uint8)
    return (np.concatenate(parts), rows, cpx, missing), (np.concatenate(twin_parts), twin_rows, bms)
