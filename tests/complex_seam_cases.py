"""Complex-packed rows that sit on the seams of the decode kernels (smm_grib_cpx_unpack / _mv: tiles of 256 groups, tiles
of 1024 values, blocks of 256 positions, carries scanned 64 parts at a step, the two-level search from a value to its
group) and rows that must be refused with a status, shared by tests/test_grib_complex_seams.py and
tests/test_gpu_grib_complex_seams.py.  Plain numpy and Python integers, no GPU and no product code.

THE REFERENCE (`tables`, `reference`) is a scalar decoder written from the header text of smm_grib_cpx.hpp -- THE FORMAT,
MISSING VALUES INSIDE THE GROUPS and the five lines of A ROW ENDS AS in their order -- in Python integers, reduced mod
2^64 where the text says so.  It shares nothing with complex_cases.numpy_decode: it reads one number at a time from the
bytes, gives a status for every row and takes rows of n_values <= order.  What a case expects -- status, integers,
bitmap, the simple-packed twin -- is what the reference gives for the case's bytes; the builders' own integers are
compared with it in the CPU tests.

THE FAMILIES (`family("A")` .. `family("H")`, each with a census in tests/test_grib_complex_seams.py)
    A  group tiles: NG at 255 / 256 / 257, 511 / 512 / 513 and around 64 tiles of groups; lengths 1..3, widths that differ
       from group to group
    B  value tiles: n_values around 256, 1024, 2048 and 64 tiles of values at orders 0, 1, 2; first and second
       differences that are not zero at any block or tile edge; long rows whose first differences stay negative from
       value 30000 on, so that the tile sums and carries of the prefix sums are wrapped uint64
    C  groups of no values, at orders 0 and 2 and under missing value management 0, 1 and 2
    D  every width 1..32 at every bit phase 0..31 of a 32-bit word of the call's buffer
    E  descriptors: n_oct 1..4, g negative, zero, "minus zero" and at +-(2^(8 n_oct - 1) - 1), h_1 "minus zero";
       rows whose present values are fewer than, as many as and one more than the order; rows of n_values <= order
       (`refused`: check_grib_cpx turns them away at every entry, they reach the scalar decoder through the harness only)
    F  X == 2^32 - 1 (ok), 2^32 and -1 (invalid) at exactly one value: the last of a tile, the first of a tile, the last of
       the row in a partial wave, in tile 65
    G  rows with missing values at the seams of the blocks of 256 positions and of the ballot's two halves
    H  malformed rows, each with the status it must end with (`want`)
"""
import numpy as np

from tests import complex_cases as xc
from tests import complex_mv_cases as mv
from tests.ccsds_cases import pack_bits

OK, EXHAUSTED, INVALID = 0, 1, 2
STATUS_NAMES = {OK: "ok", EXHAUSTED: "exhausted", INVALID: "invalid"}
M64 = (1 << 64) - 1
TWO32 = 1 << 32
GROUP_TILE, VALUE_TILE, BLOCK, STEP = 256, 1024, 256, 64


# ------------------------------------------------------------------------------------------------ the reference
def _peek(stream, pos, n):
    """The n bits at bit `pos` of the bytes `stream`, MSB first."""
    if n <= 0:
        return 0
    b0, b1 = pos >> 3, (pos + n + 7) >> 3
    assert b1 <= len(stream), "the reference reads nothing that a status has not let through"
    return (int.from_bytes(stream[b0:b1], "big") >> (8 * b1 - pos - n)) & ((1 << n) - 1)


def _signed(v, n_oct):
    sign = 1 << (8 * n_oct - 1)
    return -(v & (sign - 1)) if v & sign else v & (sign - 1)


def tables(stream, n_values, p):
    """The first four lines of A ROW ENDS AS: a dict with `status` and, as far as the row got, where its parts begin
    (`refs_bit`, `widths_bit`, `lengths_bit`, `data_bit`: bit positions in the stream), `ws`, `ls`, `refs`, `h` (h_1,
    h_2) and `g`."""
    stream = np.asarray(stream, dtype=np.uint8).tobytes()
    n, ng, order, n_oct = int(n_values), int(p["n_groups"]), int(p["order"]), int(p["n_oct"])
    t = dict(status=OK, bytes=stream)
    if ng > n:
        return dict(t, status=INVALID)
    head = (order + 1) * n_oct if order > 0 else 0
    sizes = [(ng * int(p[k]) + 7) // 8 for k in ("nbits", "width_bits", "length_bits")]
    if head + sum(sizes) > len(stream):
        return dict(t, status=EXHAUSTED)
    t["refs_bit"] = 8 * head
    t["widths_bit"] = t["refs_bit"] + 8 * sizes[0]
    t["lengths_bit"] = t["widths_bit"] + 8 * sizes[1]
    t["data_bit"] = t["lengths_bit"] + 8 * sizes[2]
    wb, lb = int(p["width_bits"]), int(p["length_bits"])
    t["ws"] = [int(p["width_ref"]) + _peek(stream, t["widths_bit"] + g * wb, wb) for g in range(ng)]
    t["ls"] = [int(p["length_ref"]) + int(p["length_inc"]) * _peek(stream, t["lengths_bit"] + g * lb, lb) for g in range(ng - 1)]
    if ng:
        t["ls"].append(int(p["length_last"]))
    if any(w > 32 for w in t["ws"]) or any(v > n for v in t["ls"]) or sum(t["ls"]) != n:
        return dict(t, status=INVALID)
    if sum(w * v for w, v in zip(t["ws"], t["ls"])) > 8 * len(stream) - t["data_bit"]:
        return dict(t, status=EXHAUSTED)
    nb = int(p["nbits"])
    t["refs"] = [_peek(stream, t["refs_bit"] + g * nb, nb) for g in range(ng)]
    d = [_signed(_peek(stream, 8 * n_oct * k, 8 * n_oct), n_oct) for k in range(order + 1)] if order > 0 else []
    t["h"], t["g"] = (d[:order] + [0, 0])[:2], d[order] if order > 0 else 0
    return t


def reference(stream, n_values, p, m=0):
    """(status, X) of a row without missing value management, (status, X, present) of a row with m = 1 or 2: X the
    integers as Python ints (n_values of them, the P present ones under m), present a bool per position.  Not ok: the
    integers are zero (none under m) and no position is present."""
    n, order, nbits = int(n_values), int(p["order"]), int(p["nbits"])
    if n == 0:
        return (OK, []) if m == 0 else (OK, [], [])
    t = tables(stream, n, p)
    failed = lambda status: (status, [0] * n) if m == 0 else (status, [], [False] * n)          # noqa: E731
    if t["status"] != OK:
        return failed(t["status"])
    stream, (h1, h2), g = t["bytes"], t["h"], t["g"]
    X, present, pos, x1, x2 = [], [], t["data_bit"], 0, 0
    for ref, w, length in zip(t["refs"], t["ws"], t["ls"]):
        for _ in range(length):
            s = _peek(stream, pos, w)
            pos += w
            if m:
                v, top = (s, (1 << w) - 1) if w > 0 else (ref, (1 << nbits) - 1)
                gone = v == top or (m == 2 and v == top - 1)          # 2^0 - 2 is negative here: it matches nothing
                present.append(not gone)
                if gone:
                    continue
            k, z = len(X), ref + s
            if order == 0:
                x = z
            elif k == 0:
                x = h1
            elif order == 1:
                x = x1 + z + g
            elif k == 1:
                x = h2
            else:
                x = 2 * x1 - x2 + z + g
            x &= M64
            x2, x1 = x1, x
            X.append(x)
    if any(x >> 32 for x in X):
        return failed(INVALID)
    return (OK, X) if m == 0 else (OK, X, present)


# ------------------------------------------------------------------------------------------------ a case
class Seam:
    """A row: its bytes, its record's parameters, its missing value management and what its builder meant (`meant_X`,
    `meant_present`, `want`: None where the builder says nothing).  Everything a test compares with -- status, X,
    present, P, width, the simple-packed twin `packed`, `bitmap`, `bitmap_slot` -- is the reference's."""

    def __init__(self, name, stream, params, n_values, m=0, X=None, present=None, want=None, refused=False, **notes):
        self.name, self.family, self.m, self.order = name, name[0], int(m), int(params["order"])
        self.stream = np.ascontiguousarray(stream, dtype=np.uint8)
        self.params, self.n_values = {k: int(params[k]) for k in xc.PARAM_NAMES}, int(n_values)
        self.meant_X = None if X is None else [int(v) for v in X]
        self.meant_present = None if present is None else np.asarray(present, dtype=bool)
        self.want, self.refused, self.notes = want, refused, notes
        self._got = None

    def _decoded(self):
        if self._got is None:
            got = reference(self.stream, self.n_values, self.params, self.m)
            status, X = got[0], np.array(got[1], dtype=np.uint64).astype(np.int64) if got[0] == OK else np.zeros(len(got[1]), np.int64)
            present = np.array(got[2], dtype=bool) if self.m else np.full(self.n_values, status == OK)
            self._got = (status, X, present)
        return self._got

    status = property(lambda self: self._decoded()[0])
    X = property(lambda self: self._decoded()[1])
    present = property(lambda self: self._decoded()[2])
    P = property(lambda self: int(self.X.size) if self.m else (self.n_values if self.status == OK else 0))
    width = property(lambda self: xc.bit_length(int(self.X.max())) if self.X.size else 0)

    @property
    def bitmap(self):
        return np.packbits(self.present.astype(np.uint8))

    @property
    def bitmap_slot(self):
        return np.concatenate([self.bitmap, np.zeros(-self.bitmap.size % 4, np.uint8)])

    @property
    def packed(self):
        packed = pack_bits(self.X, self.width) if self.X.size and self.width else np.zeros(0, np.uint8)
        return np.concatenate([packed, np.zeros(-packed.size % 4, np.uint8)])

    def tables(self):
        return tables(self.stream, self.n_values, self.params)

    def record(self, byte_off):
        return xc.record(byte_off, self.stream.size, self.n_values, self.params)

    def __repr__(self):
        return self.name


def patched(stream, bit, width, value):
    """A copy of the stream with the `width` bits at `bit` holding `value`."""
    out = np.array(stream, dtype=np.uint8)
    for b in range(width):
        at, one = bit + b, (int(value) >> (width - 1 - b)) & 1
        out[at >> 3] = (int(out[at >> 3]) & ~(0x80 >> (at & 7)) & 0xFF) | (one * (0x80 >> (at & 7)))
    return out


def assemble(order, n_oct, descriptors, refs, ws, ls, stored, nbits=None, width_bits=None, length_bits=None):
    """(stream, params) from the numbers themselves, for what the encoders of complex_cases / complex_mv_cases assert
    away.  descriptors: h_1 .. h_order, g as (sign bit, magnitude)."""
    refs, ws, ls = [int(v) for v in refs], [int(v) for v in ws], [int(v) for v in ls]
    head = b"".join((((1 << (8 * n_oct - 1)) if neg else 0) | int(mag)).to_bytes(n_oct, "big") for neg, mag in descriptors) if order else b""
    assert len(descriptors) == (order + 1 if order else 0)
    p = dict(n_groups=len(ls), order=order, n_oct=n_oct if order else 0, length_inc=1, length_last=ls[-1])
    p["nbits"] = xc.bit_length(max(refs)) if nbits is None else nbits
    p["width_ref"] = min(ws)
    p["width_bits"] = xc.bit_length(max(ws) - min(ws)) if width_bits is None else width_bits
    inner = ls[:-1]
    p["length_ref"] = min(inner) if inner else ls[-1]
    scaled = [v - p["length_ref"] for v in inner] + [0]
    p["length_bits"] = xc.bit_length(max(scaled)) if length_bits is None else length_bits
    per_w = np.repeat(np.asarray(ws, dtype=np.int64), ls)
    data = np.packbits(xc._bits(stored, per_w, int(per_w.sum()))).tobytes()
    stream = head + xc._table(refs, p["nbits"]) + xc._table([w - p["width_ref"] for w in ws], p["width_bits"]) + \
        xc._table(scaled, p["length_bits"]) + data
    return np.frombuffer(stream, dtype=np.uint8).copy(), p


def integrate(a, order, h):
    """X (Python ints, not reduced) from a_i = z_i + g for i >= order and the first values h."""
    X = [int(v) for v in h[:order]][:len(a)]
    for i in range(len(X), len(a)):
        X.append(int(a[i]) if order == 0 else X[-1] + int(a[i]) if order == 1 else 2 * X[-1] - X[-2] + int(a[i]))
    return X


# ------------------------------------------------------------------------------------------------ A: group tiles
A_GROUPS = [255, 256, 257, 511, 512, 513, STEP * GROUP_TILE - 1, STEP * GROUP_TILE, STEP * GROUP_TILE + 1, (STEP + 1) * GROUP_TILE + 1]


def _uneven_row(ng, seed, order):
    """ng groups of 1..3 values whose widths 1..11 differ from one group to the next; order 0 or 1."""
    rng = np.random.default_rng(seed)
    ls = rng.integers(1, 4, ng)
    ws = 1 + (np.arange(ng) * 5 + seed) % 11
    z = rng.integers(0, np.int64(1) << np.repeat(ws, ls)) + np.repeat(rng.integers(0, 5000, ng), ls)
    if order == 0:
        return z, ls, ws
    z[7] = 0                                        # the smallest z of all: g is the encoder's own
    X = (1 << 24) + np.cumsum(z - int(z.mean()))
    return X, ls, ws + 13                           # a reference moves a group's values: 13 bits more hold any of them


def family_a():
    out = []
    for k, ng in enumerate(A_GROUPS):
        order = k % 2
        X, ls, ws = _uneven_row(ng, 100 + k, order)
        stream, p = xc.encode(X, order, ls, n_oct=4, widths=[int(w) for w in ws])
        out.append(Seam(f"A_ng{ng}_order{order}", stream, p, X.size, X=X))
    return out


# ------------------------------------------------------------------------------------------------ B: value tiles
B_SIZES = [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 65535, 65536, 65537, 66561]
B_TURN = 30000           # a long row climbs up to here and falls from here on


def b_values(n, seed):
    rng = np.random.default_rng(seed)
    step = rng.integers(1, 10, n)
    for e in range(BLOCK, n, BLOCK):               # 2, 5, 3 around every edge: no first or second difference is zero there
        step[e - 1:e + 2] = (2, 5, 3)[:len(step[e - 1:e + 2])]
    if n > 2 * B_TURN:
        step[B_TURN:] *= -1
    return 200000 + np.cumsum(step)


def family_b():
    out = []
    for k, n in enumerate(B_SIZES):
        X = b_values(n, 200 + k)
        for order in (0, 1, 2):
            if n <= order:
                continue                            # family E's
            stream, p = xc.encode(X, order, xc.even(n, max(1, n // 37)), n_oct=3)
            out.append(Seam(f"B_n{n}_order{order}", stream, p, n, X=X))
    return out


# ------------------------------------------------------------------------------------------------ C: groups of no values
C_LENGTHS = {
    "first_two": [0, 0, 350] + [0] * 254 + [350],                     # and groups 3..256 empty: across the first seam
    "last_zero": [3] + [0] * 270 + [657] + [0] * 5 + [40] + [0] * 3,  # length_last == 0
    "whole_tile": [2] * 256 + [0] * 256 + [3] * 10,                   # tile 1 holds no value
    "straddle": [2] * 250 + [0] * 13 + [3] * 20,                      # groups 250..262
    "forced": [5, 0, 0, 300] + [0] * 252 + [0, 0, 200, 0],            # empty groups with a width and a reference
    "beside_width0": [4, 5, 0, 5, 0, 0, 6, 4, 0],                     # groups 1 and 3 have width 0
    # 2048 values, the gather's row: groups 250..262 and the whole of tile 2 are empty
    "gather": [0, 8] + [4] * 248 + [0] * 13 + [4] * 237 + [5] * 12 + [0] * 256 + [8] * 5 + [0],
}
C_FLAT = {"beside_width0": (1, 3)}


def c_row(name, order, m, seed):
    ls = C_LENGTHS[name]
    n = sum(ls)
    rng = np.random.default_rng(seed)
    starts = np.cumsum(ls) - np.asarray(ls)
    flat = [(int(starts[g]), int(starts[g]) + ls[g]) for g in C_FLAT.get(name, ())]
    present = np.ones(n, dtype=bool)
    if m:
        present = rng.random(n) >= 0.25
        present[:2] = True
        for a, b in flat:
            present[a - 2:b] = True                 # a group of width 0 has every position present
    P = int(present.sum())
    X = rng.integers(0, 4096, P) if order == 0 else xc._smooth(P, seed, 0.0005, 16)
    rank = np.cumsum(present) - present
    for a, b in flat:
        ra, rb = int(rank[a]), int(rank[b - 1]) + 1
        if order == 0:
            X[ra:rb] = X[ra]
        else:
            X[ra - 2:rb] = X[ra - 2] + 3 * np.arange(rb - ra + 2)         # linear: its second differences are one number
    empty = [g for g, v in enumerate(ls) if v == 0]
    if m:
        kinds = np.ones(n + 1, dtype=np.int64) + (np.arange(n + 1) % 2) * (m == 2)       # (one more: a last group may be empty)
        widths = {g: 3 + g % 5 for g in empty} if name == "forced" else None
        stream, p = mv.encode(X, present, m, order, ls, n_oct=3, widths=widths, kinds=kinds)
    else:
        stream, p = xc.encode(X, order, ls, n_oct=3)
        if name == "forced":
            ws = tables(stream, n, p)["ws"]
            stream, p = xc.encode(X, order, ls, n_oct=3, widths=[3 + g % 5 if ls[g] == 0 else w for g, w in enumerate(ws)])
    if name == "forced":                            # references of all ones in the empty groups
        t = tables(stream, n, p)
        for g in empty:
            stream = patched(stream, t["refs_bit"] + g * p["nbits"], p["nbits"], (1 << p["nbits"]) - 1)
    return Seam(f"C_{name}_order{order}_m{m}", stream, p, n, m=m, X=X, present=present if m else None)


def family_c():
    return [c_row(name, order, m, 300 + 7 * k + m) for k, name in enumerate(C_LENGTHS) for order in (0, 2) for m in (0, 1, 2)]


# ------------------------------------------------------------------------------------------------ D: width x phase
def family_d():
    """Four rows of eight widths each.  A width's 32 groups of four values -- all ones, the top bit alone, zero, anything
    -- alternate with 32 groups of one value in one bit: 4 w + 1 is odd, so the 32 pairs begin at 32 different phases
    wherever the row's bits begin."""
    out = []
    for k in range(4):
        rng = np.random.default_rng(400 + k)
        X, ls, ws = [], [], []
        for w in range(8 * k + 1, 8 * k + 9):
            for _ in range(32):
                X += [(1 << w) - 1, 1 << (w - 1), 0, int(rng.integers(0, 1 << w)), int(rng.integers(0, 2))]
                ls += [4, 1]
                ws += [w, 1]
        stream, p = xc.encode(X, 0, ls, widths=ws)
        out.append(Seam(f"D_w{8 * k + 1}_to_{8 * k + 8}", stream, p, len(X), X=X))
    return out


# ------------------------------------------------------------------------------------------------ E: descriptors
def e_row(name, order, n_oct, g, h1_minus_zero=False, seed=0):
    """g: (sign bit, magnitude).  a_i = z_i + g in 0..3 above max(g, 0): X climbs; as many values as stay below 2^32."""
    rng = np.random.default_rng(500 + seed)
    gval, n = (-g[1] if g[0] else g[1]), 40
    h = [0 if h1_minus_zero else 100, 103][:order]
    while True:
        a = rng.integers(0, 4, n) + max(gval, 0)
        X = integrate(a, order, h)
        if max(X) < TWO32 or n == order + 1:
            break
        n = max(n // 2, order + 1)
    z = a - gval
    ls = xc.even(n, min(3, n))
    refs = [int(z[s - v:s].min()) for s, v in zip(np.cumsum(ls), ls)]
    ws = [xc.bit_length(int(z[s - v:s].max()) - r) for s, v, r in zip(np.cumsum(ls), ls, refs)]
    descr = [(h1_minus_zero and k == 0, v) for k, v in enumerate(h)] + [g]
    stream, p = assemble(order, n_oct, descr, refs, ws, ls, z - np.repeat(refs, ls))
    return Seam(name, stream, p, n, X=X, g=g, h1_minus_zero=h1_minus_zero)


def family_e():
    out = []
    for n_oct in (1, 2, 3, 4):
        top = (1 << (8 * n_oct - 1)) - 1
        for order in (1, 2):
            for what, g in (("neg", (True, 5)), ("zero", (False, 0)), ("minus_zero", (True, 0)), ("plus_top", (False, top)),
                            ("minus_top", (True, top))):
                out.append(e_row(f"E_noct{n_oct}_order{order}_g_{what}", order, n_oct, g, seed=len(out)))
            out.append(e_row(f"E_noct{n_oct}_order{order}_h1_minus_zero", order, n_oct, (True, 2), h1_minus_zero=True, seed=len(out)))
    # n_values <= order: the stored values are placeholders, read past; h_1 = 77, h_2 = 80, g = -3
    for n, order in ((1, 1), (1, 2), (2, 2)):
        descr = [(False, 77), (False, 80)][:order] + [(True, 3)]
        stream, p = assemble(order, 2, descr, [5], [3], [n], [6, 1][:n])
        out.append(Seam(f"E_n{n}_order{order}_plain", stream, p, n, X=[77, 80][:n], refused=True))
    rng = np.random.default_rng(599)
    for m in (1, 2):
        for n, order in ((1, 1), (1, 2), (2, 2)):                          # the same three with codes inside: every P
            for P in range(n + 1):
                present = np.arange(n) < P
                X = [77, 80][:P]
                stream, p = mv.encode(X, present, m, order, [n], kinds=np.ones(n + 1, dtype=np.int64))
                out.append(Seam(f"E_n{n}_order{order}_P{P}_m{m}", stream, p, n, m=m, X=X, present=present, refused=True))
        for order in (1, 2):                                               # P below, at and one above the order
            for P in (order - 1, order, order + 1):
                present = np.zeros(8, dtype=bool)
                present[rng.permutation(8)[:P]] = True
                X = [int(v) for v in rng.integers(0, 120, P)]
                stream, p = mv.encode(X, present, m, order, [3, 5], n_oct=2)
                out.append(Seam(f"E_n8_order{order}_P{P}_m{m}", stream, p, 8, m=m, X=X, present=present))
    return out


# ------------------------------------------------------------------------------------------------ F: range
F_SMALL, F_BIG = 1500, 66700                                              # 1499 is lane 27 of a wave; 66600 lies in tile 65
F_PLACES = {"tile_last": (F_SMALL, 1023), "tile_first": (F_SMALL, 1024), "row_last": (F_SMALL, F_SMALL - 1), "tile65": (F_BIG, 66600)}
F_KINDS = {"top": (TWO32 - 1, OK), "over": (TWO32, INVALID), "under": (-1, INVALID)}


def f_values(n, k, kind, seed):
    """X with F_KINDS[kind] at k and nowhere else.  h_1 and h_2 are sign-magnitude numbers below 2^31, so a row near 2^32
    climbs there over its first values with second differences of 2^29."""
    c = np.random.default_rng(seed).integers(1, 1000, n)
    if kind == "under":
        X = c.copy()
    else:
        X = TWO32 - 1 - c
        X[:4] = (2 ** 31 - 1, 2 ** 31 - 1, 2 ** 31 - 1 + 2 ** 29, 2 ** 31 - 1 + 2 ** 29 + 2 ** 30)
    X[k] = F_KINDS[kind][0]
    return X


def family_f():
    out = []
    for place, (n, k) in F_PLACES.items():
        for j, kind in enumerate(F_KINDS):
            for order in ((1, 2) if n == F_SMALL else (1 + (j + 1) % 2,)):
                X = f_values(n, k, kind, 600 + len(out))
                stream, p = xc.encode(X, order, xc.even(n, n // 40), n_oct=4)
                out.append(Seam(f"F_{place}_{kind}_order{order}", stream, p, n, X=X, want=F_KINDS[kind][1], at=k))
        for kind, pair in (("top", (TWO32 - 2, TWO32 - 1)), ("over", (TWO32 - 1, TWO32))):   # order 0: a reference plus a stored 1
            X = np.random.default_rng(650 + len(out)).integers(0, 1000, n)
            X[k - 1:k + 1] = pair
            ls = xc.even(k - 1, max(1, (k - 1) // 40)) + [2] + (xc.even(n - k - 1, max(1, (n - k - 1) // 40)) if n - k - 1 else [])
            stream, p = xc.encode(X, 0, ls)
            out.append(Seam(f"F_{place}_{kind}_order0", stream, p, n, X=X, want=F_KINDS[kind][1], at=k))
    return out


# ------------------------------------------------------------------------------------------------ G: missing values at the seams
G_SIZES = [1, 31, 32, 33, 255, 256, 257, STEP * BLOCK - 1, STEP * BLOCK, STEP * BLOCK + 1]


def g_row(name, present, m, order, seed):
    present = np.asarray(present, dtype=bool)
    n, P = present.size, int(present.sum())
    rng = np.random.default_rng(seed)
    X = rng.integers(0, 4096, P) if order == 0 or P < 8 else xc._smooth(P, seed, 0.0005, 16)
    stream, p = mv.encode(X, present, m, order, xc.even(n, max(1, n // 29)), n_oct=3)
    return Seam(name, stream, p, n, m=m, X=X, present=present)


def family_g():
    out = []

    def add(name, present, k):
        m, order = 1 + k % 2, k % 3
        if present.size <= order:
            order = 0
        out.append(g_row(f"G_{name}_order{order}_m{m}", present, m, order, 700 + k))
    for k, n in enumerate(G_SIZES):
        add(f"n{n}", np.random.default_rng(70 + k).random(n) >= 0.3, k)
    gone_block = np.ones(1024, dtype=bool)
    gone_block[256:512] = False
    add("block_missing_beside_block_present", gone_block, 10)
    for P in (256, 1024):
        present = np.zeros(2500, dtype=bool)
        present[np.random.default_rng(71 + P).permutation(2500)[:P]] = True
        add(f"P{P}", present, 11 + P // 512)
    add("P0", np.zeros(300, dtype=bool), 12)
    for first in (255, 256, 257):
        add(f"first_present_{first}", np.arange(600) >= first, 14 + first)
    for at in (31, 32, 63, 64):
        add(f"missing_at_{at}", np.arange(200) != at, 20 + at)
    add("missing_at_31_32_63_64", ~np.isin(np.arange(200), (31, 32, 63, 64)), 25)
    seams = np.random.default_rng(77).random(2048) >= 0.2                 # 2048 positions: the gather's row
    seams[256:512] = False
    seams[512:768] = True
    seams[[31, 32, 63, 64, 1023, 1024]] = False
    add("gather", seams, 28)
    return out


# ------------------------------------------------------------------------------------------------ H: malformed rows
H_GROUPS = STEP * GROUP_TILE + 300
H_PLACES = {"g0": 0, "g255": 255, "g256": 256, "tile64": STEP * GROUP_TILE + 5, "last": H_GROUPS - 1}
H_NBITS, H_WIDTH_BITS, H_LENGTH_BITS = 32, 6, 17


def _h_base():
    """Order 0, 66 tiles of groups; every table entry is wide enough to hold a fault: references of 32 bits, widths of 6,
    lengths of 17.  The groups of H_PLACES hold two values, ref and ref + 1."""
    rng = np.random.default_rng(800)
    ng = H_GROUPS
    ls = rng.integers(1, 4, ng)
    ls[list(H_PLACES.values())] = 2
    ws = 1 + (np.arange(ng) * 5) % 11
    X = rng.integers(0, np.int64(1) << np.repeat(ws, ls)) + np.repeat(rng.integers(0, 5000, ng), ls)
    starts = np.cumsum(ls) - ls
    for g in H_PLACES.values():
        X[starts[g] + 1] = X[starts[g]] + 1
    stream, p = xc.encode(X, 0, ls, widths=[int(w) for w in ws], nbits=H_NBITS, width_bits=H_WIDTH_BITS, length_bits=H_LENGTH_BITS)
    return X, ls, ws, stream, p


def _h_exact():
    """300 groups whose bits end with the stream's last byte: groups of one value are widened until they do."""
    rng = np.random.default_rng(801)
    ng = 300
    ls = rng.integers(1, 4, ng)
    ws = 1 + (np.arange(ng) * 5) % 11
    X = rng.integers(0, np.int64(1) << np.repeat(ws, ls)) + np.repeat(rng.integers(0, 5000, ng), ls)
    ones = [g for g in range(ng) if ls[g] == 1]
    for g in ones[:(-int((ws * ls).sum())) % 8]:
        ws[g] += 1
    stream, p = xc.encode(X, 0, ls, widths=[int(w) for w in ws], width_bits=H_WIDTH_BITS)
    return X, ls, ws, stream, p, ones[-1]


def family_h():
    out = []
    X, ls, ws, stream, p = _h_base()
    n, ng = int(X.size), H_GROUPS
    t = tables(stream, n, p)
    assert t["status"] == OK

    def add(name, want, s=stream, m=0, groups=None, **changes):
        out.append(Seam("H_" + name, s, dict(p, **changes), n, m=m, want=want, groups=groups))
    width_at = lambda g: t["widths_bit"] + g * H_WIDTH_BITS                   # noqa: E731
    length_at = lambda g: t["lengths_bit"] + g * H_LENGTH_BITS                # noqa: E731

    def with_length(s, g, length):
        return patched(s, length_at(g), H_LENGTH_BITS, length - p["length_ref"])
    add("intact", OK)
    for place, g in H_PLACES.items():
        add(f"width33_{place}", INVALID, patched(stream, width_at(g), H_WIDTH_BITS, 33 - p["width_ref"]))
        if g == ng - 1:
            add(f"length_over_n_{place}", INVALID, length_last=n + 1)
        else:
            add(f"length_over_n_{place}", INVALID, with_length(stream, g, n + 1))
        add(f"bits_run_out_{place}", EXHAUSTED, patched(stream, width_at(g), H_WIDTH_BITS, int(ws[g]) + 8 - p["width_ref"]))
        add(f"integer_2p32_{place}", INVALID, patched(stream, t["refs_bit"] + g * H_NBITS, H_NBITS, TWO32 - 1))
    # the sum of the lengths
    half = with_length(with_length(stream, 10, n // 2 + 1), 20, n // 2 + 1)
    add("sum_over_n_in_one_tile", INVALID, half, groups=(10, 20))
    far = with_length(with_length(stream, 10, n - 2000), 3 * GROUP_TILE + 10, n - 2000)
    add("sum_over_n_across_tiles", INVALID, far, groups=(10, 3 * GROUP_TILE + 10))
    three = next(g for g in range(300, ng) if ls[g] == 3)
    less = with_length(stream, three, 2)
    add("sum_one_less", INVALID, less)
    # two faults at once: the earlier line wins
    cut = t["data_bit"] // 8 + 100
    add("width33_and_bits_run_out", INVALID, patched(stream, width_at(H_PLACES["tile64"]), H_WIDTH_BITS, 33 - p["width_ref"])[:-10])
    add("sum_one_less_and_bits_run_out", INVALID, less[:cut])
    add("more_groups_than_values_and_no_tables", INVALID, stream[:3], n_groups=n + 1)
    add("tables_cut_by_one_byte_big", EXHAUSTED, stream[:t["data_bit"] // 8 - 1])
    # the same faults in a row with codes inside its groups: the tables' statuses come before the missing-value rule
    add("intact_m1", OK, m=1)
    add("width33_g256_m1", INVALID, patched(stream, width_at(256), H_WIDTH_BITS, 33 - p["width_ref"]), m=1)
    add("sum_one_less_m2", INVALID, less, m=2)
    add("bits_run_out_last_m1", EXHAUSTED, patched(stream, width_at(ng - 1), H_WIDTH_BITS, int(ws[ng - 1]) + 8 - p["width_ref"]), m=1)
    add("tables_cut_by_one_byte_m2", EXHAUSTED, stream[:t["data_bit"] // 8 - 1], m=2)
    # the bits' end to the bit
    X2, ls2, ws2, stream2, p2, one = _h_exact()
    t2 = tables(stream2, X2.size, p2)
    out.append(Seam("H_bits_fit_exactly", stream2, p2, X2.size, X=X2, want=OK))
    wider = patched(stream2, t2["widths_bit"] + one * H_WIDTH_BITS, H_WIDTH_BITS, int(ws2[one]) + 1 - p2["width_ref"])
    out.append(Seam("H_bits_pass_the_end_by_one_bit", wider, p2, X2.size, want=EXHAUSTED))
    out.append(Seam("H_tables_cut_by_one_byte", stream2[:t2["data_bit"] // 8 - 1], p2, X2.size, want=EXHAUSTED))
    out.append(Seam("H_bits_fit_exactly_m2", stream2, p2, X2.size, m=2, want=OK))
    # more groups than values while the tables fit
    few = dict(n_groups=5, nbits=8, width_ref=0, width_bits=4, length_ref=1, length_inc=1, length_last=0, length_bits=4, order=0, n_oct=0)
    out.append(Seam("H_more_groups_than_values", np.zeros(16, np.uint8), few, 4, want=INVALID))
    return out


# ------------------------------------------------------------------------------------------------ all of them
_BUILDERS = dict(A=family_a, B=family_b, C=family_c, D=family_d, E=family_e, F=family_f, G=family_g, H=family_h)
_FAMILIES = {}


def family(letter):
    """The cases of a family, built once."""
    if letter not in _FAMILIES:
        _FAMILIES[letter] = _BUILDERS[letter]()
    return list(_FAMILIES[letter])


def cases():
    return [c for letter in _BUILDERS for c in family(letter)]


def case(name):
    return next(c for c in family(name[0]) if c.name == name)


EMPTY = dict(n_groups=0, nbits=0, width_ref=0, width_bits=0, length_ref=0, length_inc=0, length_last=0, length_bits=0, order=0, n_oct=0)


def empty_row(m=0):
    """A row of no values."""
    return Seam("empty_row", np.zeros(0, np.uint8), EMPTY, 0, m=m)


def family_rows(letter, coded_missing):
    """The rows of a family's call on the GPU: its valid rows without (coded_missing False: grib_unpack_cpx) or with
    (True: grib_unpack_cpx_mv) missing value management, a row marked simple-packed behind the fourth of them and a row of
    no values at the end."""
    cs = [c for c in family(letter) if not c.refused and c.status == OK and bool(c.m) == coded_missing]
    return cs[:4] + [None] + cs[4:] + [empty_row(m=1 if coded_missing else 0)]


def call(order, seed=2):
    """The rows `order` -- a Seam, or None for a row marked simple-packed -- as one call: (buf, rows, recs, missing).
    Row i's stream begins at an offset that is i + 1 mod 4, behind one to four bytes of garbage."""
    from smmregrid_amd import GRIB_CPX_DTYPE
    from tests.ccsds_cases import rules
    rows = rules(len(order), seed)
    recs = np.zeros(len(order), dtype=GRIB_CPX_DTYPE)
    parts, at = [], 0
    for i, c in enumerate(order):
        pad = 1 + ((i + 1) - (at + 1)) % 4
        parts.append(np.full(pad, 0xA5, np.uint8))
        at += pad
        if c is None:
            rows["nbits"][i], rows["byte_off"][i], recs[i] = 12, 12345, xc.simple_record()
            continue
        assert at % 4 == (i + 1) % 4
        rows["nbits"][i], recs[i] = c.params["nbits"], c.record(at)
        parts.append(c.stream)
        at += c.stream.size
    missing = np.array([c.m if c is not None else 0 for c in order], dtype=np.uint8)
    return np.concatenate(parts), rows, recs, missing
