"""Inputs of the categorical (largest area fraction) tests: operators with planted rows, class fields, the independent
statement of the rule on indicator fields, and the count of what a case covers.  Plain numpy and the C oracle, no GPU.

An operator of `operator(D, ...)` has S = 300 source cells.  When D >= N_PLANTED its first rows are PLANTED on reserved
source cells (the first RESERVED of them, which no other row links to), so that a field can put chosen values there:

  row 0  a tie: four links of 0.25, values a b a b              -> a, the first link's class, share 0.5
  row 1  a missing link: (missing .5) (a .25) (a .25)           -> a, val / tot = 0.5; dst_frac 0.5: dead at area_min 0.3
  row 2  ten links of 0.09 for a around one of 0.10 for b       -> a: the winner is not the heaviest single link
  row 3  no links                                               -> dead
  row 4  two links, both missing                                -> dead
  row 5  weights 0.0 and -0.5                                   -> dead: no share > 0
  row 6  dst_imask 0                                            -> dead when masked
  row 7  dst_frac 0.1, nothing missing                          -> dead at area_min 0.3 and 0.9
  row 8  b through two zero-weight links first, then a 0.3      -> a: a class of zero-weight links cannot win

The other rows cycle through LENGTHS (slice by slice: those up to 17, those up to 64, all of them; and `long_rows`)
with columns drawn from the unreserved cells; half of them have
dyadic weights k / 16 (k = 0 .. 4: exact sums, so ties and zero weights arise by themselves), half random ones.

`coverage` counts, over the (batch row, destination row) pairs of a case, what the issue wants every GPU case to hold.
A case cannot hold what its shape rules out, and `required` says so: a tie and a winner that is not the heaviest link
need two classes, a missing link needs a float field or a fill value, and the planted rows need D >= N_PLANTED (the D = 1
case is one ordinary row)."""
from collections import namedtuple

import numpy as np

from oracle import oracle
from smmregrid_amd.categorical import ModeRule

S = 300
RESERVED = 40
N_PLANTED = 9
LENGTHS = (0, 1, 2, 3, 16, 17, 33, 64, 65)
AREA_MINS = (0.0, 0.3, 0.9)
DTYPES = {"f32": np.dtype(np.float32), "f64": np.dtype(np.float64), "i16": np.dtype(np.int16), "u16": np.dtype(np.uint16)}
FILLS = {"i16": (-32768, -1), "u16": (65535, 0)}
CLASSES = {"f32": (1.0, 2.5, -3.0, 0.0, 1e30), "f64": (1.0, 2.5, -3.0, 0.0, 1e300), "i16": (1, 2, 7, -5, 30000),
           "u16": (1, 2, 7, 40000, 65534)}

Operator = namedtuple("Operator", "n_src n_dst src dst w csr imask frac planted")
# planted row -> (weights, value codes): "a" / "b" the two classes of the batch row, "m" a missing value
PLANTED = (((0.25, 0.25, 0.25, 0.25), "abab"),
           ((0.5, 0.25, 0.25), "maa"),
           ((0.09,) * 5 + (0.10,) + (0.09,) * 5, "aaaaabaaaaa"),
           ((), ""),
           ((0.5, 0.5), "mm"),
           ((0.0, -0.5), "ab"),
           ((0.5, 0.5), "aa"),
           ((0.5, 0.5), "ab"),
           ((0.0, 0.0, 0.3), "bba"))


def operator(D, seed=0, lengths=LENGTHS, long_rows=None):
    """long_rows: {destination row: length} for rows longer than the cycle gives them."""
    rng = np.random.default_rng([20261021, seed, D])
    planted = D >= N_PLANTED
    rows, at = [], 0
    for d in range(D):
        if planted and d < N_PLANTED:
            w = np.array(PLANTED[d][0], dtype=np.float64)
            cols = np.arange(at, at + w.size)
            at += w.size
        else:
            # slices take turns: lengths up to 17, up to 64, and the whole cycle -- a slice with a row of 65 links is past
            # the capacity of the kernel's LDS form for every type, one of up to 64 for float64 alone, one of up to 17 never
            cycle = [n for n in lengths if n <= (17, 64, 1 << 30)[(d // 64) % 3]]
            n = (long_rows or {}).get(d, cycle[(d + seed) % len(cycle)])
            lo = RESERVED if planted else 0
            cols = np.sort(rng.choice(np.arange(lo, S), size=n, replace=False))
            w = rng.integers(0, 5, size=n) / 16.0 if (d % 2) else rng.uniform(0.01, 1.0, size=n)
        rows.append((cols, w))
    assert at <= RESERVED
    rowptr = np.zeros(D + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum([c.size for c, _ in rows])
    col = np.concatenate([c for c, _ in rows]).astype(np.int32) if D else np.zeros(0, np.int32)
    val = np.concatenate([w for _, w in rows]).astype(np.float64) if D else np.zeros(0)
    dst = np.repeat(np.arange(1, D + 1), np.diff(rowptr)).astype(np.int32)
    # the links in a shuffled order: the operator sorts them back into the canonical CSR
    order = rng.permutation(col.size)
    imask = (rng.random(D) > 0.1).astype(np.int32)
    frac = rng.uniform(0.35, 1.0, size=D)
    if planted:
        imask[:N_PLANTED] = 1
        imask[6] = 0
        frac[:N_PLANTED] = 1.0
        frac[1], frac[7] = 0.5, 0.1
    return Operator(S, D, (col + 1)[order], dst[order], val[order], (rowptr, col, val), imask, frac, planted)


def rule_of(kind, n_fill):
    if kind in ("f32", "f64"):
        return ModeRule()
    fills = FILLS[kind][:n_fill]
    return ModeRule(fills, FILLS[kind][0])


def field(op, B, kind, n_classes=5, n_fill=1, seed=0, pitch=0):
    """(x, rule): a (B, S + pitch) field of class codes.  n_classes 1 .. 5, or "own": every cell a class of its own.
    About a tenth of the cells is missing where the type can say so; the pad holds a value no class has."""
    dtype = DTYPES[kind]
    rng = np.random.default_rng([20261021, seed, B, op.n_dst])
    rule = rule_of(kind, n_fill)
    if kind in ("f32", "f64"):
        missing = np.array([np.nan, np.inf, -np.inf], dtype=dtype)
    else:
        missing = np.array(rule.fill, dtype=dtype)
    if n_classes == "own":
        x = (np.arange(1, S + 1)[None, :] + np.arange(B)[:, None]).astype(dtype)
        classes = None
    else:
        classes = np.array(CLASSES[kind][:n_classes], dtype=dtype)
        x = classes[rng.integers(0, classes.size, size=(B, S))]
    if missing.size:
        hole = rng.random((B, S)) < 0.1
        x[hole] = missing[rng.integers(0, missing.size, size=int(hole.sum()))]
    if op.planted:
        at = 0
        for weights, codes in PLANTED:
            for b in range(B):
                if classes is None:
                    a, c = dtype.type(1000 + b), dtype.type(2000 + b)
                else:
                    a, c = classes[b % classes.size], classes[(b + 1) % classes.size]
                m = missing[b % missing.size] if missing.size else a
                x[b, at:at + len(codes)] = [{"a": a, "b": c, "m": m}[ch] for ch in codes]
            at += len(codes)
    if pitch:
        pad = np.full((B, pitch), 77 if dtype.kind != "f" else 777.0, dtype=dtype)
        x = np.concatenate([x, pad], axis=1)
    return np.ascontiguousarray(x), rule


def indicator_statement(op, x, rule, masked=False, area_min=0.0):
    """(y, share) by the independent statement: one plain apply of the C oracle per distinct value, on the float64
    indicator field x == c -- the shares bit for bit -- then the argmax, bit-equal shares going to the class whose first
    link comes first in the CSR; tot and val the same applies on ones and on the field of what is not missing."""
    rowptr, col, _ = op.csr
    x = np.asarray(x)[:, :op.n_src]
    B, D = x.shape[0], op.n_dst
    miss = rule.missing(x)
    values = np.unique(x[~miss])
    best = np.zeros((B, D))
    best_first = np.full((B, D), np.iinfo(np.int64).max)
    best_val = np.zeros((B, D), dtype=x.dtype)
    big = np.iinfo(np.int64).max
    for c in values:
        ind = (x == c) & ~miss
        share = oracle.apply_c(op.csr, ind.astype(np.float64), fill=False)
        first = np.full((B, D), big)
        rep = np.zeros((B, D), dtype=x.dtype)
        for d in range(D):
            hit = ind[:, col[rowptr[d]:rowptr[d + 1]]]
            if hit.shape[1] and hit.any():
                k = np.where(hit.any(axis=1), hit.argmax(axis=1), big)
                first[:, d] = k
                rows = np.flatnonzero(k != big)
                rep[rows, d] = x[rows, col[rowptr[d] + k[rows]]]      # the first link's own bits (-0.0 stays -0.0)
        better = (share > best) | ((share == best) & (share > 0) & (first < best_first))
        best = np.where(better, share, best)
        best_first = np.where(better, first, best_first)
        best_val = np.where(better, rep, best_val)
    alive = best > 0
    if masked:
        alive &= op.imask[None, :] != 0
    if area_min > 0.0:
        tot = oracle.apply_c(op.csr, np.ones((1, x.shape[1])), fill=False)
        val = oracle.apply_c(op.csr, (~miss).astype(np.float64), fill=False)
        with np.errstate(invalid="ignore", divide="ignore"):
            alive &= ~(op.frac[None, :] * (val / tot) < area_min)
    dead = np.nan if x.dtype.kind == "f" else rule.checked(x.dtype)[1]
    y = np.where(alive, best_val, np.asarray(dead, dtype=x.dtype)).astype(x.dtype)
    return y, np.where(alive, best, 0.0)


def coverage(op, x, rule):
    """Counts over the (batch row, destination row) pairs of what the issue wants a case to hold."""
    rowptr, col, val = op.csr
    x = np.asarray(x)[:, :op.n_src]
    n = dict(tied=0, missing_link=0, dead_no_links=0, dead_all_missing=0, dead_no_positive=0, dead_masked=0, dead_area=0,
             not_heaviest=0)
    miss = rule.missing(x)
    for d in range(op.n_dst):
        c, w = col[rowptr[d]:rowptr[d + 1]], val[rowptr[d]:rowptr[d + 1]]
        for b in range(x.shape[0]):
            v, m = x[b, c], miss[b, c]
            shares = {}
            for k in range(c.size):
                if not m[k]:
                    key = float(v[k]) + 0.0      # -0.0 and +0.0 are one class
                    shares[key] = shares.get(key, 0.0) + w[k]
            top = max(shares.values(), default=0.0)
            n["missing_link"] += bool(m.any() and not m.all())
            if c.size == 0:
                n["dead_no_links"] += 1
            elif m.all():
                n["dead_all_missing"] += 1
            elif not top > 0.0:
                n["dead_no_positive"] += 1
            else:
                n["tied"] += sum(s == top for s in shares.values()) > 1
                heaviest = int(np.argmax(np.where(m, -np.inf, w)))
                winner = [k for k in shares if shares[k] == top]
                n["not_heaviest"] += (float(v[heaviest]) + 0.0) not in winner
                n["dead_masked"] += op.imask[d] == 0
                vsum, tot = sum(w[~m]), sum(w)
                n["dead_area"] += bool(op.frac[d] * (vsum / tot) < 0.3) if tot != 0 else 0
    return {k: int(v) for k, v in n.items()}


def required(op, x, rule):
    """The counts of `coverage` that must be positive for this case (see the module text)."""
    need = []
    two = np.unique(x[:, :op.n_src][~rule.missing(x[:, :op.n_src])]).size >= 2
    can_miss = x.dtype.kind == "f" or bool(rule.fill)
    if op.planted:
        need += ["dead_no_links", "dead_no_positive", "dead_masked", "dead_area"]
        if two:
            need += ["tied", "not_heaviest"]
        if can_miss:
            need += ["missing_link", "dead_all_missing"]
    return need


def checked_field(op, B, kind, **kw):
    """`field`, with its coverage asserted."""
    x, rule = field(op, B, kind, **kw)
    got = coverage(op, x, rule)
    lacking = [k for k in required(op, x, rule) if got[k] < 1]
    assert not lacking, (lacking, got)
    return x, rule


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(f"u{a.dtype.itemsize}")


def assert_bits(got, want, what=""):
    """Bit equality; in float arrays a NaN equals a NaN (dead rows)."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    diff = bits(got) != bits(want)
    if got.dtype.kind == "f":
        diff &= ~(np.isnan(got) & np.isnan(want))
    assert not diff.any(), f"{what}: {int(diff.sum())} cells differ, first at {np.argwhere(diff)[:4].tolist()}"
