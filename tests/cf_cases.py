"""Adversarial float64 inputs for the CF encode rule (`CFEncode.encode`, `YTraits<PackedY<Q>>::encode`), built on the
CPU, and numpy models of the kernels one could write by mistake.

For a rule (scale, offset, raw dtype) the pool is y0 = offset + (n + h) * scale for every n from iinfo.min - 2 to
iinfo.max + 2 and h in {0, 0.5}, each with its neighbours up to +-3 ulp: the values next to every raw count and every
rounding boundary.  `cases()` keeps from it what can tell a right encode from a wrong one -- exact ties, values on
which a wrong-kernel model disagrees with the reference, the edges of the raw range, values that round onto the fill
value -- adds fixed specials, and truncates to at most `MAX_CASES` values in a seeded order.

With a power-of-two scale the subtraction and the division are exact: models (a) and (b) cannot be told from the
reference, nor can (c) on values float32 holds exactly.  `CONTROL` is such a rule, kept to record that.  The other
rules are of the kind real files carry.

Ties: for several rules the pool holds more exact ties than `MAX_CASES` (a tie's ulp neighbours often divide to the
same t).  All ties are kept where they fit; otherwise a seeded sample of them fills the room left by the edges, the
specials, the fill values and `PER_MODEL` separating values per model."""
import functools

import numpy as np

from smmregrid_amd import CFEncode

CONTROL = (0.25, -1024.125)
RULES = [(1.9e-3, 2.7e2), (1.0e-3, 20.0), (0.01, 273.15), (1.0 / 3.0, 0.1), (-0.0037, 101325.0), CONTROL]
NON_DYADIC = [r for r in RULES if r != CONTROL]
FILLS = {np.dtype(np.int16): -32768, np.dtype(np.uint16): 65535}
RAWS = [np.dtype(np.int16), np.dtype(np.uint16)]
# (scale, offset) whose float32 decode does not read back through the encode: at 101325 one float32 ulp (2**-7) is twice
# the scale, so neighbouring raw counts decode to the same float32 (tests/test_cf_encode_reference.py)
NO_F32_ROUND_TRIP = {(-0.0037, 101325.0)}
MAX_CASES = 60000
PER_MODEL = 500
SEED = 20261017

_NAN = np.array([0x7FF8000000000000, 0xFFF4000000ABCDEF], dtype=np.uint64).view(np.float64)   # two payloads
SPECIALS = np.concatenate([np.array([0.0, -0.0, 5e-324, 2.2250738585072014e-308, -2.2250738585072014e-308, 1e19, -1e19,
                                     np.nextafter(1e19, np.inf), -1e300, 1e300, np.inf, -np.inf]), _NAN])
SPECIALS.setflags(write=False)


def rule_id(scale, offset, raw):
    return f"{scale!r},{offset!r}->{np.dtype(raw).name}"


def encoder(scale, offset, raw):
    return CFEncode(scale, offset, FILLS[np.dtype(raw)], raw)


def reference(y, scale, offset, raw):
    """The contract: `CFEncode.encode`."""
    return encoder(scale, offset, raw).encode(y)


# ---------------------------------------------------------------- wrong-kernel models, y -> raw

def _store(y, r, raw, bad_range=None):
    """The reference's tail: fill where y is not finite or r is out of range (or where `bad_range` says so)."""
    info = np.iinfo(raw)
    if bad_range is None:
        bad_range = (r < info.min) | (r > info.max)
    bad = ~np.isfinite(y) | bad_range
    return np.where(bad, FILLS[np.dtype(raw)], r).astype(raw)


def _t(y, s, o):
    return (y - np.float64(o)) / np.float64(s)


def m_reciprocal(y, s, o, raw):
    """(a) (y - o) * (1 / s) instead of the division."""
    return _store(y, np.rint((y - np.float64(o)) * (np.float64(1.0) / np.float64(s))), raw)


def m_reassociated(y, s, o, raw):
    """(b) y * (1 / s) - o / s."""
    return _store(y, np.rint(y * (np.float64(1.0) / np.float64(s)) - np.float64(o) / np.float64(s)), raw)


def m_float32(y, s, o, raw):
    """(c) the subtraction and the division in float32."""
    t = ((y.astype(np.float32) - np.float32(o)) / np.float32(s)).astype(np.float64)
    return _store(y, np.rint(t), raw)


def m_half_away(y, s, o, raw):
    """(d) round half away from zero (C's round())."""
    t = _t(y, s, o)
    w = np.trunc(t)
    return _store(y, w + np.where(np.abs(t - w) >= 0.5, np.sign(t), 0.0), raw)


def m_truncate(y, s, o, raw):
    """(e) truncation toward zero."""
    return _store(y, np.trunc(_t(y, s, o)), raw)


def m_saturate(y, s, o, raw):
    """(f) saturation at the ends of the raw range instead of the fill value."""
    info = np.iinfo(raw)
    r = np.clip(np.rint(_t(y, s, o)), info.min, info.max)
    return _store(y, r, raw, bad_range=np.zeros(y.shape, bool))


def m_wrap(y, s, o, raw):
    """(g) wrap-around: astype(raw) of the int64."""
    r = np.rint(_t(y, s, o))
    fin = np.isfinite(y) & np.isfinite(r)
    wrapped = np.where(fin, r, 0.0).astype(np.int64).astype(raw)
    return np.where(np.isfinite(y), wrapped, np.dtype(raw).type(FILLS[np.dtype(raw)])).astype(raw)


def m_range_on_t(y, s, o, raw):
    """(h) the range tested on t instead of on r."""
    info = np.iinfo(raw)
    t = _t(y, s, o)
    return _store(y, np.rint(t), raw, bad_range=~((t >= info.min) & (t <= info.max)))


def m_finite_on_t(y, s, o, raw):
    """(i) the finiteness tested on t instead of on y.  (The same function as the reference for every finite rule:
    t is finite only if y is, and a non-finite t of a finite y rounds out of range.  Kept for the record.)"""
    info = np.iinfo(raw)
    t = _t(y, s, o)
    r = np.rint(t)
    bad = ~np.isfinite(t) | (r < info.min) | (r > info.max)
    return np.where(bad, FILLS[np.dtype(raw)], r).astype(raw)


MODELS = {"a_reciprocal": m_reciprocal, "b_reassociated": m_reassociated, "c_float32": m_float32,
          "d_half_away": m_half_away, "e_truncate": m_truncate, "f_saturate": m_saturate, "g_wrap": m_wrap,
          "h_range_on_t": m_range_on_t, "i_finite_on_t": m_finite_on_t}
EXACT_ON_DYADIC = ("a_reciprocal", "b_reassociated", "c_float32")


def run_model(name, y, scale, offset, raw):
    with np.errstate(all="ignore"):
        return MODELS[name](np.asarray(y, np.float64), scale, offset, np.dtype(raw))


def disagreements(name, y, scale, offset, raw):
    """Mask of the values of y on which model `name` and the reference give different raw counts."""
    return run_model(name, y, scale, offset, raw) != reference(y, scale, offset, raw)


# ---------------------------------------------------------------- the pool and the selection

def _bits(y):
    return np.ascontiguousarray(y, dtype=np.float64).view(np.uint64)


def _unique(y):
    """Deduplicated by bit pattern: -0.0 and +0.0, and the NaN payloads, stay apart."""
    return np.unique(_bits(y)).view(np.float64)


def pool(scale, offset, raw):
    info = np.iinfo(raw)
    n = np.arange(info.min - 2, info.max + 3, dtype=np.float64)
    parts = []
    for h in (0.0, 0.5):
        y0 = np.float64(offset) + (n + h) * np.float64(scale)
        parts.append(y0)
        for direction in (-np.inf, np.inf):
            y = y0
            for _ in range(3):
                y = np.nextafter(y, direction)
                parts.append(y)
    return _unique(np.concatenate(parts))


def _rounded(y, scale, offset):
    return np.rint(_t(np.asarray(y, np.float64), scale, offset))


def _ordered(y):
    """float64 -> int64 that sorts like the value (finite y)."""
    b = int(np.float64(y).view(np.int64))
    return b if b >= 0 else -(1 << 63) - b


def _unordered(k):
    return np.int64(k if k >= 0 else -(1 << 63) - k).view(np.float64)


def _step_at(scale, offset, k):
    """(largest y that still rounds below k, smallest y that rounds to k or above) along increasing r; found by
    bisection over the doubles: r(y) = rint((y - offset) / scale) is monotone in y."""
    centre = offset + k * scale
    a, b = centre - 2.0 * abs(scale), centre + 2.0 * abs(scale)
    below, above = (a, b) if scale > 0 else (b, a)        # r(below) < k <= r(above)
    assert _rounded(below, scale, offset) < k <= _rounded(above, scale, offset)
    lo, hi = _ordered(below), _ordered(above)
    while abs(hi - lo) > 1:
        mid = (lo + hi) // 2
        if _rounded(_unordered(mid), scale, offset) >= k:
            hi = mid
        else:
            lo = mid
    return float(_unordered(lo)), float(_unordered(hi))


def edges(scale, offset, raw):
    """[largest y that rounds to max, smallest that rounds to max + 1, the value that last rounds to min - 1, the
    first that rounds to min] ("largest" / "smallest" along increasing raw count: mirrored for a negative scale)."""
    info = np.iinfo(raw)
    out = []
    for k in (info.max + 1, info.min):
        below, at = _step_at(scale, offset, k)
        assert _rounded(below, scale, offset) == k - 1 and _rounded(at, scale, offset) == k
        out += [below, at]
    return np.array(out)


@functools.lru_cache(maxsize=None)
def _analyse(scale, offset, raw_name):
    raw = np.dtype(raw_name)
    fill = FILLS[raw]
    rng = np.random.default_rng(SEED)
    p = pool(scale, offset, raw)
    with np.errstate(all="ignore"):
        t = _t(p, scale, offset)
    ties = p[np.abs(t - np.floor(t)) == 0.5]
    sep = {name: p[disagreements(name, p, scale, offset, raw)] for name in MODELS}
    counts = {name: int(v.size) for name, v in sep.items()}
    onto_fill = p[np.rint(t) == fill]
    onto_fill = np.concatenate([onto_fill, np.nextafter(onto_fill, -np.inf), np.nextafter(onto_fill, np.inf)])
    fixed = _unique(np.concatenate([SPECIALS, edges(scale, offset, raw), onto_fill]))
    some = [v if v.size <= PER_MODEL else rng.choice(v, PER_MODEL, replace=False) for v in sep.values()]
    fixed = _unique(np.concatenate([fixed] + some))
    # every tie is kept where that fits; where the pool holds more of them than the room left (the dyadic control, and
    # four of the non-dyadic rule / raw type pairs), a seeded sample of them fills that room
    room = n_fixed_room = MAX_CASES - fixed.size
    ties = ties[~np.isin(_bits(ties), _bits(fixed))]
    all_ties = ties.size <= room
    if not all_ties:
        ties = rng.choice(ties, room, replace=False)
    kept = _unique(np.concatenate([fixed, ties]))
    room = MAX_CASES - kept.size
    rest = _unique(np.concatenate(list(sep.values())))
    rest = rest[~np.isin(_bits(rest), _bits(kept))]
    if rest.size > room:
        rest = rng.choice(rest, room, replace=False)
    out = np.concatenate([kept, rest])
    out = out[rng.permutation(out.size)]
    assert out.size <= MAX_CASES and np.unique(_bits(out)).size == out.size
    out.setflags(write=False)
    return out, counts, {"pool": int(p.size), "ties": int((np.abs(t - np.floor(t)) == 0.5).sum()), "all_ties": all_ties,
                         "tie_room": int(n_fixed_room)}


def cases(scale, offset, raw):
    """The 1-D float64 case array of a rule (read-only, the same array on every call)."""
    return _analyse(float(scale), float(offset), np.dtype(raw).name)[0]


def pool_counts(scale, offset, raw):
    """model name -> number of values of the WHOLE pool on which it disagrees with the reference."""
    return dict(_analyse(float(scale), float(offset), np.dtype(raw).name)[1])


def pool_info(scale, offset, raw):
    return dict(_analyse(float(scale), float(offset), np.dtype(raw).name)[2])
