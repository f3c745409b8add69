"""Shared pieces of the half-precision tests (float16 / bfloat16 fields and results): an independent float64 -> half
rounding in integer arithmetic on the float64 bits, its exact check in `fractions.Fraction` arithmetic, the adversarial
float64 values, and the small operators and fields of tests/test_gpu_half.py.

The rounding here is written independently of `smmregrid_amd.to_bfloat16` and of the kernels' encode: the normal range
adds the rounding bias to the re-biased float64 bits and shifts once, the subnormal range shifts the significand by its
distance to the smallest subnormal.  `exact_bits` restates the rule with rational numbers."""
import functools
from fractions import Fraction

import numpy as np

F16 = (5, 10, np.uint16(0x7E00))     # exponent bits, stored significand bits, canonical quiet NaN
BF16 = (8, 7, np.uint16(0x7FC0))
KINDS = {"f16": F16, "bf16": BF16}


def round_bits(v, kind):
    """Bits of float64 `v` rounded to nearest even into the half type `kind` ("f16" / "bf16"); NaN -> canonical."""
    eb, mb, qnan = KINDS[kind]
    v = np.ascontiguousarray(v, dtype=np.float64)
    u = v.view(np.uint64)
    sign = ((u >> np.uint64(48)) & np.uint64(0x8000))
    a = u & np.uint64(0x7FFFFFFFFFFFFFFF)
    e = (a >> np.uint64(52)).astype(np.int64)
    bias = (1 << (eb - 1)) - 1
    e_first = 1023 - bias + 1                       # float64 exponent field of the half type's smallest normal
    drop = 52 - mb
    inf = np.uint64(((1 << eb) - 1) << mb)
    # normal results: re-bias, add half an ulp minus one plus the kept bit's parity, shift -- the carry walks into the exponent
    norm = a - (np.uint64(e_first - 1) << np.uint64(52))
    rn = (norm + np.uint64((1 << (drop - 1)) - 1) + ((norm >> np.uint64(drop)) & np.uint64(1))) >> np.uint64(drop)
    rn = np.minimum(rn, inf)
    # subnormal results: the significand counted in units of the smallest subnormal, 2 ** (1 - bias - mb)
    m = (a & np.uint64(0x000FFFFFFFFFFFFF)) | np.uint64(1 << 52)
    sh = np.minimum((1075 + 1 - bias - mb) - e, 63).astype(np.uint64)     # value = m * 2 ** (e - 1075)
    sh = np.maximum(sh, np.uint64(1))
    sub = (m + ((np.uint64(1) << (sh - np.uint64(1))) - np.uint64(1)) + ((m >> sh) & np.uint64(1))) >> sh
    bits = np.where(e >= e_first, rn, sub)
    bits = np.where(a > np.uint64(0x7FF0000000000000), np.uint64(qnan), bits | sign)
    return bits.astype(np.uint16).reshape(v.shape)


@functools.lru_cache(maxsize=None)
def _table(kind):
    """exact value -> bits of every non-negative finite element of the half type"""
    eb, mb, _ = KINDS[kind]
    bias = (1 << (eb - 1)) - 1
    out = {}
    for b in range(((1 << eb) - 1) << mb):
        ex, fr = b >> mb, b & ((1 << mb) - 1)
        val = Fraction(fr, 1 << mb) * Fraction(2) ** (1 - bias) if ex == 0 else \
            (1 + Fraction(fr, 1 << mb)) * Fraction(2) ** (ex - bias)
        out[val] = b
    return out


def exact_bits(x, kind):
    """The same for one Python float, in exact rational arithmetic: the nearest element, ties to the even significand,
    +-inf from the midpoint between the largest finite element and the next power of two on."""
    eb, mb, qnan = KINDS[kind]
    if x != x:
        return int(qnan)
    bias = (1 << (eb - 1)) - 1
    inf = ((1 << eb) - 1) << mb
    sign = 0x8000 if np.signbit(x) else 0
    if x in (float("inf"), float("-inf")):
        return sign | inf
    f = abs(Fraction(x))
    k = 1 - bias
    if f > 0:
        while Fraction(2) ** (k + 1) <= f:
            k += 1
    ulp = Fraction(2) ** (k - mb)
    n = f / ulp
    r = n.numerator // n.denominator
    rest = n - r
    if rest > Fraction(1, 2) or (rest == Fraction(1, 2) and r % 2 == 1):
        r += 1
    val = r * ulp
    if val >= Fraction(2) ** (bias + 1):
        return sign | inf
    return sign | _table(kind)[val]


def widen(bits, kind):
    """float32 value of every element (exact)."""
    bits = np.asarray(bits, dtype=np.uint16)
    if kind == "f16":
        return bits.view(np.float16).astype(np.float32)
    return (bits.astype(np.uint32) << np.uint32(16)).view(np.float32)


def adversarial(kind):
    """float64 values that tell a correctly rounded conversion from a float32 detour, a truncation or a flush."""
    eb, mb, _ = KINDS[kind]
    bias = (1 << (eb - 1)) - 1
    u = 2.0 ** -mb                                    # ulp of 1.0
    top = (2.0 - u) * 2.0 ** bias                     # largest finite
    over = (2.0 - u / 2) * 2.0 ** bias                # first value that rounds to inf (a tie, even = inf)
    tiny = 2.0 ** (1 - bias - mb)                     # smallest subnormal
    vals = [1 + u / 2 + 2.0 ** -40,                   # a float32 detour lands on the tie and rounds down to 1.0
            1 + u / 2 - 2.0 ** -40, 1 + u / 2, 1 + 3 * u / 2, 1 + 5 * u / 2,      # ties to even and to odd
            1 + 3 * u / 2 + 2.0 ** -40, 1 + 3 * u / 2 - 2.0 ** -40,
            top, np.nextafter(over, 0.0), over, np.nextafter(over, np.inf), -over, -np.nextafter(over, 0.0),
            tiny / 2, tiny / 2 * (1 + 2.0 ** -30), tiny, tiny * 1.5, tiny * 2.5, tiny * (1.5 - 2.0 ** -30),
            2.0 ** (1 - bias) - tiny / 2, 2.0 ** (1 - bias) * (1 - 2.0 ** -30),     # subnormal -> first normal
            0.0, -0.0, -tiny / 2, -tiny / 2 * (1 + 2.0 ** -30), 5e-324, 2.2250738585072014e-308,
            65519.99, 65520.0, 2.0 ** -25, 2.0 ** -25 * (1 + 2.0 ** -30),
            1 + 2.0 ** -11 + 2.0 ** -40, 1 + 2.0 ** -8 + 2.0 ** -40,
            np.nextafter(1e19, 0.0), 1e19, np.nextafter(1e19, np.inf), 1.0000001e19, -1e19, -1e30, 1e30,
            np.inf, -np.inf, np.nan]
    rng = np.random.default_rng(20261018)
    # random significands at random binades: the exact tie above each and its two neighbours 2 ** -40 away
    sig = 1 + rng.integers(0, 1 << mb, size=64) * u
    ex = rng.integers(3 - bias - mb, min(bias, 62), size=64)
    for s, e in zip(sig, ex):
        for d in (0.0, -2.0 ** -40, 2.0 ** -40):
            vals.append(float(np.ldexp(s + u / 2 + d, int(e))))
            vals.append(-float(np.ldexp(s + u / 2 + d, int(e))))
    return np.array(vals, dtype=np.float64)


# ---------------------------------------------------------------- operators and fields of the GPU tests

N_SRC = 201          # odd: 2-byte rows start off 4-byte boundaries
ROW_LENGTHS = (0, 1, 4, 17, 23)


def small_links(n_dst, seed, n_src=N_SRC, used=None):
    """Rows of 0, 1, 4, 17 and 23 links with positive weights summing to one; `used`: draw from the first `used` cells."""
    rng = np.random.default_rng(seed)
    src, dst, w = [], [], []
    for d in range(n_dst):
        ln = ROW_LENGTHS[d % len(ROW_LENGTHS)] if d < 2 * len(ROW_LENGTHS) else int(rng.choice(ROW_LENGTHS))
        if ln == 0:
            continue
        cols = rng.choice(used or n_src, size=ln, replace=False)
        ww = rng.random(ln) + 0.05
        src.append(cols + 1)
        dst.append(np.full(ln, d + 1))
        w.append(ww / ww.sum() if ln > 1 else np.ones(1))
    src, dst, w = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32), np.concatenate(w)
    perm = rng.permutation(src.size)
    return src[perm], dst[perm], w[perm]


def epilogue_vectors(n_dst, seed):
    rng = np.random.default_rng(seed + 1)
    return (rng.random(n_dst) > 0.15).astype(np.int32), np.round(rng.random(n_dst), 3)


def half_field(kind, shape, seed):
    """uint16 bits of a half field: ordinary values plus NaN, +-inf, +-0, subnormals and the largest finite element."""
    eb, mb, _ = KINDS[kind]
    rng = np.random.default_rng(seed)
    bits = round_bits(3.0 * rng.standard_normal(shape), kind)
    top = (((1 << eb) - 1) << mb) - 1
    special = np.array([0x7E00 if kind == "f16" else 0x7FC0, ((1 << eb) - 1) << mb, 0x8000 | (((1 << eb) - 1) << mb),
                        0x0000, 0x8000, 0x0001, 0x8003, (1 << mb) - 1, top, 0x8000 | top], dtype=np.uint16)
    pick = rng.random(shape) < 0.08
    bits[pick] = rng.choice(special, size=int(pick.sum()))
    return bits


def float_field(dtype, shape, seed):
    """float32 / float64 field whose results exercise the narrowing: magnitudes from subnormal-half to beyond the
    largest half, NaN and +-inf."""
    rng = np.random.default_rng(seed)
    x = rng.standard_normal(shape) * 10.0 ** rng.integers(-9, 6, size=shape)
    pick = rng.random(shape) < 0.05
    x[pick] = rng.choice(np.array([np.nan, np.inf, -np.inf, 0.0, -0.0, 65504.0, 3.3e38, -3.3e38]), size=int(pick.sum()))
    with np.errstate(over="ignore"):
        return x.astype(dtype)
