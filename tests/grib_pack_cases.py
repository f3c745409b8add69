"""The rows that pin the GRIB encode rule (smm_grib_codec.hpp / GribEncode.encode), shared by the CPU harness test and
the GPU tests of smm_grib_pack.  Plain numpy, no GPU.

`batch(n_dst, seed)` gives one call's worth: float64 values (rows, n_dst), the widths and the decimal scale factors,
every row kind below once per pass, the widths cycling through WIDTHS and D through DECIMALS with coprime periods so
that two passes give every kind two different widths."""
import numpy as np

WIDTHS = (1, 7, 12, 16, 17, 24, 25, 31, 32)
DECIMALS = (-2, 0, 3)
FLT_MAX = float(np.finfo(np.float32).max)


def _holes(rng, v, density):
    v = v.copy()
    v[rng.random(v.size) < density] = np.nan
    return v


def row(kind, n, width, rng):
    """One row of n values of the named kind; `width` is the width the row will be packed with."""
    base = rng.normal(280.0, 15.0, n)
    if kind == "full":
        return base
    if kind.startswith("missing"):
        return _holes(rng, base, int(kind[7:]) / 100.0)
    if kind == "all_missing":
        return np.full(n, np.nan)
    if kind in ("one_first", "one_last"):
        v = np.full(n, np.nan)
        v[0 if kind == "one_first" else -1] = base[0]
        return v
    if kind == "constant":
        return np.full(n, 273.15)
    if kind == "constant_holes":
        return _holes(rng, np.full(n, -41.5), 0.4)
    if kind == "ties":           # min 0, max 2^width - 1: E = 0 when D = 0, and every k + 0.5 is an exact half step
        top = float(2 ** width - 1)
        v = np.minimum(rng.integers(0, 1000, n).astype(np.float64) + 0.5, top)
        v[rng.integers(0, n)] = top
        v[rng.integers(0, n)] = 0.0
        if n == 1:
            v[0] = 0.5
        return v
    if kind == "adjacent":       # a range of a few ulps of float64
        return 1.0 + rng.integers(0, 4, n) * 2.0 ** -52
    if kind == "huge":
        return rng.normal(0.0, 1.0, n) * 1e30
    if kind == "over_fltmax":    # beyond float32 as they are, or once multiplied by 10^D
        v = base.copy()
        v[rng.random(n) < 0.3] = 1e39
        v[rng.random(n) < 0.2] = -3e38
        v[rng.random(n) < 0.2] = 2e36
        return v
    if kind == "inf":
        v = base.copy()
        v[rng.random(n) < 0.2] = np.inf
        v[rng.random(n) < 0.2] = -np.inf
        return v
    if kind == "subnormal":      # a subnormal range: E is raised to -1022
        return rng.integers(0, 6, n) * 1e-310
    if kind == "zeros":          # -0.0 and +0.0 among small values of both signs
        v = rng.choice(np.array([-0.0, 0.0, 0.0, -0.0, 1e-3, -2e-3]), n)
        return v
    if kind == "signed_zero_only":
        return rng.choice(np.array([-0.0, 0.0]), n)
    raise KeyError(kind)


KINDS = ("full", "missing5", "missing50", "missing95", "all_missing", "one_first", "one_last", "constant",
         "constant_holes", "ties", "adjacent", "huge", "over_fltmax", "inf", "subnormal", "zeros", "signed_zero_only")


def batch(n_dst, seed, passes=2):
    rng = np.random.default_rng(seed)
    kinds = list(KINDS) * passes
    nbits = np.array([WIDTHS[i % len(WIDTHS)] for i in range(len(kinds))], dtype=np.int32)
    dec = np.array([0 if k == "ties" else DECIMALS[(i // 2) % len(DECIMALS)] for i, k in enumerate(kinds)], dtype=np.int64)
    values = np.stack([row(k, n_dst, int(w), rng) for k, w in zip(kinds, nbits)])
    return values, nbits, dec, kinds
