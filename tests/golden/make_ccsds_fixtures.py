"""Writes tests/golden/ccsds/*.npz: CCSDS streams from libaec's own encoder (through ctypes), their parameters and the
integers they code.  Run from the repository root where libaec is installed:

    python tests/golden/make_ccsds_fixtures.py

Every fixture is decoded back with libaec (the arbiter) and with the project's host decoder, and the set must take
every coding option of the histogram at least once.  ccsdsFlags as ecCodes writes them carry AEC_DATA_MSB and
AEC_DATA_3BYTE, which say nothing about the stream: some fixtures record them to show that they are ignored."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from smmregrid_amd import _lib                    # noqa: E402
from tests import ccsds_cases as cc               # noqa: E402

GRID = 2048      # the source grid of the GPU tests: 64 x 32
SHORT = 1500     # values of a bitmapped row of that grid


def smooth(rng, n, xmax, step):
    return np.clip(np.cumsum(rng.integers(-step, step + 1, n)) + xmax // 2, 0, xmax).astype(np.uint64)


def contents(kind, rng, n, nbits, block):
    xmax = (1 << nbits) - 1
    if kind == "noise":          # white noise: uncompressed blocks
        return rng.integers(0, xmax + 1, n, dtype=np.uint64)
    if kind == "smooth":         # small steps: split-sample with a small k
        return smooth(rng, n, xmax, 2)
    if kind == "rough":          # larger steps: split-sample with k > 0
        return smooth(rng, n, xmax, min(200, max(xmax // 8, 1)))
    if kind == "near_constant":  # a rare step of one: second extension, zero blocks between
        return np.clip(xmax // 3 + np.cumsum(rng.random(n) < 0.08) % 2, 0, xmax).astype(np.uint64)
    if kind == "extremes":       # values sitting at 0 and 2^nbits - 1: the mapper's clamped branch
        v = np.where(rng.random(n) < 0.5, 0, xmax).astype(np.uint64)
        v[n // 2:] = np.where(rng.random(n - n // 2) < 0.9, xmax, xmax - min(xmax, 1))
        return v
    if kind == "runs":           # constant runs of >= 5 blocks that cross a 64-block segment boundary, smooth between
        v = smooth(rng, n, xmax, 3)
        for first, blocks in ((58, 12), (100, 7), (130, 80)):
            a, b = first * block, (first + blocks) * block
            if a < n:
                v[a:b] = v[a]
        return v
    if kind == "sparse":         # mostly zero with the preprocessor off: zero blocks of raw samples
        return np.where(rng.random(n) < 0.02, rng.integers(0, min(xmax, 7) + 1, n), 0).astype(np.uint64)
    raise KeyError(kind)


def cases():
    out = []
    # the edges of a block and of an interval, small J and rsi so that both fall inside a few hundred samples
    J, rsi = 8, 2
    sizes = (5, J - 1, J, J + 1, J * rsi, J * rsi + 1, 2 * J * rsi + J + 3)
    kinds = ("smooth", "noise", "near_constant", "extremes", "rough", "smooth", "near_constant")
    for i, n in enumerate(sizes):
        for pp in (1, 0):
            nbits = cc.WIDTHS[(i + 3 * pp) % len(cc.WIDTHS)]
            out.append((f"edge_n{n}_w{nbits}_pp{pp}", kinds[i], n, nbits, J, rsi, pp, 0))
    for J in (16, 32, 64):       # the same edges for the other block sizes, three intervals with a ragged last block
        out.append((f"ragged_j{J}_w12_pp1", "smooth", 2 * J * 3 + J + 5, 12, J, 3, 1, 0))
        out.append((f"ragged_j{J}_w17_pp0", "sparse", 2 * J * 3 + J + 5, 17, J, 3, 0, 0))
    # rows of the GPU tests' grid: every width, both settings, the parameters ecCodes writes among them
    eccodes = cc.MSB | cc.THREE_BYTE
    out += [("grid_w12_smooth", "smooth", GRID, 12, 32, 128, 1, eccodes),
            ("grid_w16_runs", "runs", GRID, 16, 8, 128, 1, eccodes),
            ("grid_w8_near_constant", "near_constant", GRID, 8, 16, 4, 1, 0),
            ("grid_w24_noise", "noise", GRID, 24, 64, 2, 1, eccodes),
            ("grid_w32_extremes", "extremes", GRID, 32, 8, 2, 1, 0),
            ("grid_w17_sparse", "sparse", GRID, 17, 32, 16, 0, 0),
            ("grid_w1_bits", "noise", GRID, 1, 8, 64, 1, 0),
            ("grid_w16_rough", "rough", GRID, 16, 16, 4096, 1, eccodes),
            ("grid_w12_noise_pp0", "noise", GRID, 12, 32, 128, 0, cc.MSB),
            ("grid_w32_smooth", "smooth", GRID, 32, 64, 1, 1, 0),
            ("short_w16_smooth", "smooth", SHORT, 16, 32, 128, 1, eccodes),
            ("short_w12_rough", "rough", SHORT, 12, 16, 8, 1, 0),
            ("short_w24_runs", "runs", SHORT, 24, 8, 128, 0, 0)]
    return out


def main():
    assert cc.load_libaec() is not None, "libaec is not installed here (or set SMM_LIBAEC to its path)"
    os.makedirs(cc.GOLDEN, exist_ok=True)
    rng = np.random.default_rng(20231019)
    hist = cc.new_histogram()
    for name, kind, n, nbits, block, rsi, pp, extra in cases():
        values = contents(kind, rng, n, nbits, block)
        stream = cc.aec_encode(values, nbits, block, rsi, pp)
        flags = (cc.PREPROCESS if pp else 0) | extra
        assert np.array_equal(cc.aec_decode_libaec(stream, n, nbits, block, rsi, pp), values.astype(np.uint32)), name
        assert np.array_equal(cc.host_decode(stream, n, nbits, block, rsi, flags, hist), values.astype(np.uint32)), name
        path = os.path.join(cc.GOLDEN, name + ".npz")
        np.savez_compressed(path, stream=stream, values=values.astype(np.uint32), nbits=np.int32(nbits),
                            block_size=np.int32(block), rsi=np.int32(rsi), flags=np.uint32(flags))
        assert os.path.getsize(path) < 256 * 1024, name
    taken = dict(zip(_lib.GRIB_AEC_OPTIONS, hist.tolist()))
    print(taken)
    assert all(taken.values()), f"a coding option is never taken: {taken}"


if __name__ == "__main__":
    main()
