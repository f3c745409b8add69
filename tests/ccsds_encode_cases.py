"""Hand-built integers for the CCSDS encoder, shared by tests/test_grib_ccsds_encode.py (smm_grib_aec_encode_host) and
tests/test_gpu_grib_ccsds_encode.py (smm_grib_aec_pack).  A case: name, the integers, nbits, block size, reference
sample interval, preprocessor, and -- where the rule determines it -- the histogram the stream must decode with, in the
order of `_lib.GRIB_AEC_OPTIONS`: zero run, zero run coded ROS, second extension, split k = 0, split k > 0, uncompressed,
blocks with a reference sample (None: that bin is not pinned).  Plain numpy, no GPU."""
import numpy as np

from smmregrid_amd import _lib

PREPROCESS = _lib.GRIB_AEC_PREPROCESS


class Case:
    def __init__(self, name, q, nbits, block, rsi, pp, hist=None):
        self.name, self.values = name, np.asarray(q, dtype=np.uint32)
        self.nbits, self.block, self.rsi, self.preprocess, self.hist = nbits, block, rsi, bool(pp), hist
        self.flags = PREPROCESS if pp else 0
        self.n_values = int(self.values.size)
        assert self.n_values == 0 or int(self.values.max()) < 2 ** nbits, name

    def __repr__(self):
        return self.name


def _walk(rng, n, nbits, step=3):
    top = 2 ** nbits - 1
    return np.clip(top // 2 + np.cumsum(rng.integers(-step, step + 1, n)), 0, top)


def _blocks(pattern, J, noise):
    """One block per character: 'N' a block of the noise values (never all zero), 'Z' a block of zeros."""
    out = []
    for i, c in enumerate(pattern):
        out.append(np.zeros(J, dtype=np.uint32) if c == "Z" else noise[(i * J) % (noise.size - J):][:J])
    return np.concatenate(out)


def edge_cases():
    rng = np.random.default_rng(42)
    cases = []
    # the ends of the last block and of the first reference sample interval: J = 8, rsi = 4, 32 samples an interval
    for n in (1, 7, 8, 9, 31, 32, 33):
        for pp in (1, 0):
            cases.append(Case(f"n{n}_pp{pp}", _walk(rng, n, 12), 12, 8, 4, pp))
    # the ID-width boundaries (3 bits up to 8, 4 up to 16, 5 beyond), smooth and rough
    for w in (1, 8, 9, 16, 17, 32):
        cases.append(Case(f"w{w}_smooth", _walk(rng, 150, w, 1 if w == 1 else 2), w, 16, 3, 1))
        cases.append(Case(f"w{w}_rough", rng.integers(0, 2 ** min(w, 10), 150), w, 16, 3, 0))
    noise = rng.integers(1, 200, 4096).astype(np.uint32)
    # an all-zero field: 200 blocks, intervals of 128 = segments of 64, 64, 64 and 8 blocks; the last run ends with the
    # data, not with its segment: fs = 8.  With the preprocessor two of the runs begin at a reference block
    cases.append(Case("all_zero_pp0", np.zeros(1600, np.uint32), 16, 8, 128, 0, [1, 3, 0, 0, 0, 0, 0]))
    cases.append(Case("all_zero_pp1", np.zeros(1600, np.uint32), 16, 8, 128, 1, [1, 3, 0, 0, 0, 0, 2]))
    # runs of 4, 5 and 6 blocks in mid-segment: fs = 3, 5, 6
    cases.append(Case("runs_456_mid", _blocks("N" + "Z" * 4 + "N" + "Z" * 5 + "N" + "Z" * 6 + "N", 8, noise), 8, 8, 64, 0,
                      [3, 0, None, None, None, None, 0]))
    # a run of 4 that ends exactly at a segment's end (fs = 3) and a run of 5 that does (ROS)
    cases.append(Case("runs_45_at_segment_end", _blocks("N" * 60 + "Z" * 4 + "N" * 59 + "Z" * 5, 8, noise), 8, 8, 128, 0,
                      [1, 1, None, None, None, None, 0]))
    # a run of 6 + 6 across a segment boundary splits: ROS up to the boundary, fs = 6 behind it
    cases.append(Case("run_across_segment", _blocks("N" * 58 + "Z" * 12 + "N" * 3, 8, noise), 8, 8, 128, 0,
                      [1, 1, None, None, None, None, 0]))
    # and across the end of an interval of 16 blocks: 4 + 4 (fs = 3 twice), then 6 + 6 (ROS, fs = 6)
    cases.append(Case("run_across_rsi", _blocks("N" * 12 + "Z" * 8 + "N" * 6 + "Z" * 12 + "N" * 2, 8, noise), 8, 8, 16, 0,
                      [3, 1, None, None, None, None, 0]))
    # intervals shorter than a segment and no multiple of one: 5 blocks (runs of 5 = ROS each), 100 blocks (64 + 36)
    cases.append(Case("rsi5_zero", np.zeros(8 * 23, np.uint32), 12, 8, 5, 0, [1, 4, 0, 0, 0, 0, 0]))
    cases.append(Case("rsi100_zero", np.zeros(16 * 230, np.uint32), 12, 16, 100, 1, [1, 4, 0, 0, 0, 0, 3]))
    cases.append(Case("rsi100_mixed", np.concatenate([_walk(rng, 1700, 12), np.zeros(900, np.uint32), _walk(rng, 1000, 12)]),
                      12, 16, 100, 1))
    # an all-zero reference block: a constant field under the preprocessor -- every symbol is 0, the references are 7
    cases.append(Case("constant_pp1", np.full(8 * 4 * 2 + 3, 7, np.uint32), 8, 8, 4, 1, [3, 0, 0, 0, 0, 0, 3]))
    # 0 / 1 data with few ones: the second extension is the shortest
    cases.append(Case("bits_sparse", (rng.random(16 * 40) < 0.2).astype(np.uint32), 8, 16, 128, 0))
    one = np.array([1, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0], dtype=np.uint32)
    cases.append(Case("second_ext_block", one, 8, 16, 128, 0, [0, 0, 1, 0, 0, 0, 0]))
    # a pair of value 91 = (13, 0) among the same small values: the second extension is no candidate; (12, 0) = 78 is
    over = one.copy()
    over[4] = 13
    cases.append(Case("pair_above_90", over, 8, 16, 128, 0, [0, 0, 0, None, None, None, 0]))
    under = one.copy()
    under[4] = 12
    cases.append(Case("pair_of_78", under, 8, 16, 128, 0))
    # full-range noise: every block uncompressed
    cases.append(Case("noise_w16", rng.integers(0, 2 ** 16, 32 * 9), 16, 32, 128, 0, [0, 0, 0, 0, 0, 9, 0]))
    cases.append(Case("noise_w32_pp1", rng.integers(0, 2 ** 32, 64 * 4), 32, 64, 2, 1, [0, 0, 0, 0, 0, 4, 2]))
    # the extremes alternating at 32 bits: the far branch of the map in every sample
    cases.append(Case("extremes_w32", np.tile(np.array([0, 2 ** 32 - 1], dtype=np.uint64), 100), 32, 8, 4, 1))
    cases.append(Case("extremes_w32_pp0", np.tile(np.array([2 ** 32 - 1, 0], dtype=np.uint64), 100), 32, 8, 4, 0))
    return cases
