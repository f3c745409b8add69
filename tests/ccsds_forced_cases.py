"""CCSDS 121.0-B streams whose coding options are chosen by the test, not by an encoder: shared by
tests/test_grib_ccsds_forced.py (the host decoder) and tests/test_gpu_grib_ccsds_forced.py (smm_grib_aec_unpack).
Plain numpy, no GPU, no libaec, none of the project's encode or decode functions.  Three independent statements of the
format text in the head of smmregrid_amd/csrc/smm_grib_aec.hpp:

  write_stream   a writer that codes every block with the option a `plan` names (numpy, its own bit writer and its own
                 statement of the preprocessor's map), and refuses a plan the format cannot carry
  ref_decode     a decoder in plain Python over the stream as a string of '0' / '1': one loop per block, one `if` per
                 option, the inverse map.  It shares nothing with the writer beyond the bit order
  window_walk    the parse kernel's window rule restated: where every block starts relative to the window base

A plan is a list with one entry per CODE of the row (a zero run is one code that stands for c blocks):
  "raw" | "se" | ("split", k) | ("zero", c, "count" | "ros")

Cases are built in the domain of the coded symbols (so that an option fits by construction) and turned into sample
values with the inverse map; that the writer's forward map gives the symbols back is what `ref_decode(stream) ==
values` then shows.  Every seed is fixed."""
from typing import NamedTuple

import numpy as np

PREPROCESS = 8                      # AEC_DATA_PREPROCESS, section 5's flag bit
WIN_WORDS, REFILL_AT = 128, 60      # kWinWords, kRefillAt of smm_grib_aec.hip
OPTIONS = ("zero_block", "zero_block_ros", "second_extension", "split_k0", "split_k", "uncompressed", "reference")
OK, EXHAUSTED, INVALID = 0, 1, 2


def id_len(nbits):
    return 3 if nbits <= 8 else 4 if nbits <= 16 else 5


# ------------------------------------------------------------------------------------------------ the writer
class BitWriter:
    """Bits MSB first; `bytes()` pads the last byte with zero bits."""

    def __init__(self):
        self.parts, self.n = [], 0

    def _add(self, bits):
        self.parts.append(bits)
        self.n += bits.size

    def put(self, values, nbits):
        """every value of `values` (or one number) as nbits bits"""
        v = np.atleast_1d(np.asarray(values)).astype(np.uint64)
        if nbits and v.size:
            shifts = np.arange(nbits - 1, -1, -1, dtype=np.uint64)
            self._add(((v[:, None] >> shifts) & np.uint64(1)).astype(np.uint8).ravel())

    def put_fs(self, values):
        """every value as a fundamental sequence: that many zeros, then a one"""
        v = np.atleast_1d(np.asarray(values)).astype(np.int64)
        if v.size:
            ends = np.cumsum(v + 1) - 1
            bits = np.zeros(int(ends[-1]) + 1, np.uint8)
            bits[ends] = 1
            self._add(bits)

    def put_bits(self, bits):
        self._add(np.asarray(bits, dtype=np.uint8))

    def bytes(self):
        return np.packbits(np.concatenate(self.parts)) if self.parts else np.zeros(0, np.uint8)


def premap(values, nbits, span):
    """The symbols the preprocessor codes: the reference sample at the start of every interval of `span` samples, and
    elsewhere the error of the unit-delay predictor (the sample before) folded into 0 .. xmax: with theta the distance
    of the prediction from its nearer bound, an error within +-theta alternates (0, -1, +1, -2, ...), a larger one
    counts on from 2 theta."""
    x = np.asarray(values, dtype=np.int64)
    xmax = (1 << nbits) - 1
    pred = np.concatenate([[0], x[:-1]])
    err = x - pred
    theta = np.minimum(pred, xmax - pred)
    folded = np.where(err >= 0, 2 * err, -2 * err - 1)
    d = np.where(np.abs(err) > theta, theta + np.abs(err), folded)
    d[::span] = x[::span]
    return d


def write_stream(values, nbits, J, rsi, preprocess, plan, strict=True, starts=None):
    """The stream (uint8) of `values` with every block coded as `plan` says.  ValueError on a plan the format cannot
    carry; strict=False lifts only the refusal of a block that breaks the decoder's rule 1 (the FS codes of a block take
    more than J * nbits - nc * k bits).  starts: a list the bit position of every code is appended to."""
    x = np.asarray(values, dtype=np.int64)
    n, xmax, idl = x.size, (1 << nbits) - 1, id_len(nbits)
    if n == 0 or x.min() < 0 or x.max() > xmax:
        raise ValueError("values outside 0 .. 2^nbits - 1, or none")
    nb = -(-n // J)
    sym = premap(x, nbits, J * rsi) if preprocess else x
    sym = np.concatenate([sym, np.zeros(nb * J - n, np.int64)])      # the last block padded with zero symbols
    w, blk = BitWriter(), 0
    for entry in plan:
        if blk >= nb:
            raise ValueError("the plan has more codes than the row has blocks")
        kind = entry if isinstance(entry, str) else entry[0]
        b = blk % rsi
        ref = bool(preprocess) and b == 0
        s = sym[blk * J:(blk + 1) * J]
        coded = s[1:] if ref else s
        if starts is not None:
            starts.append(w.n)
        if kind == "raw":
            w.put(2 ** idl - 1, idl)
            w.put(s, nbits)
            blk += 1
        elif kind == "se":
            first, second = s[0::2].copy(), s[1::2]
            if ref:
                first[0] = 0
            if ((first + second) > 12).any():
                raise ValueError("a second-extension pair sum above 12")
            m = (first + second) * (first + second + 1) // 2 + second
            if strict and int((m + 1).sum()) > J * nbits:
                raise ValueError("rule 1: the second-extension codes take more than J * nbits bits")
            w.put(0, idl)
            w.put(1, 1)
            if ref:
                w.put(s[0], nbits)
            w.put_fs(m)
            blk += 1
        elif kind == "split":
            k, nc = entry[1], coded.size
            if k > 2 ** idl - 3:
                raise ValueError("k above 2^id_len - 3")
            q = coded >> k
            if strict and int(q.sum()) + nc > J * nbits - nc * k:
                raise ValueError("rule 1: the FS codes take more than J * nbits - nc * k bits")
            w.put(k + 1, idl)
            if ref:
                w.put(s[0], nbits)
            w.put_fs(q)
            w.put(coded & ((1 << k) - 1), k)
            blk += 1
        elif kind == "zero":
            _, c, how = entry
            to_end = min(rsi - b, 64 - b % 64)
            if not 1 <= c <= to_end:
                raise ValueError("a zero run that crosses its 64-block segment or its RSI")
            if how == "ros" and c != to_end:
                raise ValueError("ROS runs to the end of the segment or of the RSI")
            if sym[blk * J + (1 if ref else 0):min(blk + c, nb) * J].any():
                raise ValueError("a zero block whose coded symbols are not all zero")
            w.put(0, idl + 1)
            if ref:
                w.put(s[0], nbits)
            w.put_fs(4 if how == "ros" else c - 1 if c <= 4 else c)
            blk += c
        else:
            raise ValueError(f"unknown plan entry {entry!r}")
    if blk < nb:
        raise ValueError("the plan ends before the row does")
    return w.bytes()


def plan_histogram(plan, rsi, preprocess):
    """The option histogram a decoder must count on a stream written by `plan`, in the order of OPTIONS."""
    h, blk = [0] * len(OPTIONS), 0
    for entry in plan:
        kind = entry if isinstance(entry, str) else entry[0]
        if preprocess and blk % rsi == 0:
            h[6] += 1
        if kind == "zero":
            h[1 if entry[2] == "ros" else 0] += 1
            blk += entry[1]
            continue
        h[5 if kind == "raw" else 2 if kind == "se" else 3 if entry[1] == 0 else 4] += 1
        blk += 1
    return h


# ------------------------------------------------------------------------------------------------ the reference decoder
def unmap_all(symbols, nbits, span):
    """The samples of the symbols `premap` makes, sample after sample."""
    xmax, out, x = (1 << nbits) - 1, [], 0
    for i, d in enumerate(symbols):
        d = int(d)
        if i % span == 0:
            x = d
        else:
            theta = min(x, xmax - x)
            if d <= 2 * theta:
                x += d // 2 if d % 2 == 0 else -(d + 1) // 2
            elif x <= xmax - x:
                x += d - theta          # beyond the reach below the prediction: up
            else:
                x -= d - theta
        out.append(x)
    return out


def parse(stream, n_values, nbits, J, rsi, preprocess):
    """(symbols, bit position of every code) of a well-formed stream; ValueError where it ends early."""
    s = "".join(format(int(v), "08b") for v in np.asarray(stream, dtype=np.uint8))
    idl, pos, b = id_len(nbits), 0, 0
    symbols, starts = [], []

    def take(n):
        nonlocal pos
        if pos + n > len(s):
            raise ValueError("the stream ends early")
        v = int(s[pos:pos + n], 2) if n else 0
        pos += n
        return v

    def fs():
        nonlocal pos
        end = s.find("1", pos)
        if end < 0:
            raise ValueError("the stream ends early")
        v, pos = end - pos, end + 1
        return v

    while len(symbols) < n_values:
        starts.append(pos)
        ref = bool(preprocess) and b == 0
        ident, blocks = take(idl), 1
        if ident == 2 ** idl - 1:
            block = [take(nbits) for _ in range(J)]
        elif ident == 0:
            second = take(1)
            head = [take(nbits)] if ref else []
            if second:
                block = []
                for _ in range(J // 2):
                    m, t = fs(), 0
                    while (t + 1) * (t + 2) // 2 <= m:
                        t += 1
                    bb = m - t * (t + 1) // 2
                    block += [t - bb, bb]
                if ref:
                    block[0] = head[0]
            else:
                f = fs()
                blocks = min(rsi - b, 64 - b % 64) if f == 4 else f if f > 4 else f + 1
                block = head + [0] * (blocks * J - len(head))
        else:
            k = ident - 1
            head = [take(nbits)] if ref else []
            quot = [fs() for _ in range(J - len(head))]
            block = head + [(q << k) + take(k) for q in quot]
        symbols += block
        b = (b + blocks) % rsi
    return symbols[:n_values], starts


def ref_decode(stream, n_values, nbits, J, rsi, preprocess):
    symbols, _ = parse(stream, n_values, nbits, J, rsi, preprocess)
    return np.array(unmap_all(symbols, nbits, J * rsi) if preprocess else symbols, dtype=np.uint32)


# ------------------------------------------------------------------------------------------------ the window
class Step(NamedTuple):
    entry: int        # the code's start in bits from the window base in force when the decoder reaches it
    refilled: bool    # the window is loaded anew here: the first code, and every entry of 32 * REFILL_AT bits or more
    distance: int     # ... from the base in force while the code is parsed


def window_walk(stream, byte_off, n_values, nbits, J, rsi, preprocess):
    """A Step per code of the row: the parse kernel keeps WIN_WORDS 32-bit words of the buffer from a base word on and
    moves the base to the word of the cursor at a code's start when the cursor is REFILL_AT words or more into it."""
    _, starts = parse(stream, n_values, nbits, J, rsi, preprocess)
    steps, base = [], None
    for st in starts:
        pos = 8 * byte_off + st
        entry = pos & 31 if base is None else pos - 32 * base
        refilled = base is None or (pos >> 5) - base >= REFILL_AT
        if refilled:
            base = pos >> 5
        steps.append(Step(entry, refilled, pos - 32 * base))
    return steps


# ------------------------------------------------------------------------------------------------ cases
class Case(NamedTuple):
    name: str
    group: str
    values: np.ndarray      # uint32: the integers the stream codes (G: what a decoder leaves behind)
    nbits: int
    block: int
    rsi: int
    preprocess: bool
    plan: list
    stream: np.ndarray
    meta: dict              # D: target, distance, off4, step; E: end4; G: status, bad_from

    @property
    def n_values(self):
        return int(self.values.size)

    @property
    def flags(self):
        return PREPROCESS if self.preprocess else 0

    @property
    def J(self):
        return self.block

    def __repr__(self):
        return self.name


def values_of(symbols, nbits, span, preprocess):
    return np.array(unmap_all(symbols, nbits, span) if preprocess else [int(v) for v in symbols], dtype=np.uint32)


def make_case(name, group, nbits, J, rsi, pp, codes, n_values=None, meta=None, strict=True):
    """codes: (plan entry, the symbols of the blocks it stands for) in row order."""
    plan = [c[0] for c in codes]
    symbols = np.concatenate([np.asarray(c[1], dtype=np.int64) for c in codes])
    if n_values is not None:
        symbols = symbols[:n_values]
    values = values_of(symbols, nbits, J * rsi, pp)
    stream = write_stream(values, nbits, J, rsi, pp, plan, strict=strict)
    return Case(name, group, values, nbits, J, rsi, bool(pp), plan, stream, dict(meta or {}))


def spread(total, n, cap):
    """n numbers <= cap that sum to total, as even as can be"""
    assert 0 <= total <= n * cap, (total, n, cap)
    return np.array([total // n + (i < total % n) for i in range(n)], dtype=np.int64)


def split_kmax(nbits, J, ref):
    """The largest k a decodable split block can have: the ID carries k <= 2^id_len - 3, and the nc codes need a bit each
    within rule 1's limit, nc (k + 1) <= J nbits (the issue's nc k < J nbits leaves the limit positive but may leave
    fewer than nc bits).  That is nbits - 1 in a plain block, and nbits in a reference block where nbits >= J - 1."""
    nc = J - (1 if ref else 0)
    return min(2 ** id_len(nbits) - 3, J * nbits // nc - 1)


def option_block(rng, option, nbits, J, ref):
    """(plan entry, J symbols) of one block that `option` can code, or None where the format has no such block."""
    xmax, nc = (1 << nbits) - 1, J - (1 if ref else 0)
    refval = [int(rng.integers(1, xmax + 1))] if ref else []
    if option == "raw":
        s = rng.integers(0, xmax + 1, J)
        s[rng.integers(0, J, 4)] = [xmax, max(xmax - 1, 0), 0, 1]         # the bounds and their neighbours
        # under the preprocessor the symbol xmax is the jump to the far bound, whatever the sample before: the samples
        # go bound, other bound, bound, then (xmax - 1) next to the other bound, then a folded step of one
        at = int(rng.integers(1, J - 5))
        s[at:at + 5] = [xmax, xmax, xmax, xmax - 1, 1]
        if ref:
            s[0] = refval[0]
        return "raw", s
    if option == "zero":
        return ("zero", 1, "count"), np.array(refval + [0] * nc)
    if option == "se":
        budget, pairs = J * nbits, []
        for i in range(J // 2):
            a, bb = int(rng.integers(0, min(xmax, 12) + 1)), 0
            bb = int(rng.integers(0, min(xmax, 12 - a) + 1))
            if ref and i == 0:
                a = 0
            m = (a + bb) * (a + bb + 1) // 2 + bb
            if m + 1 > budget - (J // 2 - 1 - i):                         # a bit is left for each code behind
                a, bb, m = 0, 0, 0
            budget -= m + 1
            pairs += [a, bb]
        if ref:
            pairs[0] = refval[0]
        return "se", np.array(pairs)
    k = {"split0": 0, "split1": 1, "splitmax": split_kmax(nbits, J, ref)}[option]
    extra = J * nbits - nc * k - nc                                       # zeros the FS part may hold
    if extra < 0 or k > 2 ** id_len(nbits) - 3:
        return None
    rem = rng.integers(0, 1 << k, nc) if k else np.zeros(nc, np.int64)
    if k >= nbits:
        rem = np.minimum(rem, xmax)
    quot = np.zeros(nc, np.int64)
    for i in rng.permutation(nc):
        top = min(extra, 5, (xmax - int(rem[i])) >> k) if k < nbits else 0
        quot[i] = rng.integers(0, top + 1)
        extra -= int(quot[i])
    return ("split", k), np.array(refval + list((quot << k) + rem))


A_WIDTHS = (1, 2, 3, 4, 5, 7, 8, 9, 12, 15, 16, 17, 24, 25, 31, 32)
A_OPTIONS = ("raw", "se", "split0", "split1", "splitmax", "zero")


def group_a():
    """Per (width, J, preprocessor) six rows of eight blocks, rsi = 3: blocks 0, 3, 6 carry a reference sample, block 7
    is the padded last one with 1 or J - 1 samples.  Block i of row r takes option (i + r) mod 6, so over the six rows
    every block position meets every option; an option the format cannot code at that size (split 1 at one bit) gives
    its place to split 0, under preprocessing all symbols of a raw block at 1 bit alternate 0 / xmax."""
    cases = []
    for nbits in A_WIDTHS:
        for J in (8, 16, 32, 64):
            for pp in (0, 1):
                for r in range(6):
                    rng = np.random.default_rng([1, nbits, J, pp, r])
                    codes = []
                    for i in range(8):
                        ref = bool(pp) and i % 3 == 0
                        got = option_block(rng, A_OPTIONS[(i + r) % 6], nbits, J, ref) or option_block(rng, "split0", nbits, J, ref)
                        codes.append(got)
                    left = 1 if r % 2 == 0 else J - 1
                    last = codes[7][1].copy()
                    last[left:] = 0                                        # what the writer pads with
                    codes[7] = (codes[7][0], last)
                    cases.append(make_case(f"A_w{nbits}_j{J}_pp{pp}_r{r}", "A", nbits, J, 3, pp, codes, 7 * J + left))
    return cases


def long_code_block(nbits, J, k, where, ref=False, refval=0):
    """A split-k block whose FS part takes exactly rule 1's limit: one long code at position `where`, zeros elsewhere."""
    nc = J - (1 if ref else 0)
    quot = np.zeros(nc, np.int64)
    quot[where] = J * nbits - nc * k - nc
    assert quot[where] << k <= (1 << nbits) - 1
    return ("split", k), np.array(([refval] if ref else []) + list((quot << k) + ((1 << k) - 1 if k else 0)))


def group_b():
    rng = np.random.default_rng(2)
    cases = []
    # w = ceil(limit / 64) bits a lane: 1 (8 x 8), 2 (8 x 16), 31 (64 x 31), 32 (64 x 32), all with k = 0
    for nbits, J, w in ((8, 8, 1), (16, 8, 2), (31, 64, 31), (32, 64, 32)):
        assert -(-J * nbits // 64) == w
        small = option_block(rng, "split0", nbits, J, False)
        codes = [long_code_block(nbits, J, 0, 0), small, long_code_block(nbits, J, 0, J // 2 - 1),
                 long_code_block(nbits, J, 0, J - 1), (("split", 0), np.zeros(J, np.int64)), small]
        cases.append(make_case(f"B_limit_w{w}", "B", nbits, J, 128, 0, codes))
        # the same under a k that leaves room, every remainder all ones (long_code_block sets them), and in a reference block
        k = 2 if nbits > 8 else 1
        ones = (("split", k), np.full(J, (1 << k) - 1))
        codes = [long_code_block(nbits, J, k, 0, True, 5), ones, long_code_block(nbits, J, k, J // 2), ones,
                 long_code_block(nbits, J, k, J - 2, True, (1 << nbits) - 1), long_code_block(nbits, J, k, J - 1)]
        cases.append(make_case(f"B_limit_k{k}_w{-(-(J * nbits - J * k) // 64)}_pp1", "B", nbits, J, 4, 1, codes))
    # second extension: m = 0 throughout; as many m = 90 = (0, 12) as rule 1 lets in, then (12, 0) = 78 and (0, 12)
    for nbits, J in ((4, 64), (12, 16), (32, 64)):
        fit = min(J // 2, (J * nbits - J // 2) // 90)
        m90 = np.array([0, 12] * fit + [0, 0] * (J // 2 - fit))
        mix = np.array(([12, 0, 0, 12] * J)[:2 * min(fit, J // 2)] + [0, 0] * (J // 2 - min(fit, J // 2)))
        assert fit >= 2
        codes = [("se", np.zeros(J, np.int64)), ("se", m90), ("se", mix), ("se", np.zeros(J, np.int64))]
        cases.append(make_case(f"B_se_w{nbits}_j{J}", "B", nbits, J, 128, 0, codes))
    # second extension in reference blocks (the first a is dropped), the last one with an odd number of samples left
    for nbits, J, left in ((9, 8, 5), (17, 32, 1), (32, 16, 15)):
        xmax = (1 << nbits) - 1
        codes = [("se", np.array([xmax - 1, 3] + [1, 2, 0, 0] * (J // 4 - 1) + [2, 0])),
                 ("se", np.array([xmax, 0] + [0, 1] * (J // 2 - 1)))]
        cases.append(make_case(f"B_se_ref_w{nbits}_j{J}_left{left}", "B", nbits, J, 1, 1, codes, J + left))
    return cases


def small_blocks(rng, count, J, pp_first, nbits):
    """`count` split-0 blocks of symbols 0..2; the first with a reference sample where pp_first"""
    out = []
    for i in range(count):
        s = rng.integers(0, 3, J)
        s[0] = 1 + s[0]
        if pp_first and i == 0:
            s[0] = (1 << nbits) // 3 + 1
        out.append((("split", 0), s))
    return out


def group_c():
    rng = np.random.default_rng(3)
    cases, nbits, J = [], 12, 8
    zeros = lambda c: np.zeros(c * J, np.int64)                            # noqa: E731
    raw = lambda: ("raw", rng.integers(1, 1 << nbits, J))                  # noqa: E731
    for c in (1, 2, 3, 4, 5, 6, 63, 64):                                   # by count: fs = c - 1 up to 4, fs = c from 5 on
        pp = c % 2
        run = zeros(c)
        run[0] = 77 * pp                                                    # a run from a reference block on
        cases.append(make_case(f"C_count{c}_pp{pp}", "C", nbits, J, 128, pp, [(("zero", c, "count"), run), raw(), raw()]))
    for t in (1, 4, 5, 64):                                                 # ROS with t blocks to the end of rsi = 64
        codes = small_blocks(rng, 64 - t, J, False, nbits) + [(("zero", t, "ros"), zeros(t)), raw()]
        cases.append(make_case(f"C_ros{t}_to_rsi_end", "C", nbits, J, 64, 0, codes))
    # at a segment's end inside an interval; at an interval's end that is no segment's
    codes = small_blocks(rng, 60, J, True, nbits) + [(("zero", 4, "ros"), zeros(4)), raw(), raw()]
    cases.append(make_case("C_ros_segment_end_rsi130", "C", nbits, J, 130, 1, codes))
    codes = small_blocks(rng, 64, J, False, nbits) + [(("zero", 1, "ros"), zeros(1)), raw()]
    cases.append(make_case("C_ros_rsi65_b64", "C", nbits, J, 65, 0, codes))
    run = zeros(3)
    run[0] = 4000
    cases.append(make_case("C_ros_rsi3_ref", "C", nbits, J, 3, 1, [(("zero", 3, "ros"), run), raw(), (("zero", 2, "ros"), zeros(2))]))
    cases.append(make_case("C_adjacent_runs", "C", nbits, J, 128, 0,
                           [raw(), (("zero", 2, "count"), zeros(2)), (("zero", 3, "count"), zeros(3)), raw()]))
    cases.append(make_case("C_run_from_nonzero_reference_w32", "C", 32, 16, 8, 1,
                           [(("zero", 3, "count"), np.concatenate([[2 ** 32 - 2], np.zeros(47, np.int64)])),
                            ("raw", rng.integers(0, 2 ** 32, 16))]))
    # the last code's blocks reach past n_values: 10 blocks coded, one and three samples of them wanted
    cases.append(make_case("C_run_past_the_end", "C", nbits, J, 128, 0, [raw(), raw(), (("zero", 10, "count"), zeros(10))], 2 * J + 3))
    cases.append(make_case("C_ros_past_the_end", "C", nbits, J, 32, 0, [raw(), (("zero", 31, "ros"), zeros(31))], J + 1))
    return cases


# ---- D: targets at chosen distances from the window base
class Target(NamedTuple):
    name: str
    nbits: int
    J: int
    preprocess: bool
    codes: list          # (plan entry, symbols) of the target and what follows it
    prefix: tuple        # the prefix lengths (in blocks) the target can stand behind: a zero run of 64 starts a segment
    rsi: int             # 0: as many blocks as the prefix has (the target is a reference block)


def targets():
    rng = np.random.default_rng(4)
    big = rng.integers(0, 2 ** 32, 64)
    big[[0, 21, 63]] = [2 ** 32 - 1, 0, 2 ** 32 - 1]
    tail = ("raw", rng.integers(0, 2 ** 32, 8))
    return [Target("raw_w32_j64", 32, 64, False, [("raw", big)], (), 128),                      # 5 + 2048 bits
            Target("raw_w32_j64_ref", 32, 64, True, [("raw", big)], (), 0),
            Target("split_limit_w32_j64", 32, 64, False, [long_code_block(32, 64, 5, 31)], (), 128),   # 5 + 2048 bits
            Target("split_limit_w32_j64_ref", 32, 64, True, [long_code_block(32, 64, 5, 62, True, 2 ** 32 - 1)], (), 0),   # 5 + 32 + 2048
            Target("zero_fs64_w32_j8", 32, 8, False, [(("zero", 64, "count"), np.zeros(512, np.int64)), tail], (0, 64), 128)]


EDGE = 32 * REFILL_AT     # 1920: a code that starts this many bits into the window, or more, reloads it
D_DISTANCES = (0, 1, 31, 32, EDGE - 1, EDGE)


def place(t, distance, byte_off):
    """The target behind split-0 blocks of the same width and J whose symbol sums are tuned so that it starts
    `distance` bits from the window base.  With the stream at byte_off the first code starts 8 (byte_off % 4) bits into
    the first window; a start of 32 REFILL_AT = 1920 bits or more reloads the window from the start's own word on.  So
    8 (byte_off % 4) is reached with no prefix, distances up to 1920 from there on directly, and a small distance d
    through a reload: the target starts 1920 + d bits in (1952 for d = 0 where the direct way is closed).  32 lies
    between: no split-0 block is as short as 32 bits, so the prefix ends with a single zero block (ID, selector, FS of
    one bit) that starts at 1920 + 32 - its length.  The Step of `window_walk` is asserted and returned in meta."""
    nbits, J, pp, idl = t.nbits, t.J, t.preprocess, id_len(t.nbits)
    off8, zlen = 8 * (byte_off % 4), idl + 2
    base_len, cap = idl + J, J * nbits - J                 # a split-0 block's bits with all symbols 0; the sum it may add
    first_extra = nbits - 1 if pp else 0                   # the reference sample, less the symbol it replaces
    lens = [c for c in (t.prefix or range(1, 200)) if c]

    def blocks_for(total, use_zero):
        return next((c for c in lens if (c - use_zero) * base_len + first_extra <= total <= (c - use_zero) * (base_len + cap)), None)
    # the ways to the distance, the shortest first: no prefix, straight there, through a reload
    ways = [(distance - off8, False)]
    if distance <= 31:
        ways.append(((EDGE + distance if distance else EDGE + 32) - off8, False))
    if distance == 32:
        ways.append((EDGE + 32 - zlen - off8, True))
    total, use_zero, count = None, False, 0
    for total, use_zero in ways:
        if total == 0 and (not t.prefix or 0 in t.prefix):
            count = 0
            break
        count = blocks_for(total, use_zero) if total > 0 else None
        if count:
            break
    else:
        raise ValueError(f"{t.name}: no prefix reaches {distance} bits at byte_off % 4 = {byte_off % 4}")
    n_split = count - use_zero
    codes = []
    if n_split:
        slack = total - n_split * base_len - first_extra
        for i in reversed(range(n_split)):                 # the slack goes to the last blocks: each starts below 1920
            nc = J - (1 if pp and i == 0 else 0)
            room = cap if nc == J else J * nbits - nc
            mine = min(slack, room)
            slack -= mine
            s = list(spread(mine, nc, 1 << 31))
            codes.append((("split", 0), np.array(([(1 << nbits) // 2] if nc < J else []) + s)))
        assert slack == 0
        codes.reverse()
    if use_zero:
        codes.append((("zero", 1, "count"), np.zeros(J, np.int64)))
    rsi = t.rsi or max(count, 1)
    case = make_case(f"D_{t.name}_d{distance}_o{byte_off % 4}", "D", nbits, J, rsi, pp, codes + list(t.codes))
    steps = window_walk(case.stream, byte_off, case.n_values, nbits, J, rsi, pp)
    step = steps[count]
    # the one reload on the way is the target's, or that of the zero block before it
    assert not any(st.refilled for st in steps[1:count - use_zero]), (case.name, steps[:count])
    assert step.distance == distance % EDGE and (step.entry == distance or step.refilled), (case.name, step)
    assert distance != EDGE - 1 or not step.refilled
    assert distance != EDGE or (step.refilled and step.entry == EDGE)
    case.meta.update(target=t.name, distance=distance, off4=byte_off % 4, step=step, index=count)
    return case


def group_d():
    return [place(t, d, o) for t in targets() for d in D_DISTANCES for o in (0, 1, 2, 3)]


def group_e():
    """Rows that end with an FS code in the stream's last bits -- a split block, a second extension, a zero run -- and
    one that ends raw, each to be laid so that its last byte falls on every residue mod 4 of the buffer (meta end4);
    the bytes behind are 0xFF, so a decoder that reads an FS code past the stream's end finds ones there."""
    rng = np.random.default_rng(5)
    cases = []
    for end4 in range(4):
        nbits, J = (12, 8) if end4 % 2 else (17, 16)
        s = rng.integers(0, 4, J)
        rows = {"split": [small_blocks(rng, 1, J, True, nbits)[0], (("split", 1), s)],
                "se": [small_blocks(rng, 1, J, True, nbits)[0], ("se", np.array([0, 1] * (J // 2)))],
                "zero": [("raw", rng.integers(1, 1 << nbits, J)), (("zero", 7, "count"), np.zeros(7 * J, np.int64))],
                "raw": [(("zero", 1, "count"), np.array([9] + [0] * (J - 1))), ("raw", rng.integers(1, 1 << nbits, J))]}
        for kind, codes in rows.items():
            n = (len(codes) - 1) * J + 3 if kind != "zero" else 3 * J + 2
            cases.append(make_case(f"E_{kind}_end{end4}", "E", nbits, J, 16, 1, codes, n, meta=dict(end4=end4)))
    return cases


def smooth_walk(rng, n, nbits, step):
    top = (1 << nbits) - 1
    return np.clip(top // 2 + np.cumsum(rng.integers(-step, step + 1, n)), 0, top).astype(np.uint32)


def plan_fixed_k(values, nbits, J, rsi, pp, k):
    """split k in every block, raw where rule 1 refuses that"""
    n = len(values)
    nb = -(-n // J)
    sym = premap(values, nbits, J * rsi) if pp else np.asarray(values, dtype=np.int64)
    sym = np.concatenate([sym, np.zeros(nb * J - n, np.int64)]).reshape(nb, J)
    plan = []
    for blk in range(nb):
        coded = sym[blk, 1:] if pp and blk % rsi == 0 else sym[blk]
        fits = int((coded >> k).sum()) + coded.size <= J * nbits - coded.size * k
        plan.append(("split", k) if fits else "raw")
    return plan


def group_f():
    """[0] the row that enters a second interval of the largest span (J rsi = 2^18 samples); [1] 193 intervals of one
    block: four groups of the inverse kernel, the last partial; [2] two groups, the second of 17 samples."""
    rng = np.random.default_rng(6)
    cases = []
    for name, nbits, J, rsi, n, step, k in (("F_long_2p18", 16, 64, 4096, 2 ** 18 + 70, 40, 4), ("F_rsi1_193_intervals", 12, 8, 1, 1541, 9, 2),
                                            ("F_rsi3_two_groups", 16, 16, 3, 16 * 3 * 64 + 17, 300, 6)):
        values = smooth_walk(rng, n, nbits, step)
        values[n // 2:n // 2 + 2 * J] = values[n // 2]                     # some blocks the fixed k is too large for stay split
        values[n // 3:n // 3 + J] = rng.integers(0, 1 << nbits, J)         # and one it is too small for goes raw
        plan = plan_fixed_k(values, nbits, J, rsi, 1, k)
        assert "raw" in plan and ("split", k) in plan
        cases.append(Case(name, "F", values, nbits, J, rsi, True, plan, write_stream(values, nbits, J, rsi, 1, plan), {}))
    return cases


# ---- G: malformed streams, one change each
def _bits(case):
    starts = []
    stream = write_stream(case.values, case.nbits, case.block, case.rsi, case.preprocess, case.plan, strict=False, starts=starts)
    return np.unpackbits(stream), starts


def _broken(name, case, code, stream, status, note, end4=1):
    """`case` with the stream replaced: the decoder fails in code `code` of the plan with `status`, and leaves the
    samples of the blocks before it and zeros from there on (all G rows are without the preprocessor, or fail in a
    reference block, so the zeros stay zeros)."""
    blocks = sum(e[1] if not isinstance(e, str) and e[0] == "zero" else 1 for e in case.plan[:code])
    values = case.values.copy()
    values[blocks * case.block:] = 0
    return Case(name, "G", values, case.nbits, case.block, case.rsi, case.preprocess, case.plan, np.asarray(stream, np.uint8),
                dict(status=status, bad_from=blocks * case.block, note=note, end4=end4))


def _cut(name, case, code, bit_in_code, note):
    """the stream cut before the byte that holds bit `bit_in_code` of code `code`: that code has begun, the bit is gone"""
    bits, starts = _bits(case)
    keep = (starts[code] + bit_in_code) // 8
    assert keep * 8 > starts[code], (name, starts[code], keep)
    return _broken(name, case, code, np.packbits(bits)[:keep], EXHAUSTED, note)


def _spliced(name, case, code, writer, status, note, tail=(0x55,) * 24, end4=1):
    """the stream up to code `code`, then the bits `writer` holds, padded to a byte, then the bytes `tail` (24 of 0x55,
    so that the stream goes on)"""
    bits, starts = _bits(case)
    w = BitWriter()
    w.put_bits(bits[:starts[code]])
    w.put_bits(np.concatenate(writer.parts))
    stream = np.concatenate([w.bytes(), np.array(tail, dtype=np.uint8)])
    return _broken(name, case, code, stream, status, note, end4)


def group_g():
    rng = np.random.default_rng(7)
    cases = []
    nbits, J = 12, 16
    first = small_blocks(rng, 1, J, False, nbits)[0]
    raw = ("raw", rng.integers(1, 1 << nbits, J))
    # truncated in the middle of each option's body (the body of a zero run is its FS code: 64 zeros and a one)
    bodies = {"raw": (raw, 4 + 100), "se": (("se", np.array([1, 2] * (J // 2))), 5 + 40),
              "split_fs": ((("split", 3), rng.integers(8, 64, J)), 4 + 30), "split_remainders": ((("split", 11), rng.integers(0, 1 << 11, J)), 4 + J + 90),
              "zero_fs": ((("zero", 64, "count"), np.zeros(64 * J, np.int64)), 5 + 30)}
    for kind, (code, bit) in bodies.items():
        good = make_case("good", "G", nbits, J, 128, 0, [code, raw] if kind == "zero_fs" else [first, code, raw])
        at = 0 if kind == "zero_fs" else 1
        cases.append(_cut(f"G_cut_in_{kind}", good, at, bit, "cut inside the body"))
    # truncated inside the ID: the ID 1100 (split k = 11) with its first three bits in the stream's last byte.  Ones
    # behind the end would make it 1101, k = 12, which no block of 16 x 12 bits can have (nc k >= J nbits): a decoder
    # that judges the ID before it looks at the end calls that invalid, and the stream merely ends
    for extra in range(8):
        s = first[1].copy()
        s[1] += extra
        good = make_case("good", "G", nbits, J, 128, 0, [(("split", 0), s), (("split", 11), rng.integers(0, 1 << 11, J)), raw])
        bits, starts = _bits(good)
        if starts[1] % 8 == 5:
            cases.append(_cut("G_cut_in_id_k_too_large_behind", good, 1, 3, "three bits of the ID are left"))
            break
    else:
        raise AssertionError("no prefix puts the ID three bits before a byte's end")
    good = make_case("good", "G", 32, 8, 128, 0, [("raw", rng.integers(0, 2 ** 32, 8)), ("raw", rng.integers(0, 2 ** 32, 8))])
    cases.append(_cut("G_cut_in_id_w32", good, 1, 3, "5 + 256 bits lie before the ID: three of its five bits are left"))
    # truncated inside a reference sample (the second interval's)
    good = make_case("good", "G", 32, 8, 1, 1, [(("split", 2), np.array([2 ** 31 + 5] + [3] * 7)), (("split", 2), np.array([2 ** 32 - 1] + [1] * 7))])
    cases.append(_cut("G_cut_in_reference", good, 1, 5 + 20, "20 bits of the reference sample are left"))
    # an FS part one bit over rule 1
    code, s = long_code_block(nbits, J, 2, 5)
    s = s.copy()
    s[9] += 1 << 2
    cases.append(_broken_rule1("G_fs_one_over_rule1", nbits, J, [first, (code, s), raw, raw]))
    # a second-extension value of 91 = (13, 0)
    good = make_case("good", "G", nbits, J, 128, 0, [first, ("se", np.array([1, 0] * (J // 2))), raw])
    w = BitWriter()
    w.put(0, 4)
    w.put(1, 1)
    w.put_fs([1, 2, 91] + [0] * (J // 2 - 3))
    cases.append(_spliced("G_second_extension_91", good, 1, w, INVALID, "the third value is 91"))
    # the same value with the stream ending in the block behind it.  A decoder that takes the codes in order has met the
    # 91 inside the stream: invalid, not exhausted.  Once with nothing behind the 91's code but the pad bits (ones behind
    # the end complete the block's other codes), once with zero bytes to a word's end (no one ever comes)
    w = BitWriter()
    w.put(0, 4)
    w.put(1, 1)
    w.put_fs([1, 2, 91])
    cases.append(_spliced("G_second_extension_91_then_the_end", good, 1, w, INVALID, "the stream ends behind the 91", tail=()))
    cases.append(_spliced("G_second_extension_91_then_zeros_to_the_end", good, 1, w, INVALID,
                          "8 zero bytes behind the 91, the end on a word's end", tail=(0,) * 8, end4=0))
    # a zero run of more blocks than the interval has left: three blocks from block 1 of an interval of 3
    good = make_case("good", "G", nbits, J, 3, 0, [first, (("zero", 2, "count"), np.zeros(2 * J, np.int64)), raw, raw])
    w = BitWriter()
    w.put(0, 5)
    w.put_fs(2)
    cases.append(_spliced("G_zero_run_past_the_rsi", good, 1, w, INVALID, "fs = 2: three blocks, two are left"))
    # a zero-run FS code of 65 zeros
    good = make_case("good", "G", nbits, J, 128, 0, [first, (("zero", 2, "count"), np.zeros(2 * J, np.int64)), raw])
    w = BitWriter()
    w.put(0, 5)
    w.put_fs(65)
    cases.append(_spliced("G_zero_run_fs_65", good, 1, w, INVALID, "65 zeros before the one"))
    # byte_len one less than needed
    good = make_case("good", "G", nbits, J, 128, 0, [first, (("split", 3), rng.integers(0, 64, J))])
    cases.append(_broken("G_byte_len_one_short", good, 1, good.stream[:-1], EXHAUSTED, "the last byte is missing"))
    return cases


def _broken_rule1(name, nbits, J, codes):
    good = make_case("good", "G", nbits, J, 128, 0, codes, strict=False)
    try:
        write_stream(good.values, nbits, J, 128, 0, good.plan)
    except ValueError as e:
        assert "rule 1" in str(e)
    else:
        raise AssertionError("the strict writer takes the block")
    return _broken(name, good, 1, good.stream, INVALID, "the FS part takes limit + 1 bits")


_CACHE = {}
GROUPS = dict(A=group_a, B=group_b, C=group_c, D=group_d, E=group_e, F=group_f, G=group_g)


def group(letter):
    """The cases of a group, built once."""
    if letter not in _CACHE:
        _CACHE[letter] = GROUPS[letter]()
    return list(_CACHE[letter])


def gather_rows():
    """Eight forced rows of 2048 values for the operator of tests/test_gpu_grib_ccsds.py: the widths the fixtures lack,
    every J, both preprocessor settings, the options in rotation over the blocks."""
    if "gather" not in _CACHE:
        cases = []
        for i, (nbits, J, rsi) in enumerate(((2, 8, 5), (5, 16, 64), (9, 32, 3), (15, 64, 1), (25, 8, 128), (31, 16, 7), (3, 64, 2), (7, 32, 4096))):
            rng, pp = np.random.default_rng([8, i]), i % 2 == 0
            codes = []
            for blk in range(2048 // J):
                ref = pp and blk % rsi == 0
                codes.append(option_block(rng, A_OPTIONS[(blk + i) % 6], nbits, J, ref) or option_block(rng, "split0", nbits, J, ref))
            cases.append(make_case(f"gather_w{nbits}_j{J}_rsi{rsi}_pp{int(pp)}", "A", nbits, J, rsi, pp, codes))
        _CACHE["gather"] = cases
    return list(_CACHE["gather"])
