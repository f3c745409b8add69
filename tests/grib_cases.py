"""GRIB simple packing built from chosen integers, for the tests of smm_apply_grib and friends: data sections and
`GRIB_ROW_DTYPE` row tables where q, nbits, E, D, ref and the byte offset are all picked by the test, and a reference
decoder that shares nothing with the product -- the chosen (or Python-integer extracted) q, then griblite's numpy
statement `(ref + x * scale) / 10.0 ** D` verbatim, then `.astype(float32)`."""
import numpy as np

from smmregrid_amd import GRIB_ROW_DTYPE

WIDTHS = (0, 1, 7, 12, 16, 17, 24, 25, 31, 32)


def pack_bits(q, nbits):
    """The big-endian bit stream of the integers q, nbits each, padded with zero bits to a whole byte."""
    q = np.asarray(q, dtype=np.uint64).ravel()
    if nbits == 0:
        return b""
    bits = ((q[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8).ravel()
    return np.packbits(bits).tobytes()


def unpack_ints(raw, nbits, count):
    """Python-integer extraction: the whole stream as one big integer, each value cut out by shift and mask."""
    if nbits == 0:
        return np.zeros(count, dtype=np.uint64)
    raw = bytes(raw)[:(count * nbits + 7) // 8]
    total, big = 8 * len(raw), int.from_bytes(raw, "big")
    mask = (1 << nbits) - 1
    return np.array([(big >> (total - (i + 1) * nbits)) & mask for i in range(count)], dtype=np.uint64)


def decode_ref(q, ref, E, D):
    """What griblite computes for a message, then the float32 store of open_grib."""
    x = np.asarray(q).astype(np.float64)
    scale = 2.0 ** E
    with np.errstate(over="ignore", invalid="ignore"):
        packed = (ref + x * scale) / 10.0 ** D
        return packed.astype(np.float32)


def decode_rows(buf, rows, count):
    """The (B, count) float32 field of a row table over `buf`, by the reference decoder."""
    raw = np.asarray(buf, dtype=np.uint8).tobytes()
    out = np.empty((len(rows), count), dtype=np.float32)
    for i, r in enumerate(rows):
        nbits, off = int(r["nbits"]), int(r["byte_off"])
        x = unpack_ints(raw[off:off + (count * nbits + 7) // 8], nbits, count).astype(np.float64)
        with np.errstate(over="ignore", invalid="ignore"):
            out[i] = ((float(r["ref"]) + x * float(r["bscale"])) / float(r["ddiv"])).astype(np.float32)
    return out


def random_q(rng, count, nbits):
    """q = 0, all ones and random, in that mix: the first two values are the extremes."""
    if nbits == 0:
        return np.zeros(count, dtype=np.uint64)
    q = rng.integers(0, 1 << nbits, size=count, dtype=np.uint64, endpoint=False)
    q[0], q[1 % count] = 0, (1 << nbits) - 1
    q[rng.random(count) < 0.02] = (1 << nbits) - 1
    q[rng.random(count) < 0.02] = 0
    return q


def build(specs, rng=None, shuffle=True, tail_residue=None):
    """specs: one dict per batch row with q (integers), nbits, E, D, ref and residue (byte offset mod 4).  The rows'
    data sections are laid into one buffer -- in shuffled order when `shuffle`, each at the next offset with its residue,
    a few garbage bytes between them -- and the last one laid ends exactly at the end of the buffer; tail_residue: the
    buffer length mod 4 wanted (the last section is shifted to reach it).  Returns (buf uint8, rows, field float32
    (B, count)) with the field decoded from the chosen q."""
    rng = np.random.default_rng(7) if rng is None else rng
    order = rng.permutation(len(specs)) if shuffle else np.arange(len(specs))
    rows = np.zeros(len(specs), dtype=GRIB_ROW_DTYPE)
    chunks, pos = [], 0
    for n, i in enumerate(order):
        s = specs[i]
        data = pack_bits(s["q"], s["nbits"])
        want = s.get("residue", 0) % 4
        if n == len(order) - 1 and tail_residue is not None:
            want = (tail_residue - len(data)) % 4
        gap = (want - pos) % 4
        chunks.append(bytes(rng.integers(0, 256, size=gap, dtype=np.uint8).tolist()))
        pos += gap
        rows[i] = (pos, s["ref"], 2.0 ** s["E"], 10.0 ** s["D"], s["nbits"], 0)
        chunks.append(data)
        pos += len(data)
    buf = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    field = np.stack([decode_ref(s["q"], s["ref"], s["E"], s["D"]) for s in specs])
    return buf, rows, field


def row_specs(rng, count, n_batch, widths, D=(0,), tie_rows=True):
    """n_batch rows over the widths given (cycled), each with its own ref / E / residue; D cycled from `D`.  Widths >= 25
    get bscale = 1, ref = 0 on their first row, which makes float64 -> float32 ties and near-ties (q needs more than 24
    bits); negative and positive E, negative ref."""
    specs = []
    for b in range(n_batch):
        nbits = widths[b % len(widths)]
        if nbits >= 25 and tie_rows and b < len(widths):
            E, ref = 0, 0.0
        else:
            E = int(rng.integers(-12, 9))
            ref = float(np.float32(rng.normal(0.0, 300.0)))       # IEEE f32 / short IBM reference values, some negative
        specs.append(dict(q=random_q(rng, count, nbits), nbits=nbits, E=E, D=D[b % len(D)], ref=ref, residue=b % 4))
    return specs
