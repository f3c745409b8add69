"""CCSDS (GRIB-2 template 5.42) cases shared by tests/test_grib_ccsds.py, tests/test_gpu_grib_ccsds.py and the fixture
generator tests/golden/make_ccsds_fixtures.py.  Plain numpy and ctypes, no GPU.

The fixtures under tests/golden/ccsds/ were written by libaec's encoder; `load_libaec` finds the library where it is
installed (the fuzz test against `aec_buffer_decode` is skipped where it is not; nothing else needs it)."""
import ctypes
import ctypes.util
import glob
import os
import shutil
import sys

import numpy as np

from smmregrid_amd import _lib
from smmregrid_amd.griblite import GRIB_AEC_DTYPE, GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, aec_decode

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "ccsds")
PREPROCESS, MSB, THREE_BYTE = _lib.GRIB_AEC_PREPROCESS, _lib.GRIB_AEC_MSB, _lib.GRIB_AEC_3BYTE
WIDTHS = (1, 8, 12, 16, 17, 24, 32)


# ------------------------------------------------------------------------------------------------ libaec
class AecStream(ctypes.Structure):
    """struct aec_stream of libaec.h"""
    _fields_ = [("next_in", ctypes.c_void_p), ("avail_in", ctypes.c_size_t), ("total_in", ctypes.c_size_t),
                ("next_out", ctypes.c_void_p), ("avail_out", ctypes.c_size_t), ("total_out", ctypes.c_size_t),
                ("bits_per_sample", ctypes.c_uint), ("block_size", ctypes.c_uint), ("rsi", ctypes.c_uint),
                ("flags", ctypes.c_uint), ("state", ctypes.c_void_p)]


_AEC = []


def load_libaec():
    """libaec through ctypes, or None: $SMM_LIBAEC, the loader's search path, then lib/ of the Python and conda prefixes."""
    if _AEC:
        return _AEC[0]
    names = [os.environ.get("SMM_LIBAEC"), ctypes.util.find_library("aec"), "libaec.so.0"]
    prefixes = [sys.prefix, sys.base_prefix, os.environ.get("CONDA_PREFIX")]
    conda = shutil.which("conda")
    if conda:
        prefixes.append(os.path.dirname(os.path.dirname(os.path.realpath(conda))))
    # where conda's installers and container images put a prefix by default
    prefixes += [os.path.expanduser("~/miniconda3"), os.path.expanduser("~/anaconda3"), "/opt/conda"]
    names += [os.path.join(p, "lib", "libaec.so.0") for p in prefixes if p]
    lib = None
    for name in names:
        if not name:
            continue
        try:
            lib = ctypes.CDLL(name)
            break
        except OSError:
            continue
    if lib is not None:
        for fn in (lib.aec_buffer_encode, lib.aec_buffer_decode):
            fn.restype, fn.argtypes = ctypes.c_int, [ctypes.POINTER(AecStream)]
    _AEC.append(lib)
    return lib


def _container(nbits):
    """libaec's sample container without AEC_DATA_3BYTE / AEC_DATA_MSB: 1, 2 or 4 little-endian bytes."""
    return np.dtype("<u1" if nbits <= 8 else "<u2" if nbits <= 16 else "<u4")


def aec_encode(values, nbits, block, rsi, preprocess):
    """The CCSDS stream libaec writes for these unsigned integers (uint8 array)."""
    lib = load_libaec()
    src = np.ascontiguousarray(values, dtype=_container(nbits))
    dst = np.zeros(src.nbytes * 2 + 4096, dtype=np.uint8)
    st = AecStream(src.ctypes.data, src.nbytes, 0, dst.ctypes.data, dst.nbytes, 0, nbits, block, rsi,
                   PREPROCESS if preprocess else 0, None)
    rc = lib.aec_buffer_encode(ctypes.byref(st))
    assert rc == 0, f"aec_buffer_encode: {rc}"
    return dst[:st.total_out].copy()


def aec_decode_libaec(stream, n_values, nbits, block, rsi, preprocess):
    """`aec_buffer_decode` of a stream: the arbiter of the format."""
    lib = load_libaec()
    src = np.ascontiguousarray(stream, dtype=np.uint8)
    dst = np.zeros(n_values, dtype=_container(nbits))
    st = AecStream(src.ctypes.data, src.nbytes, 0, dst.ctypes.data, dst.nbytes, 0, nbits, block, rsi,
                   PREPROCESS if preprocess else 0, None)
    rc = lib.aec_buffer_decode(ctypes.byref(st))
    assert rc == 0, f"aec_buffer_decode: {rc}"
    return dst.astype(np.uint32)


# ------------------------------------------------------------------------------------------------ the project's decoder
def record(byte_off, byte_len, n_values, nbits, block, rsi, flags):
    return np.array((byte_off, byte_len, n_values, nbits, block, rsi, flags, 0), dtype=GRIB_AEC_DTYPE)


def host_decode(stream, n_values, nbits, block, rsi, flags, histogram=None):
    """smm_grib_aec_decode_host on a stream of its own buffer."""
    stream = np.ascontiguousarray(stream, dtype=np.uint8)
    return aec_decode(stream, record(0, stream.size, n_values, nbits, block, rsi, flags), histogram)


def new_histogram():
    return np.zeros(len(_lib.GRIB_AEC_OPTIONS), dtype=np.uint64)


# ------------------------------------------------------------------------------------------------ fixtures
class Fixture:
    def __init__(self, path):
        z = np.load(path)
        self.name = os.path.splitext(os.path.basename(path))[0]
        self.stream = z["stream"]
        self.values = z["values"]
        self.nbits, self.block, self.rsi, self.flags = (int(z[k]) for k in ("nbits", "block_size", "rsi", "flags"))
        self.n_values = int(self.values.size)

    @property
    def preprocess(self):
        return bool(self.flags & PREPROCESS)

    def __repr__(self):
        return self.name


_FIXTURES = []


def fixtures():
    """Every fixture of tests/golden/ccsds, sorted by name; loaded once."""
    if not _FIXTURES:
        _FIXTURES.extend(Fixture(p) for p in sorted(glob.glob(os.path.join(GOLDEN, "*.npz"))))
    return list(_FIXTURES)


def fixture(name):
    return next(f for f in fixtures() if f.name == name)


def pack_bits(q, nbits):
    """The simple-packed twin of the integers: big-endian, nbits each, the last byte zero-padded."""
    if nbits == 0 or len(q) == 0:
        return np.zeros(0, dtype=np.uint8)
    q = np.asarray(q, dtype=np.uint64)
    bits = ((q[:, None] >> np.arange(nbits - 1, -1, -1, dtype=np.uint64)) & np.uint64(1)).astype(np.uint8)
    return np.packbits(bits.ravel())


# ------------------------------------------------------------------------------------------------ GRIB-2 messages
def _section(number, body):
    return (5 + len(body)).to_bytes(4, "big") + bytes([number]) + bytes(body)


def _sm(value, nbytes):
    """sign-and-magnitude"""
    v = abs(int(value)) | ((1 << (8 * nbytes - 1)) if value < 0 else 0)
    return v.to_bytes(nbytes, "big")


def grib2_message(fields, ni, nj):
    """A GRIB-2 message on an ni x nj lon/lat grid (template 3.0) with sections 4 - 7 once per field.  A field is a dict:
    q (the unsigned integers of its present points), nbits, R (a float32 value), E, D, level (Pa, isobaric), step, and
    either nothing more -- template 5.0, the integers simple-packed -- or ccsds=(stream, flags, block_size, rsi) --
    template 5.42 around that stream; bitmap: None, a bool array of ni * nj points, or "previous" (indicator 254)."""
    s1 = (98).to_bytes(2, "big") + (0).to_bytes(2, "big") + bytes([27, 0, 1]) + (2023).to_bytes(2, "big") + \
        bytes([6, 27, 0, 0, 0, 0, 1])
    g = bytearray(58)
    g[0] = 6
    g[16:20], g[20:24] = ni.to_bytes(4, "big"), nj.to_bytes(4, "big")
    g[24:28], g[28:32] = (0).to_bytes(4, "big"), (0xFFFFFFFF).to_bytes(4, "big")
    micro = lambda v: _sm(int(round(v * 1e6)), 4)         # noqa: E731
    dlon, dlat = 360.0 / ni, 180.0 / nj
    g[32:36], g[36:40] = micro(90.0 - dlat / 2), micro(0.0)
    g[40] = 48
    g[41:45], g[45:49] = micro(-90.0 + dlat / 2), micro(360.0 - dlon)
    g[49:53] = int(round(dlon * 1e6)).to_bytes(4, "big")
    g[53:57] = int(round(dlat * 1e6)).to_bytes(4, "big")
    s3 = bytes([0]) + (ni * nj).to_bytes(4, "big") + bytes([0, 0]) + (0).to_bytes(2, "big") + bytes(g)
    body = _section(1, s1) + _section(3, s3)
    for f in fields:
        q, nbits = np.asarray(f["q"], dtype=np.uint64), int(f["nbits"])
        s4 = (0).to_bytes(2, "big") + (0).to_bytes(2, "big") + bytes([0, 0, 2, 0, 0]) + (0).to_bytes(2, "big") + \
            bytes([0, 1]) + int(f.get("step", 0)).to_bytes(4, "big") + bytes([100, 0]) + _sm(int(f.get("level", 85000)), 4) + \
            bytes([255, 255]) + (0xFFFFFFFF).to_bytes(4, "big")
        head = np.array(f.get("R", 0.0), dtype=">f4").tobytes() + _sm(f.get("E", 0), 2) + _sm(f.get("D", 0), 2) + \
            bytes([nbits, 0])
        if f.get("ccsds") is None:
            s5 = q.size.to_bytes(4, "big") + (0).to_bytes(2, "big") + head
            data = pack_bits(q, nbits).tobytes()
        else:
            stream, flags, block, rsi = f["ccsds"]
            s5 = q.size.to_bytes(4, "big") + (42).to_bytes(2, "big") + head + bytes([flags, block]) + int(rsi).to_bytes(2, "big")
            data = np.asarray(stream, dtype=np.uint8).tobytes()
        bitmap = f.get("bitmap")
        if bitmap is None:
            s6 = bytes([255])
        elif isinstance(bitmap, str):
            s6 = bytes([254])
        else:
            s6 = bytes([0]) + np.packbits(np.asarray(bitmap, np.uint8).ravel()).tobytes()
        body += _section(4, s4) + _section(5, s5) + _section(6, s6) + _section(7, data)
    body += b"7777"
    return b"GRIB" + bytes([0, 0, 0, 2]) + (16 + len(body)).to_bytes(8, "big") + body


# ------------------------------------------------------------------------------------------------ one variable, six fields
NI, NJ = 64, 32      # the 2048-cell source grid of the grid_* / short_* fixtures
# (fixture, level in Pa, step, bitmap, R, E, D) in message order: two times of three levels, different widths and coding
# parameters; the 850 hPa fields are bitmapped, the second one through "the bitmap of the field before"
MESSAGE_SPECS = [("short_w16_smooth", 85000, 0, "own", 270.0, -4, 0), ("short_w12_rough", 85000, 6, "previous", 0.0, 2, 2),
                 ("grid_w16_runs", 50000, 0, None, -12.5, -6, 1), ("grid_w24_noise", 50000, 6, None, 1.0e3, -10, 0),
                 ("grid_w12_smooth", 25000, 0, None, 250.0, -3, 0), ("grid_w8_near_constant", 25000, 6, None, 3.0, 0, 0)]


def message_present():
    """The 1500 points the bitmapped fields hold."""
    present = np.zeros(NI * NJ, dtype=bool)
    present[np.random.default_rng(5).permutation(NI * NJ)[:1500]] = True
    return present


def message_fields(ccsds):
    """The fields of MESSAGE_SPECS for `grib2_message`: CCSDS-packed around the fixtures' streams, or their
    simple-packed twins of the same integers."""
    fields = []
    for name, level, step, bitmap, R, E, D in MESSAGE_SPECS:
        fx = fixture(name)
        fields.append(dict(q=fx.values, nbits=fx.nbits, R=R, E=E, D=D, level=level, step=step,
                           bitmap=message_present() if bitmap == "own" else bitmap,
                           ccsds=(fx.stream, fx.flags, fx.block, fx.rsi) if ccsds else None))
    return fields


# ------------------------------------------------------------------------------------------------ the rows of one call
GRID_ROWS = ["grid_w12_smooth", "grid_w16_runs", "grid_w8_near_constant", "grid_w24_noise", "grid_w32_extremes",
             "grid_w17_sparse", "grid_w1_bits", "grid_w16_rough"]                                   # B = 8, all different
SHORT_ROWS = ["short_w16_smooth", "short_w12_rough", "short_w24_runs"]                              # 1500 values: bitmapped
CALLS = {"plain": dict(names=GRID_ROWS),
         "bitmaps": dict(names=GRID_ROWS[:4] + SHORT_ROWS + GRID_ROWS[4:5], bitmapped={4: 4, 5: 4, 6: 6}),
         # short_w16_smooth owns the bitmap, the two others share it; grid_w16_runs and short_w12_rough stay simple-packed
         "mixed": dict(names=GRID_ROWS[:5] + SHORT_ROWS, bitmapped={5: 5, 6: 5, 7: 5}, simple=(1, 6))}


def rules(n, seed=1):
    """R, 2^E, 10^D of n rows: different in every row, with and without the division."""
    rng = np.random.default_rng(seed)
    rows = np.zeros(n, dtype=GRIB_ROW_DTYPE)
    rows["ref"] = np.float32(rng.uniform(-300.0, 300.0, n))
    rows["bscale"] = np.ldexp(1.0, rng.integers(-12, 3, n))
    rows["ddiv"] = 10.0 ** rng.integers(0, 3, n)
    return rows


def build(names, bitmapped=(), simple=(), seed=1):
    """The rows `names` as one CCSDS call and as its simple-packed twin: (buf, rows, ccsds, bitmaps) twice.  Streams lie
    at odd offsets with garbage between them.  bitmapped: {row: row whose bitmap it shares, or itself}; simple: rows
    that are simple-packed in the CCSDS call too (block_size 0)."""
    S = NI * NJ
    fxs = [fixture(n) for n in names]
    rows = rules(len(fxs), seed)
    rows["nbits"] = [f.nbits for f in fxs]
    twin_rows, aec = rows.copy(), np.zeros(len(fxs), dtype=GRIB_AEC_DTYPE)
    bms = np.zeros(len(fxs), dtype=GRIB_BITMAP_DTYPE)
    bms["bitmap_off"], bms["n_values"] = GRIB_NO_BITMAP, S
    twin_bms = bms.copy()
    parts, twin_parts = [], []

    def put(store, data):
        at = sum(p.size for p in store) + 3                       # three bytes of garbage ahead of every piece
        store.extend([np.full(3, 0xA5, np.uint8), np.asarray(data, np.uint8)])
        return at
    present = message_present()
    for i, f in enumerate(fxs):
        packed = pack_bits(f.values, f.nbits)
        twin_rows["byte_off"][i] = put(twin_parts, packed)
        if i in simple:
            rows["byte_off"][i] = put(parts, packed)
        else:
            rows["byte_off"][i] = off = put(parts, f.stream)
            aec[i] = (off, f.stream.size, f.n_values, f.nbits, f.block, f.rsi, f.flags, 0)
    for i, owner in dict(bitmapped).items():
        assert fxs[i].n_values == 1500
        if owner == i:
            bits = np.packbits(present)
            bms["bitmap_off"][i], twin_bms["bitmap_off"][i] = put(parts, bits), put(twin_parts, bits)
        else:
            bms["bitmap_off"][i], twin_bms["bitmap_off"][i] = bms["bitmap_off"][owner], twin_bms["bitmap_off"][owner]
        bms["n_values"][i] = twin_bms["n_values"][i] = 1500
    use_bm = bool(bitmapped)
    return ((np.concatenate(parts), rows, aec, bms if use_bm else None),
            (np.concatenate(twin_parts), twin_rows, None, twin_bms if use_bm else None))
