"""smm_grib_pack alone on the GPU: synthetic float64 Y, no operator.  Every comparison is bytes for bytes against
`GribEncode.encode` of the same values -- the row records, the bitmap records and the whole buffer -- on the rows of
tests/grib_pack_cases.py (no missing cell, random missing at 5 / 50 / 95 %, all missing, one present cell first or last,
constant, constant with holes, exact half steps, adjacent doubles, about 1e30, above FLT_MAX, +-inf, a subnormal range,
signed zeros), widths 1, 7, 12, 16, 17, 24, 25, 31, 32 and D -2, 0, 3 mixed within one call."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE, GribEncode, _lib, grib_pack
from smmregrid_amd.device import DeviceArray, mem_info, to_device
from tests import far_cases as fc
from tests import grib_pack_cases as pc

pytestmark = pytest.mark.gpu

SEG = 32768          # cells of one segment of the range and rank kernels


def check(got, rows, bitmaps, want, kinds, what=""):
    for b, kind in enumerate(kinds):
        assert rows[b].tobytes() == want.rows[b].tobytes(), (what, b, kind, rows[b], want.rows[b])
        assert bitmaps[b].tobytes() == want.bitmaps[b].tobytes(), (what, b, kind, bitmaps[b], want.bitmaps[b])
    diff = np.flatnonzero(got[:want.buf.size] != want.buf)
    assert diff.size == 0, f"{what}: {diff.size} bytes differ, first at {diff[:5].tolist()}"


@pytest.mark.parametrize("n_dst", [1, 31, 32, 33, 63, 64, 65, SEG - 1, SEG, SEG + 1, 2 * SEG + 37])
def test_pack_matches_the_numpy_rule_bytewise(hip, n_dst):
    values, nbits, dec, kinds = pc.batch(n_dst, seed=n_dst, passes=2 if n_dst < 1000 else 1)
    nbits, dec = nbits[:len(kinds)], dec[:len(kinds)]
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    out, rows, bitmaps = grib_pack(to_device(values), enc)
    check(out.to_host(), rows, bitmaps, want, kinds, f"n_dst={n_dst}")


def test_wider_pitch_with_garbage_in_the_pad_and_canary_bytes_behind_the_layout(hip):
    n_dst, ldy, canary = 1000, 1024, 4096
    values, nbits, dec, kinds = pc.batch(n_dst, seed=11)
    wide = np.full((values.shape[0], ldy), np.nan)
    wide[:, n_dst + 1::2] = 1e300
    wide[:, n_dst + 2::4] = -np.inf
    wide[:, :n_dst] = values
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    total = want.buf.size
    out = DeviceArray((total + canary,), np.uint8).fill_bytes(0x5A)
    got, rows, bitmaps = grib_pack(to_device(wide), enc, n_points=n_dst, out=out)
    host = got.to_host()
    check(host, rows, bitmaps, want, kinds, "pitch")
    assert (host[total:] == 0x5A).all()                               # nothing behind the layout was touched


def test_every_byte_of_the_layout_is_written(hip):
    """The buffer starts as 0xFF: pad bits of the bitmap, the unused bits of a stream's last word and the stream bytes of
    width-0 and sparse rows must all come back zero."""
    n_dst = 77
    values, nbits, dec, kinds = pc.batch(n_dst, seed=5)
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    out = DeviceArray((want.buf.size,), np.uint8).fill_bytes(0xFF)
    got, rows, bitmaps = grib_pack(to_device(values), enc, out=out)
    check(got.to_host(), rows, bitmaps, want, kinds, "prefilled")


def test_launches_split_at_the_grid_limit(hip):
    """smm_debug_set_grid_limit lowers the largest grid: the rows go out in several launches, with the same bytes."""
    n_dst = SEG + 5
    values, nbits, dec, kinds = pc.batch(n_dst, seed=9, passes=1)
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    blocks_per_row = -(-(n_dst * 32 // 32) // 256)                   # the widest row: 32 bits, one word per cell
    _lib.call("smm_debug_set_grid_limit", 3 * blocks_per_row + 1)     # three rows per launch
    try:
        out, rows, bitmaps = grib_pack(to_device(values), enc)
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    check(out.to_host(), rows, bitmaps, want, kinds, "split")


def test_a_row_that_starts_past_2_32_elements(hip):
    """Five short Y rows on a pitch of 2^30 + K elements: row 2 starts past 2^31 elements, row 4 past 2^32.  The buffer
    is filled with finite decoys of another mean, so a row offset narrowed on its way into a kernel packs wrong bits."""
    n_dst = 300
    lay, ldy = fc.rows_layout(5, n_dst)
    need = lay.size * 8
    free = mem_info()[0]
    if free < need + (2 << 30):
        pytest.skip(f"{free / 2 ** 30:.1f} GiB of device memory free, the case needs {need / 2 ** 30:.1f} GiB + 2 GiB")
    values, nbits, dec, kinds = pc.batch(n_dst, seed=13, passes=1)
    pick = [kinds.index(k) for k in ("full", "missing50", "ties", "one_last", "inf")]
    values, nbits, dec, kinds = values[pick], nbits[pick], dec[pick], [kinds[i] for i in pick]
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    y = DeviceArray((lay.size,), np.float64).fill_random(seed=1, mean=1000.0, sigma=50.0)
    try:
        for o, v in zip(lay.offsets, values):
            DeviceArray((n_dst,), np.float64, ptr=y.ptr + o * 8, base=y).copy_from_host(v)
        assert lay.offsets[-1] >= 2 ** 32 and ldy == lay.offsets[1] - lay.offsets[0]
        rec = enc.records(5)
        rows, bitmaps = np.zeros(5, dtype=GRIB_ROW_DTYPE), np.zeros(5, dtype=GRIB_BITMAP_DTYPE)
        out = DeviceArray((want.buf.size,), np.uint8).fill_bytes(0xFF)
        _lib.call("smm_grib_pack", 0, ctypes.c_void_p(y.ptr + lay.offsets[0] * 8), ldy, n_dst, 5,
                  ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)), ctypes.c_void_p(out.ptr), out.nbytes,
                  ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
                  ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), None)
        check(out.to_host(), rows, bitmaps, want, kinds, "far")
    finally:
        y.free()
