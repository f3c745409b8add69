"""The GRIB encode that needs no device, in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/grib_pack_harness.cpp): the rule, the bitmap words, the rank table and the word assembly of smm_grib_pack --
the functions of smm_grib_codec.hpp that the kernels run, compiled with plain g++ -ffp-contract=off -- against
`GribEncode.encode` on the rows of tests/grib_pack_cases.py.  Rows, bitmap records and every byte must be identical."""
import os
import subprocess

import numpy as np
import pytest

from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE, GribEncode
from tests import grib_pack_cases as pc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "grib_pack_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_plan.cpp")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib_pack") / "grib_pack_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + SOURCES)
    return exe


def run(exe, tmp_path, values, nbits, dec, n_dst):
    enc = GribEncode(nbits, dec)
    n_rows, ldy = values.shape
    src, dst = str(tmp_path / "cases.bin"), str(tmp_path / "packed.bin")
    with open(src, "wb") as fh:
        fh.write(np.array([n_rows, n_dst, ldy], dtype=np.int64).tobytes())
        fh.write(enc.records(n_rows).tobytes())
        fh.write(np.ascontiguousarray(values, dtype=np.float64).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    raw = open(dst, "rb").read()
    total = int(np.frombuffer(raw, dtype=np.uint64, count=1)[0])
    rows = np.frombuffer(raw, dtype=GRIB_ROW_DTYPE, count=n_rows, offset=8)
    bms = np.frombuffer(raw, dtype=GRIB_BITMAP_DTYPE, count=n_rows, offset=8 + 40 * n_rows)
    buf = np.frombuffer(raw, dtype=np.uint8, offset=8 + 56 * n_rows)
    return enc, total, rows, bms, buf


@pytest.mark.parametrize("n_dst", [1, 31, 32, 33, 63, 64, 65, 1000])
def test_header_encode_matches_numpy_bytewise(harness, tmp_path, n_dst):
    values, nbits, dec, kinds = pc.batch(n_dst, seed=100 + n_dst)
    enc, total, rows, bms, buf = run(harness, tmp_path, values, nbits, dec, n_dst)
    want = enc.encode(values)
    assert total == want.buf.size == buf.size
    for b, kind in enumerate(kinds):
        assert rows[b].tobytes() == want.rows[b].tobytes(), (kind, int(nbits[b]), rows[b], want.rows[b])
        assert bms[b].tobytes() == want.bitmaps[b].tobytes(), (kind, bms[b], want.bitmaps[b])
    diff = np.flatnonzero(buf != want.buf)
    assert diff.size == 0, f"{diff.size} bytes differ, first at {diff[:5].tolist()}"


def test_pad_of_a_wider_row_pitch_is_never_read(harness, tmp_path):
    """ldy > n_dst with NaN and garbage in the pad: the harness copies each row into a block of exactly n_dst values."""
    n_dst, ldy = 77, 96
    values, nbits, dec, _ = pc.batch(n_dst, seed=7)
    wide = np.full((values.shape[0], ldy), np.nan)
    wide[:, n_dst + 1::2] = 1e300
    wide[:, :n_dst] = values
    enc, total, rows, bms, buf = run(harness, tmp_path, wide, nbits, dec, n_dst)
    want = enc.encode(values)
    assert rows.tobytes() == want.rows.tobytes() and bms.tobytes() == want.bitmaps.tobytes()
    assert np.array_equal(buf, want.buf)
