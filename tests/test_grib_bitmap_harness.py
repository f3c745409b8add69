"""The bitmap code of smm_apply_grib_bm that needs no device under AddressSanitizer + UBSan, in a stand-alone program
(tests/cpp/grib_bitmap_harness.cpp): `bitmap_block` / `bitmap_present` / `bitmap_index` -- the functions the table build
and the gather run, compiled here with plain g++ -- against a bit-by-bit loop, the refusals of the bitmap records, and the
chunk plan of smm_apply_host_grib_bm."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "grib_bitmap_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_plan.cpp")]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("gribbm") / "grib_bitmap_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + SOURCES)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-3000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines()}


def test_block_presence_and_index_match_a_bit_by_bit_loop(lines):
    """n_src 1 / 31 / 32 / 33 / 63 / 64 / 65 / 96 / 300 / 777, the bitmap at byte residues 0..3 (with and without a word in
    front of it), random, all-missing, all-present, whole-block and first-and-last patterns; the bitmap's last byte is the
    last byte of the buffer, in a heap block of exactly the rounded size (an over-read is an AddressSanitizer report),
    and every bit that is not one of the bitmap's first n_src -- set to 1, then to 0 -- leaves the table as it is."""
    bad, checked, pad_cases = lines["CODECBAD"]
    assert bad == 0 and checked == (1 + 31 + 32 + 33 + 63 + 64 + 65 + 96 + 300 + 777) * 8 * 5 and pad_cases > 300


def test_bitmap_record_refusals(lines):
    assert lines["CHECKBAD"] == [0]


def test_chunk_plan_counts_bitmap_and_table_bytes(lines):
    """Chunks are consecutive, cover all rows once and stay under the byte bound with their staged bitmaps and their
    device-only tables counted; a fat row gets a chunk of one; chunk_rows overrides the plan."""
    bad, multi_row_plans, single_over_target, rank_counted = lines["PLANBAD"]
    assert bad == 0 and multi_row_plans > 50 and single_over_target == 1 and rank_counted == 1


def test_the_segment_is_whole_threads_of_the_build_kernels(lines):
    assert lines["SEGBLOCKS"][0] % 256 == 0 and lines["SEGBLOCKS"][0] >= 256
