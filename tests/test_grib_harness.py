"""The GRIB code that needs no device under AddressSanitizer + UBSan, in a stand-alone program (tests/cpp/grib_harness.cpp):
`grib_extract` / `grib_decode` -- the functions the kernel of smm_apply_grib runs, compiled here with plain g++ -- against a
bit-by-bit loop and the decode statement in C doubles, the row-table refusals, and the chunk plan of smm_apply_host_grib."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "grib_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_plan.cpp")]


@pytest.fixture(scope="module")
def lines(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib") / "grib_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + SOURCES)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-3000:]
    return {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines()}


def test_extract_matches_a_bit_by_bit_loop_and_never_reads_past_the_buffer(lines):
    """Every nbits 0..32 x byte offset 0..3, the last value ending on the last byte of a heap block of exactly
    align4(x_bytes) bytes: an over-read would have been an AddressSanitizer report (non-zero exit)."""
    bad, checked = lines["EXTRACTBAD"]
    assert bad == 0 and checked >= 32 * 4 * (1 + 2 + 3 + 5 + 8 + 31 + 64 + 97)      # widths 1..32, at least the counts asked for


def test_decode_matches_the_statement_in_c_doubles(lines):
    bad, checked, subnormals, infs, ties = lines["DECODEBAD"]
    assert bad == 0 and checked == 16 * 8 * 6 * 3
    assert subnormals > 0 and infs > 0 and ties > 0          # the adversarial set reaches what it is there for


def test_row_table_refusals(lines):
    assert lines["CHECKBAD"] == [0]


def test_chunk_plan(lines):
    """Chunks are consecutive, cover all rows and stay under the byte bound; a row larger than the target gets a chunk
    of one; chunk_rows overrides the plan; mixed widths with 0-bit rows."""
    bad, multi_row_plans, single_over_target = lines["PLANBAD"]
    assert bad == 0 and multi_row_plans > 50 and single_over_target == 1
