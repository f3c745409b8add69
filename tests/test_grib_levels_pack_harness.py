"""The chunk plan of smm_group_apply_host_grib_pk in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/grib_levels_pack_harness.cpp): `plan_grib_chunks` with units of n_lev * n_inner records and the per-record
bytes of a packed result -- whole outer indices that tile the call, chunk_outer honoured, a tight budget giving
single-outer chunks, every larger chunk inside the budget, and each chunk's slot offsets equal to `smm_grib_out_layout`
of its own rows.  No device is touched."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "grib_levels_pack_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_plan.cpp")]


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib_levels_pack") / "grib_levels_pack_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + SOURCES)
    return exe


def test_group_pack_plans_hold_under_the_sanitizers(harness):
    out = subprocess.run([harness], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0 and out.stdout.strip() == "OK", (out.stdout + out.stderr)[-3000:]
