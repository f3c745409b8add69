"""The pure host pieces the four GRIB transcoders share (smmregrid_amd/csrc/smm_grib_xcode.hpp): the arena of a call's
scratch allocation and the cutting of a launch at the grid limit, in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/grib_xcode_harness.cpp).  No GPU involved."""
import os
import re
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_arena_and_grid_cutter(tmp_path):
    """Offsets aligned for every type, members in order without overlap, the total, an empty member; the pieces of a
    cut launch cover [0, total) exactly once for total = 0, = limit, = limit + 1, limit = 1 and total above 2^32."""
    exe = str(tmp_path / "grib_xcode_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_xcode_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert re.fullmatch(r"ok \d+\n", out.stdout), out.stdout
