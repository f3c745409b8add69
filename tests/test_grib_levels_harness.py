"""The chunk plan of the GRIB host entries in units (smm::plan_grib_chunks) and the staging layout of its chunks
(smm::layout_grib_chunk) under AddressSanitizer + UBSan, in a stand-alone program (tests/cpp/grib_levels_harness.cpp)
linked with smm_grib_plan.cpp and run as a child process: the plan is recomputed from the rows for the bench shape, a
unit that alone exceeds the bound, and a seeded sweep over random row widths, bitmaps, units, requests and free-memory
clamps; every chunk of every plan is laid out into a buffer of exactly its planned bytes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCES = [os.path.join(ROOT, "tests", "cpp", "grib_levels_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_plan.cpp")]


@pytest.fixture(scope="module")
def counts(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("griblev") / "grib_levels_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe] + SOURCES)
    out = subprocess.run([exe], capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-3000:]
    lines = {ln.split()[0]: [int(v) for v in ln.split()[1:]] for ln in out.stdout.splitlines()}
    counts = dict(zip(("bad", "multi_unit", "single_over_target", "short_last", "no_bitmaps"), lines["PLANBAD"]))
    counts.update(zip(("layout_bad", "layouts_bm", "layouts_plain", "layouts_unit1"), lines["LAYOUTBAD"]))
    return counts


def test_unit_plan_tiles_the_outer_axis_in_whole_units_within_the_bound(counts):
    """Every plan: the chunks tile [0, n_outer) exactly once and in order, each is whole units, staged + rank + Y bytes
    stay within the target unless the chunk is a single unit, chunk_outer is honoured with a short last chunk,
    max_x / max_rows / max_rank are the true maxima, and n_outer == 0 or unit == 0 give no chunks."""
    assert counts["bad"] == 0


def test_the_sweep_reached_every_branch_of_the_plan(counts):
    assert counts["multi_unit"] > 100 and counts["single_over_target"] >= 3
    assert counts["short_last"] > 20 and counts["no_bitmaps"] == 1


def test_the_layout_of_every_chunk_fills_exactly_its_planned_bytes(counts):
    """Every chunk of every plan above, laid out into a buffer of exactly chunk.x_bytes bytes (an overrun is a sanitizer
    error): the cursor ends at x_bytes, every offset is a multiple of 4, no data or bitmap range overlaps another or the
    tables, the bitmapped rows' tables add up to rank_bytes and are numbered in row order -- with and without bitmap
    records, with units of one row and of several."""
    assert counts["layout_bad"] == 0
    assert counts["layouts_bm"] > 500 and counts["layouts_plain"] > 50 and counts["layouts_unit1"] > 20
