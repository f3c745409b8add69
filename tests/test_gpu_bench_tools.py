"""Every tools/*_bench.py tool, one tiny in-process call per block, against the result the same call gave before the
tools moved onto tools/benchlib.py and tools/bench_inputs.py (tests/golden/bench_tools_parent.json): the same key tree,
the same value under every key that is neither a time nor a ratio of times -- bytes, byte ratios, row counts, widths,
chunk counts, the bits_equal flags -- and a finite positive number under every key that is one.  The tools' own
bit-for-bit comparisons run inside these calls; a SystemExit fails the case.

The operator is r70x36 -> r36x18 bilinear (S = 2520: even, 2520 % 32 = 24; D = 648) with 6 rows (more than the 4
distinct ones, no multiple of them), 5 timed steps after 1 warm-up step; the group tools run 2 levels x 2 steps on their
own grids.  `grib_bench`'s file block reads r1440x721 messages and so takes the config-2 operator, with 2 messages.
`skipna_bench` takes its problems from bench.py; here they are stand-ins on the tiny operator and the 2-level group.
"""
import argparse
import contextlib
import importlib
import io
import json
import math
import os
import sys
import types

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "bench_tools_parent.json")
ROWS, STEPS, WARMUP, LEVELS, NSTEPS = 6, 5, 1, 2, 2
TIMING = (STEPS, WARMUP)


def tool(name):
    """a module of tools/, imported the way the tools import each other: by its bare name, tools/ on sys.path"""
    tools = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools")
    if tools not in sys.path:
        sys.path.insert(0, tools)
    return importlib.import_module(name)


class World:
    """what the cases share, built once: the tiny operator, the 2-level group, the config-2 operator"""

    def __init__(self, conservative=None):
        """conservative: another way to the conservative operator (the recording of the golden file built it as the
        tools then did, from gridgen.conservative_weights)"""
        self._made = {}
        self._conservative = conservative or (lambda: tool("benchlib").build_operator(("r70x36", "r36x18", "con")))

    def _once(self, key, make):
        if key not in self._made:
            self._made[key] = make()
        return self._made[key]

    @property
    def op(self):
        return self._once("op", lambda: tool("benchlib").build_operator(("r70x36", "r36x18", "bil")))

    @property
    def op_frac(self):
        """the tiny operator with its epilogue set, as bench.py's problems have theirs"""
        def make():
            from smmregrid_amd import SparseOperator, gridgen
            w = gridgen.generate_weights("r70x36", "r36x18", method="bil")
            op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                                w["dst_address"].values, w["remap_matrix"].values, device=0)
            op.set_epilogue(w["dst_grid_imask"].values, w["dst_grid_frac"].values)
            return op
        return self._once("op_frac", make)

    @property
    def op_con(self):
        return self._once("op_con", self._conservative)

    @property
    def cfg2(self):
        return self._once("cfg2", lambda: tool("benchlib").build_operator("cfg2"))

    @property
    def group(self):
        return self._once("group", lambda: tool("benchlib").build_group(LEVELS))

    def q(self):
        return tool("bench_inputs").int16_rows(ROWS, self.op.n_src)

    def q_levels(self):
        return tool("bench_inputs").int16_levels(self.group[1], NSTEPS)


def _cf(scale, offset):
    from smmregrid_amd import CFDecode, CFEncode
    return CFDecode(scale, offset, (-32768,), np.float32), CFEncode(scale, offset, -32768, np.int16)


def _skipna_args():
    return argparse.Namespace(widths=[16], plain_only=False, steps=STEPS, warmup=WARMUP, tag="branch", nsteps=NSTEPS)


def _printed(fn):
    """the JSON lines a call prints"""
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        fn()
    return [json.loads(line) for line in out.getvalue().splitlines() if line.startswith("{")]


def _skipna_problem(w, batch):
    op = w.op_frac
    return types.SimpleNamespace(op=op, n_batch=batch, n_src=op.n_src, n_dst=op.n_dst, np_dt=np.dtype(np.float64))


def _skipna_2d(name):
    def run(m, w):
        import bench
        real = bench.Problem2D
        bench.Problem2D = lambda name, *a, **k: _skipna_problem(w, 24)
        try:
            return _printed(lambda: m.bench_2d(name, *TIMING))
        finally:
            bench.Problem2D = real
    return run


def _skipna_levels_problem(w, n_t=16):
    """what skipna_bench reads of bench.ProblemLevels, on the 2-level group: X (L, S, T) batch-fastest, NaN on land"""
    from smmregrid_amd.device import DeviceArray
    grp, masks, ml = w.group
    n_lev, S = masks.shape
    slab = 10.0 + 5.0 * np.random.default_rng(20260723).standard_normal((n_lev, S))
    slab[masks == 0] = np.nan
    x = DeviceArray((n_lev, S, n_t), np.float64)
    for lv in range(n_lev):
        x.rows(lv, lv + 1).copy_from_host(np.repeat(slab[lv][:, None], n_t, axis=1)[None])
    return types.SimpleNamespace(x=x, slab=slab, n_lev=n_lev, ldt=n_t, n_t=n_t, n_dst=grp.n_dst, group=grp,
                                 level_index=np.arange(n_lev, dtype=np.int32), masked_levels=ml)


def _skipna_levels(m, w):
    import bench
    real = bench.ProblemLevels
    bench.ProblemLevels = lambda name, *a, **k: _skipna_levels_problem(w)
    try:
        return _printed(lambda: m.bench_levels(*TIMING))
    finally:
        bench.ProblemLevels = real


def _skipna_host(m, w):
    import bench
    real = bench.Problem2D
    bench.Problem2D = lambda name, *a, **k: _skipna_problem(w, 16)
    try:
        return _printed(lambda: m.bench_host(*TIMING, rows=16))
    finally:
        bench.Problem2D = real


def _group_call(fn):
    return lambda m, w: fn(m, *w.group)


CASES = {
    "grib_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, *TIMING),
    "grib_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, *TIMING),
    "grib_bench:open": lambda m, w: m.bench_open(w.cfg2, "cfg2", 2, *TIMING),
    "grib_bitmap_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, *TIMING),
    "grib_bitmap_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, *TIMING),
    "grib_ccsds_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, *TIMING),
    "grib_ccsds_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, *TIMING),
    "grib_complex_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, *TIMING),
    "grib_complex_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, *TIMING),
    "grib_complex_bench:profile_run": lambda m, w: m.profile_run(w.op, ROWS),
    "grib_ccsds_out_bench:kernel16": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, 16, *TIMING),
    "grib_ccsds_out_bench:kernel12": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, 12, *TIMING),
    "grib_ccsds_out_bench:host16": lambda m, w: m.bench_host(w.op, "tiny", ROWS, 16, *TIMING),
    "grib_ccsds_out_bench:host12": lambda m, w: m.bench_host(w.op, "tiny", ROWS, 12, *TIMING),
    "grib_complex_out_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, 16, *TIMING),
    "grib_complex_out_bench:sizes": lambda m, w: m.bench_sizes(w.op, "tiny", ROWS, 16),
    "grib_complex_out_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, 16, *TIMING),
    "grib_complex_mv_bench:kernel+host": lambda m, w: m.bench(w.op, "tiny", ROWS, *TIMING, ["kernel", "host"]),
    "grib_complex_mv_bench:parent": lambda m, w: m.bench_parent("tiny", w.op.n_src, ROWS, *TIMING,
                                                                  importlib.import_module("smmregrid_amd._lib").LIB_PATH),
    "grib_levels_bench:host": _group_call(lambda m, grp, masks, ml: m.bench(grp, masks, ml, NSTEPS, *TIMING)),
    "grib_out_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, *TIMING),
    "grib_out_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, *TIMING),
    "grib_out_levels_bench:host": _group_call(lambda m, grp, masks, ml: m.bench(grp, masks, ml, NSTEPS, *TIMING)),
    "grib_skipna_bench:kernel": lambda m, w: m.bench_kernel(w.op, "tiny", ROWS, _skipna_args()),
    "grib_skipna_bench:host": lambda m, w: m.bench_host(w.op, "tiny", ROWS, _skipna_args()),
    "grib_skipna_bench:levels_kernel": _group_call(lambda m, grp, masks, ml: m.bench_levels(grp, masks, ml, "kernel", _skipna_args())),
    "grib_skipna_bench:levels_host": _group_call(lambda m, grp, masks, ml: m.bench_levels(grp, masks, ml, "host", _skipna_args())),
    "half_bench:kernel": lambda m, w: m.bench_kernel(w.op, ROWS, *TIMING),
    "half_bench:host": lambda m, w: m.bench_host(w.op, ROWS, *TIMING),
    "half_bench:group": lambda m, w: m.bench_group(LEVELS, NSTEPS, *TIMING),
    "host_pipeline_bench_levels:run": lambda m, w: m.run(NSTEPS, n_lev=LEVELS),
    "packed_bench:host": lambda m, w: m.bench_host(w.op, w.q(), _cf(1.9e-3, 2.7e2)[0], *TIMING),
    "packed_bench:kernel": lambda m, w: m.bench_kernels(w.op, w.q(), _cf(1.9e-3, 2.7e2)[0], *TIMING),
    "packed_levels_bench:host": lambda m, w: m.bench_host(w.group[0], w.group[2], w.q_levels(), _cf(1.0e-3, 20.0)[0], *TIMING,
                                                          ["i16", "f32", "f32b", "f64", "dec32", "dec64"]),
    "packed_levels_bench:kernel": lambda m, w: m.bench_kernels(w.group[0], w.group[2], w.q_levels(), _cf(1.0e-3, 20.0)[0], *TIMING),
    "packed_out_bench:host": lambda m, w: m.bench_host("tiny", w.op, w.q(), *_cf(1.9e-3, 2.7e2), *TIMING),
    "packed_out_bench:kernel": lambda m, w: m.bench_kernels("tiny", w.op, w.q(), *_cf(1.9e-3, 2.7e2), *TIMING),
    "packed_out_bench:host_conservative": lambda m, w: m.bench_host("tiny_con", w.op_con, w.q(), *_cf(1.9e-3, 2.7e2), *TIMING),
    "packed_out_bench:kernel_conservative": lambda m, w: m.bench_kernels("tiny_con", w.op_con, w.q(), *_cf(1.9e-3, 2.7e2), *TIMING),
    "packed_out_levels_bench:host": lambda m, w: m.bench_host(w.group[0], w.group[2], w.q_levels(), *_cf(1.0e-3, 20.0), *TIMING),
    "packed_out_levels_bench:kernel": lambda m, w: m.bench_kernels(w.group[0], w.group[2], w.q_levels(), *_cf(1.0e-3, 20.0), *TIMING),
    "skipna_bench:cfg2": _skipna_2d("cfg2"),
    "skipna_bench:cfg5tile": _skipna_2d("cfg5tile"),
    "skipna_bench:cfg3sb": _skipna_levels,
    "skipna_bench:host": _skipna_host,
    "user_path_bench:reference_sized": lambda m, w: m.reference_sized(reps=5, only=("ua_ipsl_nan",)),
}


def flatten(res, path=""):
    """{path: leaf} of a result: dicts and lists of dicts walked, anything else a leaf"""
    if isinstance(res, dict):
        return {k: v for key, sub in res.items() for k, v in flatten(sub, f"{path}/{key}").items()}
    if isinstance(res, list) and res and all(isinstance(v, dict) for v in res):
        return {k: v for i, sub in enumerate(res) for k, v in flatten(sub, f"{path}/{i}").items()}
    return {path: res}


def run_case(case, world):
    try:
        return CASES[case](tool(case.split(":")[0]), world)
    except SystemExit as exc:      # a tool's own bit-for-bit comparison, or a refused input
        raise AssertionError(f"{case} stopped: {exc}") from exc


@pytest.fixture(scope="module")
def world(hip):
    return World()


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as f:
        return json.load(f)["results"]


def test_the_golden_file_covers_every_case(golden):
    assert sorted(golden) == sorted(CASES)


@pytest.mark.parametrize("case", sorted(CASES))
def test_tool_gives_the_shape_and_the_values_it_gave_before(world, golden, case):
    want = golden[case]
    got = flatten(json.loads(json.dumps(run_case(case, world))))
    assert sorted(got) == sorted(k for name in ("values", "times", "nonneg_times", "difference_times") for k in want[name])
    for key, value in want["values"].items():
        assert got[key] == value, key
    for name in ("times", "nonneg_times", "difference_times"):
        for key in want[name]:
            assert isinstance(got[key], (int, float)) and math.isfinite(got[key]), (key, got[key])
    # a time or a ratio of times is greater than 0 ...
    assert {k: got[k] for k in want["times"] if not got[k] > 0} == {}
    # ... except where 0 is an honest answer at this size: a stage of the pipeline that had nothing to do
    # (stages*/...), a figure the tool rounds to one decimal of a millisecond (parent_road*_ms, decoded_road_ms,
    # decode*_ms, weights_ms), the spread of two medians that coincide (spread) ...
    assert {k: got[k] for k in want["nonneg_times"] if not got[k] >= 0} == {}
    # ... and the differences of two medians -- a bitmapped gather as total - table build (*_gather_ms) and its ratios
    # (*_gather_over_*) -- whose sign is not fixed where the gather is next to nothing: any finite number.
