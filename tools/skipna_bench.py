"""Cost of SMM_APPLY_SKIPNA against the plain apply on the same fields.

Every workload is timed on two seeded fields, one without NaN and one with ~3 % NaN, each with the plain and the
skipna apply; the four runs alternate inside one process (warm-up first), device time from HIP events around each
call, median over the steps.  Workloads (bench.py's problem builders, bench.py itself untouched):
  cfg2      r1440x721 -> r360x180 bilinear, B = 3600 f64, X (B, S) native layout
  cfg5tile  r1440x721 -> r720x360 conservative, B = 1024 f64
  cfg3sb    BASELINE config 3 geometry (1442x1021 -> r360x180, 75 masked levels, 64 steps), every level batch-fastest,
            one grouped launch (the extra NaN are fixed in time: the kernels' cost does not depend on where they are)
  host      smm_apply_host on 512 config-2 rows (H2D + kernel + D2H, wall clock)
Prints one JSON line per workload: {"workload", "kernel" (plain / skipna), "plain_ms", "skipna_ms", ...}.
Kernel times for a profile: run under `rocprofv3 --kernel-trace --stats -- python tools/skipna_bench.py`.

  python tools/skipna_bench.py [--steps 10] [--warmup 3] [--only cfg2,cfg5tile,cfg3sb,host]
"""
import argparse
import ctypes

import numpy as np

import benchlib
from bench_inputs import seeded_block

BLOCK = 16   # seeded host rows, replicated over the batch on the device


def _replicate(dev, blk):
    """Fill the (B, S) device array with copies of the host block."""
    from smmregrid_amd import _lib
    n = dev.shape[0]
    first = min(BLOCK, n)
    dev.rows(0, first).copy_from_host(np.ascontiguousarray(blk[:first]))
    done = first
    while done < n:
        k = min(done, n - done)
        _lib.call("smm_memcpy_d2d", ctypes.c_void_p(dev.rows(done, done + k).ptr), ctypes.c_void_p(dev.ptr),
                  k * dev.shape[1] * dev.dtype.itemsize, None)
        done += k


def _time(run, steps, warmup):
    """run: {label: callable}; the labels alternate step by step.  Median device ms per label."""
    return {k: benchlib.median(v) for k, v in benchlib.time_events(run, steps, warmup).items()}


def _emit(workload, nan_frac, ms, nan, digits=4, **more):
    benchlib.emit({"workload": workload, "nan_frac": nan_frac, **more, "plain_ms": round(ms[(nan, False)], digits),
                   "skipna_ms": round(ms[(nan, True)], digits), "ratio": round(ms[(nan, True)] / ms[(nan, False)], 3)})


def bench_2d(name, steps, warmup):
    import bench
    from smmregrid_amd import _lib
    from smmregrid_amd.device import DeviceArray
    p = bench.Problem2D(name, 0, 0)
    y = DeviceArray((p.n_batch, p.n_dst), np.float64)
    fields = {}
    for nan in (False, True):
        x = DeviceArray((p.n_batch, p.n_src), p.np_dt)
        _replicate(x, seeded_block(p.n_src, p.np_dt, nan, rows=BLOCK))
        fields[nan] = x
    run = {}
    for nan, x in fields.items():
        for sk in (False, True):
            run[(nan, sk)] = (lambda x=x, sk=sk: p.op.apply(x, y=y, remap_area_min=0.5, skipna=sk))
    ms = _time(run, steps, warmup)
    li = p.op.launch_info(p.n_batch, p.np_dt)
    lk = p.op.launch_info(p.n_batch, p.np_dt, flags=_lib.APPLY_SKIPNA)
    for nan in (False, True):
        _emit(name, 0.03 if nan else 0.0, ms, nan, kernel=[li["kernel"], lk["kernel"]])


def bench_levels(steps, warmup):
    import bench
    from smmregrid_amd.device import DeviceArray
    p = bench.ProblemLevels("cfg3sb", 0, 0, batch=64)   # 64 of the 120 time steps: two fields of 75 levels fit in HBM
    rng = np.random.default_rng(20261016)
    xs = {False: p.x}
    slab = p.slab.copy()
    slab[rng.random(slab.shape) < 0.03] = np.nan
    x2 = DeviceArray(p.x.shape, np.float64)
    for lv in range(p.n_lev):
        x2.rows(lv, lv + 1).copy_from_host(np.repeat(slab[lv][:, None], p.ldt, axis=1)[None])
    xs[True] = x2
    y = DeviceArray((p.n_t, p.n_lev, p.n_dst), np.float64)
    run = {}
    for nan, x in xs.items():
        for sk in (False, True):
            run[(nan, sk)] = (lambda x=x, sk=sk: p.group.apply_sb(
                x, p.level_index, p.masked_levels, y=y, masked=True, remap_area_min=0.5, n_batch=p.n_t, skipna=sk))
    ms = _time(run, steps, warmup)
    for nan in (False, True):
        _emit("cfg3sb", "land + 0.03" if nan else "land", ms, nan, kernel="sb-group")


def bench_host(steps, warmup, rows=512):
    import bench
    from smmregrid_amd import pinned_empty
    p = bench.Problem2D("cfg2", 0, 0, batch=16)
    out = pinned_empty((rows, p.n_dst), np.float64)
    for nan in (False, True):
        x = np.tile(seeded_block(p.n_src, np.float64, nan, rows=BLOCK), (rows // BLOCK, 1))
        legs = {(nan, sk): (lambda sk=sk: p.op.apply_host(x, out=out, remap_area_min=0.5, skipna=sk)) for sk in (False, True)}
        ms = {k: benchlib.median(v) for k, v in benchlib.time_wall(legs, steps, warmup).items()}
        _emit(f"host cfg2 x {rows} rows", 0.03 if nan else 0.0, ms, nan, digits=3)


def parser():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--only", default="cfg2,cfg5tile,cfg3sb,host")
    return ap


def main():
    a = parser().parse_args()
    names = a.only.split(",")
    for n in ("cfg2", "cfg5tile"):
        if n in names:
            bench_2d(n, a.steps, a.warmup)
    if "cfg3sb" in names:
        bench_levels(a.steps, a.warmup)
    if "host" in names:
        bench_host(a.steps, a.warmup)


if __name__ == "__main__":
    main()
