"""CF-packed int16 input (`cf=`, smm_apply_host_cf / smm_apply_cf / smm_apply_sb_cf) against the same field decoded on
the host first, on config-2 rows (r1440x721 -> r360x180 bilinear, 512 rows, as bench.py's host_to_host block).

One process, the legs interleaved step by step after a warm-up, medians:
  host   smm_apply_host, wall clock, pageable input:
           i16        the raw int16 field with the decode rule
           f32 / f64  the field decoded to float32 / float64 beforehand (decode excluded)
           f32+dec / f64+dec   the same with the numpy decode (CFDecode.decode) inside the timed region
         plus the pipeline's stage split (smm_debug_host_stats) and the H2D bytes of the i16, f32 and f64 legs
  kernel device time (HIP events) of kernel A (X (B, S)) and kernel C (X (S, B)) at B = 512: int16 against float32
Prints one JSON line per block.

  python tools/packed_bench.py [--rows 512] [--steps 9] [--warmup 2] [--only host,kernel]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def _field(rows, n_src, seed=20261016):
    """ERA5-like int16 rows: full range, -32768 as _FillValue on ~3 % of the cells."""
    rng = np.random.default_rng(seed)
    blk = rng.integers(-32767, 32768, size=(16, n_src)).astype(np.int16)
    blk[rng.random(blk.shape) < 0.03] = -32768
    return np.ascontiguousarray(np.tile(blk, ((rows + 15) // 16, 1))[:rows])


def _median(v):
    return float(np.median(np.asarray(v)))


def bench_host(op, q, cf, steps, warmup):
    from smmregrid_amd import _lib
    x32 = cf.decode(q)
    cf64 = type(cf)(cf.scale_factor, cf.add_offset, cf.fill_values, np.float64)
    x64 = cf64.decode(q)
    out = np.empty((q.shape[0], op.n_dst))
    legs = {
        "i16": lambda: op.apply_host(q, out=out, cf=cf),
        "f32": lambda: op.apply_host(x32, out=out),
        "f64": lambda: op.apply_host(x64, out=out),
        "f32+dec": lambda: op.apply_host(cf.decode(q), out=out),
        "f64+dec": lambda: op.apply_host(cf64.decode(q), out=out),
    }
    times = {k: [] for k in legs}
    stats = {k: [] for k in ("i16", "f32", "f64")}
    for step in range(warmup + steps):
        for name, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            st = _lib.host_stats(reset=True)
            if step >= warmup:
                times[name].append(dt)
                if name in stats:
                    stats[name].append(st)
    res = {"block": "host", "rows": int(q.shape[0]), "steps": steps,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()}}
    for name, sts in stats.items():
        res["stages_" + name] = {k: round(_median([s[k] for s in sts]), 3)
                                 for k in ("stage_in_ms", "h2d_ms", "kernel_ms", "d2h_ms", "copy_out_ms", "wait_ms", "chunks")}
        res["h2d_bytes_" + name] = int(sts[0]["h2d_bytes"])
    res["i16_over_f32"] = round(res["ms"]["i16"] / res["ms"]["f32"], 3)
    res["i16_over_f64"] = round(res["ms"]["i16"] / res["ms"]["f64"], 3)
    return res


def bench_kernels(op, q, cf, steps, warmup):
    from smmregrid_amd import to_device
    from smmregrid_amd.device import DeviceArray, Event
    x32 = cf.decode(q)
    B = q.shape[0]
    dq, dx = to_device(q), to_device(x32)
    dqt = to_device(np.ascontiguousarray(q.T), layout="sb")
    dxt = to_device(np.ascontiguousarray(x32.T), layout="sb")
    y = DeviceArray((B, op.n_dst), np.float64)
    from smmregrid_amd import _lib
    legs = {
        "A_i16": lambda: op.apply(dq, y=y, cf=cf),
        "A_f32": lambda: op.apply(dx, y=y, flags=_lib.APPLY_KERNEL_SELL),
        "tile_f32": lambda: op.apply(dx, y=y),
        "C_i16": lambda: op.apply_sb(dqt, y=y, cf=cf),
        "C_f32": lambda: op.apply_sb(dxt, y=y),
    }
    e0, e1 = Event(), Event()
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        for name, fn in legs.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if step >= warmup:
                times[name].append(e0.elapsed_ms(e1))
    res = {"block": "kernel", "rows": int(B), "steps": steps, "ms": {k: round(_median(v), 4) for k, v in times.items()},
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}}
    res["A_i16_over_f32"] = round(res["ms"]["A_i16"] / res["ms"]["A_f32"], 3)
    res["C_i16_over_f32"] = round(res["ms"]["C_i16"] / res["ms"]["C_f32"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="host,kernel")
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("medians need at least 7 steps")
    from smmregrid_amd import CFDecode, SparseOperator, gridgen
    w = gridgen.bilinear_weights("r1440x721", "r360x180")
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    cf = CFDecode(1.9e-3, 2.7e2, (-32768,), np.float32)
    q = _field(args.rows, op.n_src)
    for block in args.only.split(","):
        fn = {"host": bench_host, "kernel": bench_kernels}[block.strip()]
        print(json.dumps(fn(op, q, cf, args.steps, args.warmup)), flush=True)


if __name__ == "__main__":
    main()
