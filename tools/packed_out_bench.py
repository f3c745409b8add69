"""CF-packed int16 RESULTS (`cf_out=`, smm_apply_host_pk / smm_apply_pk / smm_apply_sb_pk) against the float64 result
of the same call, on config-2 rows (r1440x721 -> r360x180 bilinear) and on one conservative operator (config-5 geometry,
r1440x721 -> r720x360), B = 512.

One process, the legs interleaved step by step after a warm-up, medians:
  host    smm_apply_host host to host, wall clock, pageable input and output, int16 input:
            i16->i16      packed result (2 B per cell back)
            i16->f64      today's path (8 B per cell back)
            i16->f64+enc  today's path plus the numpy encode (CFEncode.encode) inside the timed region
          plus the pipeline's stage split (smm_debug_host_stats) and the D2H bytes of the first two legs
  kernel  device time (HIP events) of kernel A (X (B, S)) and kernel C (X (S, B)): int16 Y against float64 Y, for
          float64 X and int16 X; kernel C's packed result at 64 and at 16 destination rows per tile
          (SMM_TUNE_SB_PACKED_Y_ROWS), also kept batch-fastest (SB_Y_SB)
Prints one JSON line per block and operator.

  python tools/packed_out_bench.py [--rows 512] [--steps 9] [--warmup 2] [--only host,kernel] [--ops cfg2,cfg5]
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


def bench_host(name, op, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib
    out16 = np.empty((q.shape[0], op.n_dst), np.int16)
    out64 = np.empty((q.shape[0], op.n_dst))
    legs = {
        "i16->i16": lambda: op.apply_host(q, out=out16, cf=cf, cf_out=enc),
        "i16->f64": lambda: op.apply_host(q, out=out64, cf=cf),
        "i16->f64+enc": lambda: enc.encode(op.apply_host(q, out=out64, cf=cf)),
    }
    times = {k: [] for k in legs}
    stats = {k: [] for k in ("i16->i16", "i16->f64")}
    for step in range(warmup + steps):
        for leg, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            st = _lib.host_stats(reset=True)
            if step >= warmup:
                times[leg].append(dt)
                if leg in stats:
                    stats[leg].append(st)
    res = {"block": "host", "op": name, "rows": int(q.shape[0]), "steps": steps,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()}}
    for leg, sts in stats.items():
        res["stages_" + leg] = {k: round(_median([s[k] for s in sts]), 3)
                                for k in ("stage_in_ms", "h2d_ms", "kernel_ms", "d2h_ms", "copy_out_ms", "wait_ms", "chunks")}
        res["d2h_bytes_" + leg] = int(sts[0]["d2h_bytes"])
        res["h2d_bytes_" + leg] = int(sts[0]["h2d_bytes"])
    res["i16_over_f64"] = round(res["ms"]["i16->i16"] / res["ms"]["i16->f64"], 3)
    res["i16_over_f64_enc"] = round(res["ms"]["i16->i16"] / res["ms"]["i16->f64+enc"], 3)
    return res


def bench_kernels(name, op, q, cf, enc, steps, warmup):
    from smmregrid_amd import CFDecode, _lib, to_device
    from smmregrid_amd.device import DeviceArray, Event
    x64 = CFDecode(cf.scale_factor, cf.add_offset, cf.fill_values, np.float64).decode(q)
    B, D = q.shape[0], op.n_dst
    dq, dx = to_device(q), to_device(x64)
    dqt = to_device(np.ascontiguousarray(q.T), layout="sb")
    dxt = to_device(np.ascontiguousarray(x64.T), layout="sb")
    y64, y16 = DeviceArray((B, D), np.float64), DeviceArray((B, D), np.int16)
    t64, t16 = DeviceArray((D, B), np.float64, layout="sb"), DeviceArray((D, B), np.int16, layout="sb")
    sell = _lib.APPLY_KERNEL_SELL

    def rows16(fn):
        def run():
            with _lib.tuning(sb_packed_y_rows=16):
                fn()
        return run

    legs = {
        "A_f64->f64": lambda: op.apply(dx, y=y64, flags=sell),
        "A_f64->i16": lambda: op.apply(dx, y=y16, cf_out=enc),
        "A_i16->f64": lambda: op.apply(dq, y=y64, cf=cf),
        "A_i16->i16": lambda: op.apply(dq, y=y16, cf=cf, cf_out=enc),
        "C_f64->f64": lambda: op.apply_sb(dxt, y=y64),
        "C_f64->i16": lambda: op.apply_sb(dxt, y=y16, cf_out=enc),
        "C_f64->i16_td16": rows16(lambda: op.apply_sb(dxt, y=y16, cf_out=enc)),
        "C_i16->f64": lambda: op.apply_sb(dqt, y=y64, cf=cf),
        "C_i16->i16": lambda: op.apply_sb(dqt, y=y16, cf=cf, cf_out=enc),
        "C_i16->i16_td16": rows16(lambda: op.apply_sb(dqt, y=y16, cf=cf, cf_out=enc)),
        "Csb_i16->f64": lambda: op.apply_sb(dqt, y=t64, cf=cf, keep_batch_fastest=True),
        "Csb_i16->i16": lambda: op.apply_sb(dqt, y=t16, cf=cf, cf_out=enc, keep_batch_fastest=True),
        "Csb_i16->i16_td16": rows16(lambda: op.apply_sb(dqt, y=t16, cf=cf, cf_out=enc, keep_batch_fastest=True)),
    }
    e0, e1 = Event(), Event()
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        for leg, fn in legs.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if step >= warmup:
                times[leg].append(e0.elapsed_ms(e1))
    res = {"block": "kernel", "op": name, "rows": int(B), "steps": steps,
           "ms": {k: round(_median(v), 4) for k, v in times.items()},
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}}
    ms = res["ms"]
    res["packed_over_f64"] = {k: round(ms[k] / ms[k.replace("->i16", "->f64").replace("_td16", "")], 3)
                              for k in ms if "->i16" in k}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="host,kernel")
    ap.add_argument("--ops", default="cfg2,cfg5")
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("medians need at least 7 steps")
    from smmregrid_amd import CFDecode, CFEncode, SparseOperator, gridgen
    cf = CFDecode(1.9e-3, 2.7e2, (-32768,), np.float32)
    enc = CFEncode(1.9e-3, 2.7e2, -32768, np.int16)
    for name in args.ops.split(","):
        name = name.strip()
        if name == "cfg2":
            w = gridgen.bilinear_weights("r1440x721", "r360x180")
        elif name == "cfg5":
            w = gridgen.conservative_weights("r1440x721", "r720x360")
        else:
            ap.error(f"unknown operator {name}")
        op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                            w["dst_address"].values, w["remap_matrix"].values, device=0)
        q = _field(args.rows, op.n_src)
        for block in args.only.split(","):
            fn = {"host": bench_host, "kernel": bench_kernels}[block.strip()]
            print(json.dumps(fn(name, op, q, cf, enc, args.steps, args.warmup)), flush=True)
        op.close()


if __name__ == "__main__":
    main()
