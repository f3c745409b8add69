"""CF-packed int16 RESULTS on masked-level (3-D) weights (smm_group_apply_host_pk / smm_group_apply_sb_pk /
smm_group_apply_pk) against the float64 results of the _cf entries, on the group of tools/packed_levels_bench.py:
conservative r1440x721 -> r360x180 weights on synthetic ocean masks (native generator), an int16 field with _FillValue
where the level's mask is 0, 16 levels x 32 time steps.

One process, the legs interleaved step by step after a warm-up, medians of >= 7.  The yardstick of every comparison is
the float64-Y leg of the same process (the _cf entries: code this feature does not touch).
  host   smm_group_apply_host*, wall clock, pageable input (n_steps, n_lev, 1, S):
           i16_i16      the raw int16 field with the decode AND the encode rule: int16 back (cf + enc)
           i16_f64      the raw int16 field, float64 back (_cf)
           i16_f64_enc  i16_f64 followed by CFEncode.encode on the host: what packed_out does on 3-D weights without
                        packed_out_levels
         plus the pipeline's stage split and H2D / D2H bytes (smm_debug_host_stats) per leg
  kernel device time (HIP events), int16 X throughout:
           C_i16_td64 / C_i16_td16  the grouped batch-fastest kernel storing int16, tiles of 64 / 16 destination rows
           C_f64                    its float64-Y twin on the same field
           A_i16 / A_f64            the native layout (SELL kernel), int16 against float64 Y
Prints one JSON line per block, with min and max of the samples beside the medians.

  python tools/packed_out_levels_bench.py [--levels 16] [--nsteps 32] [--steps 7] [--warmup 2] [--only host,kernel]
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

from tools.packed_levels_bench import STAGES, _median, build_group, field      # noqa: E402  (the same group and field)


def _summary(times, digits):
    return {"ms": {k: round(_median(v), digits) for k, v in times.items()},
            "ms_min": {k: round(min(v), digits) for k, v in times.items()},
            "ms_max": {k: round(max(v), digits) for k, v in times.items()}}


def bench_host(grp, ml, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib
    n_lev = q.shape[1]
    lev = np.arange(n_lev, dtype=np.int32)
    kw = dict(masked=True, remap_area_min=0.5, cf=cf)
    last = {}

    def f64_then_encode():
        t0 = time.perf_counter()
        y = grp.apply_host(q, lev, ml, **kw)
        last["regrid_ms"] = (time.perf_counter() - t0) * 1e3
        return enc.encode(y)

    legs = {
        "i16_i16": lambda: grp.apply_host(q, lev, ml, cf_out=enc, **kw),
        "i16_f64": lambda: grp.apply_host(q, lev, ml, **kw),
        "i16_f64_enc": f64_then_encode,
    }
    times = {k: [] for k in legs}
    stats = {k: [] for k in legs}
    encode_ms = []
    for step in range(warmup + steps):
        for name, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            st = _lib.host_stats(reset=True)
            if step >= warmup:
                times[name].append(dt)
                stats[name].append(st)
                if name == "i16_f64_enc":
                    encode_ms.append(dt - last["regrid_ms"])
    res = {"block": "host", "levels": int(n_lev), "nsteps": int(q.shape[0]), "cells": int(q.size), "steps": steps}
    res.update(_summary(times, 3))
    res["host_encode_ms"] = round(_median(encode_ms), 3)
    for name, sts in stats.items():
        res["stages_" + name] = {k: round(_median([s[k] for s in sts]), 3) for k in STAGES}
        res["h2d_bytes_" + name] = int(sts[0]["h2d_bytes"])
        res["d2h_bytes_" + name] = int(sts[0]["d2h_bytes"])
    ms = res["ms"]
    res["i16_i16_over_i16_f64"] = round(ms["i16_i16"] / ms["i16_f64"], 3)
    res["i16_i16_over_i16_f64_enc"] = round(ms["i16_i16"] / ms["i16_f64_enc"], 3)
    return res


def bench_kernels(grp, ml, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib, to_device
    from smmregrid_amd.device import DeviceArray, Event
    B, n_lev, _, S = q.shape
    lev = np.arange(n_lev, dtype=np.int32)
    dq = to_device(q)
    dqs = to_device(np.ascontiguousarray(q.reshape(B, n_lev, S).transpose(1, 2, 0)), layout="sb")
    y = DeviceArray((B, 1, n_lev, grp.n_dst), np.float64)
    ys = DeviceArray((B, n_lev, grp.n_dst), np.float64)
    yq = DeviceArray((B, 1, n_lev, grp.n_dst), np.int16)
    ysq = DeviceArray((B, n_lev, grp.n_dst), np.int16)
    kw = dict(masked=True, remap_area_min=0.5, cf=cf)

    def c_i16(rows):
        def run():
            with _lib.tuning(sb_packed_y_rows=rows):
                grp.apply_sb(dqs, lev, ml, y=ysq, cf_out=enc, **kw)
        return run

    legs = {
        "C_i16_td64": c_i16(0),
        "C_i16_td16": c_i16(16),
        "C_f64": lambda: grp.apply_sb(dqs, lev, ml, y=ys, **kw),
        "A_i16": lambda: grp.apply(dq, lev, ml, y=yq, cf_out=enc, **kw),
        "A_f64": lambda: grp.apply(dq, lev, ml, y=y, **kw),
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
    res = {"block": "kernel", "levels": int(n_lev), "nsteps": int(B), "steps": steps}
    res.update(_summary(times, 4))
    ms = res["ms"]
    res["C_td64_over_f64"] = round(ms["C_i16_td64"] / ms["C_f64"], 3)
    res["C_td16_over_f64"] = round(ms["C_i16_td16"] / ms["C_f64"], 3)
    res["A_i16_over_f64"] = round(ms["A_i16"] / ms["A_f64"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the field")
    ap.add_argument("--steps", type=int, default=7, help="timed repetitions")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="host,kernel")
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("medians need at least 7 steps")
    from smmregrid_amd import CFDecode, CFEncode
    grp, masks, ml = build_group(args.levels)
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    enc = CFEncode(1.0e-3, 20.0, -32768, np.int16)
    q = field(masks, args.nsteps)
    for block in args.only.split(","):
        if block.strip() == "host":
            res = bench_host(grp, ml, q, cf, enc, args.steps, args.warmup)
        else:
            # the kernel block keeps the field on the device twice and four results: at most 32 time steps of it
            res = bench_kernels(grp, ml, q[:32], cf, enc, args.steps, args.warmup)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
