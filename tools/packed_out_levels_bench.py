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
import time

import numpy as np

import benchlib
from bench_inputs import int16_levels


def bench_host(grp, ml, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib
    n_lev = q.shape[1]
    lev = np.arange(n_lev, dtype=np.int32)
    kw = dict(masked=True, remap_area_min=0.5, cf=cf)
    regrid_ms = []

    def f64_then_encode():
        t0 = time.perf_counter()
        y = grp.apply_host(q, lev, ml, **kw)
        regrid_ms.append((time.perf_counter() - t0) * 1e3)
        return enc.encode(y)

    legs = {
        "i16_i16": lambda: grp.apply_host(q, lev, ml, cf_out=enc, **kw),
        "i16_f64": lambda: grp.apply_host(q, lev, ml, **kw),
        "i16_f64_enc": f64_then_encode,
    }
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats)
    encode_ms = [dt - regrid for dt, regrid in zip(times["i16_f64_enc"], regrid_ms[warmup:])]
    res = {"block": "host", "levels": int(n_lev), "nsteps": int(q.shape[0]), "cells": int(q.size), "steps": steps}
    res.update(benchlib.summary(times, 3, maximum=True))
    res["host_encode_ms"] = round(benchlib.median(encode_ms), 3)
    for name, sts in stats.items():
        res["stages_" + name] = benchlib.stage_split(sts)
        res["h2d_bytes_" + name] = int(sts[0]["h2d_bytes"])
        res["d2h_bytes_" + name] = int(sts[0]["d2h_bytes"])
    ms = res["ms"]
    res["i16_i16_over_i16_f64"] = round(ms["i16_i16"] / ms["i16_f64"], 3)
    res["i16_i16_over_i16_f64_enc"] = round(ms["i16_i16"] / ms["i16_f64_enc"], 3)
    return res


def bench_kernels(grp, ml, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib, to_device
    from smmregrid_amd.device import DeviceArray
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
    res = {"block": "kernel", "levels": int(n_lev), "nsteps": int(B), "steps": steps}
    res.update(benchlib.summary(benchlib.time_events(legs, steps, warmup), 4, maximum=True))
    ms = res["ms"]
    res["C_td64_over_f64"] = round(ms["C_i16_td64"] / ms["C_f64"], 3)
    res["C_td16_over_f64"] = round(ms["C_i16_td16"] / ms["C_f64"], 3)
    res["A_i16_over_f64"] = round(ms["A_i16"] / ms["A_f64"], 3)
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=7, warmup=2, only="host,kernel", cfg_rows=False, steps_help="timed repetitions")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the field")
    return ap


def main():
    args = benchlib.parse(parser(), least=7, why="medians need at least 7 steps")
    from smmregrid_amd import CFDecode, CFEncode
    grp, masks, ml = benchlib.build_group(args.levels)
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    enc = CFEncode(1.0e-3, 20.0, -32768, np.int16)
    q = int16_levels(masks, args.nsteps)
    for block in benchlib.split(args.only):
        if block == "host":
            res = bench_host(grp, ml, q, cf, enc, args.steps, args.warmup)
        else:
            # the kernel block keeps the field on the device twice and four results: at most 32 time steps of it
            res = bench_kernels(grp, ml, q[:32], cf, enc, args.steps, args.warmup)
        benchlib.emit(res)


if __name__ == "__main__":
    main()
