"""CF-packed int16 input on masked-level (3-D) weights (smm_group_apply_host_cf / smm_group_apply_sb_cf /
smm_group_apply_cf) against the same field decoded on the host first, on a config-3-shaped group: conservative
r1440x721 -> r360x180 weights on synthetic ocean masks (native generator), an int16 field with _FillValue where the
level's mask is 0.

One process, the legs interleaved step by step after a warm-up, medians of >= 7:
  host   smm_group_apply_host*, wall clock, pageable input (n_steps, n_lev, 1, S):
           i16        the raw int16 field with the decode rule
           f32 / f64  the field decoded to float32 / float64 beforehand (decode outside the timed region): what a
                      Regridder without packed_levels runs after its host decode.  f32 runs twice per step (f32,
                      f32b): the difference of the two is the run-to-run spread the i16 leg is judged against
           dec32 / dec64  the numpy decode alone (CFDecode.decode), for scale
         plus the pipeline's stage split and H2D bytes (smm_debug_host_stats) per leg
  kernel device time (HIP events): the grouped batch-fastest kernel (X (n_lev, S, B)) and the native layout
         (X (B, n_lev, 1, S), SELL kernel; tile_f32 = what the group's plan picks for float fields), int16 against float32
Prints one JSON line per block.  --legs picks the host legs (f32,f64 run on a library without the _cf entries too).

  python tools/packed_levels_bench.py [--levels 16] [--nsteps 32] [--full] [--steps 7] [--warmup 2]
                                      [--only host,kernel] [--legs i16,f32,f32b,f64,dec32,dec64]
"""
import numpy as np

import benchlib
from bench_inputs import int16_levels


def bench_host(grp, ml, q, cf, steps, warmup, want):
    from smmregrid_amd import _lib
    n_lev = q.shape[1]
    lev = np.arange(n_lev, dtype=np.int32)
    cf64 = type(cf)(cf.scale_factor, cf.add_offset, cf.fill_values, np.float64)
    x32 = cf.decode(q) if {"f32", "f32b"} & set(want) else None
    x64 = cf64.decode(q) if "f64" in want else None
    kw = dict(masked=True, remap_area_min=0.5)
    legs = {
        "i16": lambda: grp.apply_host(q, lev, ml, cf=cf, **kw),
        "f32": lambda: grp.apply_host(x32, lev, ml, **kw),
        "f64": lambda: grp.apply_host(x64, lev, ml, **kw),
        "f32b": lambda: grp.apply_host(x32, lev, ml, **kw),
        "dec32": lambda: cf.decode(q),
        "dec64": lambda: cf64.decode(q),
    }
    legs = {k: v for k, v in legs.items() if k in want}
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats)
    res = {"block": "host", "levels": int(n_lev), "nsteps": int(q.shape[0]), "cells": int(q.size), "steps": steps,
           **benchlib.summary(times, 3, maximum=True)}
    for name in (k for k in legs if not k.startswith("dec")):
        res["stages_" + name] = benchlib.stage_split(stats[name])
        res["h2d_bytes_" + name] = int(stats[name][0]["h2d_bytes"])
    ms = res["ms"]
    if "i16" in ms and "f32" in ms:
        res["i16_over_f32"] = round(ms["i16"] / ms["f32"], 3)
    if "i16" in ms and "f64" in ms:
        res["i16_over_f64"] = round(ms["i16"] / ms["f64"], 3)
    if "f32" in ms and "f32b" in ms:
        # run-to-run spread of the float32 leg: its two medians against each other, and the range of all its samples
        both = times["f32"] + times["f32b"]
        res["f32_spread"] = {"median_ratio": round(ms["f32b"] / ms["f32"], 3),
                             "range_over_median": round((max(both) - min(both)) / benchlib.median(both), 3)}
    return res


def bench_kernels(grp, ml, q, cf, steps, warmup):
    from smmregrid_amd import _lib, to_device
    from smmregrid_amd.device import DeviceArray
    B, n_lev, _, S = q.shape
    lev = np.arange(n_lev, dtype=np.int32)
    x32 = cf.decode(q)
    dq, dx = to_device(q), to_device(x32)
    sb = lambda a: to_device(np.ascontiguousarray(a.reshape(B, n_lev, S).transpose(1, 2, 0)), layout="sb")  # noqa: E731
    dqs, dxs = sb(q), sb(x32)
    del x32
    y = DeviceArray((B, 1, n_lev, grp.n_dst), np.float64)
    ys = DeviceArray((B, n_lev, grp.n_dst), np.float64)
    kw = dict(masked=True, remap_area_min=0.5)
    legs = {
        "C_i16": lambda: grp.apply_sb(dqs, lev, ml, y=ys, cf=cf, **kw),
        "C_f32": lambda: grp.apply_sb(dxs, lev, ml, y=ys, **kw),
        "A_i16": lambda: grp.apply(dq, lev, ml, y=y, cf=cf, **kw),
        "A_f32": lambda: grp.apply(dx, lev, ml, y=y, flags=_lib.APPLY_KERNEL_SELL, **kw),
        "tile_f32": lambda: grp.apply(dx, lev, ml, y=y, **kw),
    }
    res = {"block": "kernel", "levels": int(n_lev), "nsteps": int(B), "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup), 4)}
    res["C_i16_over_f32"] = round(res["ms"]["C_i16"] / res["ms"]["C_f32"], 3)
    res["A_i16_over_f32"] = round(res["ms"]["A_i16"] / res["ms"]["A_f32"], 3)
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=7, warmup=2, only="host,kernel", cfg_rows=False, steps_help="timed repetitions")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the field")
    ap.add_argument("--full", action="store_true", help="75 levels x 120 time steps (BASELINE config 3; ~100 GB of host memory)")
    ap.add_argument("--legs", default="i16,f32,f32b,f64,dec32,dec64")
    return ap


def main():
    args = benchlib.parse(parser(), least=7, why="medians need at least 7 steps")
    if args.full:
        args.levels, args.nsteps = 75, 120
    from smmregrid_amd import CFDecode
    grp, masks, ml = benchlib.build_group(args.levels)
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    q = int16_levels(masks, args.nsteps)
    for block in benchlib.split(args.only):
        if block == "host":
            res = bench_host(grp, ml, q, cf, args.steps, args.warmup, benchlib.split(args.legs))
        else:
            # the kernel block keeps the field on the device four times over: at most 32 time steps of it
            res = bench_kernels(grp, ml, q[:32], cf, args.steps, args.warmup)
        benchlib.emit(res)


if __name__ == "__main__":
    main()
