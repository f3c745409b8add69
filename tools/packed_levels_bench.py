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
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

NX, NY = 1440, 721
STAGES = ("stage_in_ms", "h2d_ms", "kernel_ms", "d2h_ms", "copy_out_ms", "wait_ms", "chunks")


def _median(v):
    return float(np.median(np.asarray(v)))


def build_group(n_lev):
    from smmregrid_amd import OperatorGroup, gridgen
    from smmregrid_amd.weights import compute_weights_matrix3d
    masks = gridgen.synthetic_ocean_masks(NX, NY, n_lev)
    w3 = gridgen.ConservativeLevels(gridgen.regular_grid(NX, NY), "r360x180").stack(masks, np.arange(n_lev, dtype=np.float64))
    ops = compute_weights_matrix3d(w3, "lev", device=0)
    imask = np.stack([op.mask_apply(masks[i]) for i, op in enumerate(ops)])
    for i, op in enumerate(ops):
        op.set_epilogue(imask[i], w3["dst_grid_frac"].values[i])
    return OperatorGroup(ops), masks, (~(imask == 1).all(axis=1)).astype(np.uint8)


def field(masks, n_steps, seed=20261016):
    """(n_steps, n_lev, 1, S) int16: full range over the ocean, -32768 (_FillValue) where the level's mask is 0;
    4 distinct time steps, tiled."""
    rng = np.random.default_rng(seed)
    n_lev, S = masks.shape
    blk = rng.integers(-32767, 32768, size=(4, n_lev, 1, S)).astype(np.int16)
    blk[:, masks[:, None, :] == 0] = -32768
    return np.ascontiguousarray(np.tile(blk, ((n_steps + 3) // 4, 1, 1, 1))[:n_steps])


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
    times = {k: [] for k in legs}
    stats = {k: [] for k in legs if not k.startswith("dec")}
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
    res = {"block": "host", "levels": int(n_lev), "nsteps": int(q.shape[0]), "cells": int(q.size), "steps": steps,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "ms_max": {k: round(max(v), 3) for k, v in times.items()}}
    for name, sts in stats.items():
        res["stages_" + name] = {k: round(_median([s[k] for s in sts]), 3) for k in STAGES}
        res["h2d_bytes_" + name] = int(sts[0]["h2d_bytes"])
    ms = res["ms"]
    if "i16" in ms and "f32" in ms:
        res["i16_over_f32"] = round(ms["i16"] / ms["f32"], 3)
    if "i16" in ms and "f64" in ms:
        res["i16_over_f64"] = round(ms["i16"] / ms["f64"], 3)
    if "f32" in ms and "f32b" in ms:
        # run-to-run spread of the float32 leg: its two medians against each other, and the range of all its samples
        both = times["f32"] + times["f32b"]
        res["f32_spread"] = {"median_ratio": round(ms["f32b"] / ms["f32"], 3),
                             "range_over_median": round((max(both) - min(both)) / _median(both), 3)}
    return res


def bench_kernels(grp, ml, q, cf, steps, warmup):
    from smmregrid_amd import _lib, to_device
    from smmregrid_amd.device import DeviceArray, Event
    B, n_lev, _, S = q.shape
    lev = np.arange(n_lev, dtype=np.int32)
    x32 = cf.decode(q)
    dq, dx = to_device(q), to_device(x32)
    sb = lambda a: to_device(np.ascontiguousarray(a.reshape(B, n_lev, S).transpose(1, 2, 0)), layout="sb")
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
    res = {"block": "kernel", "levels": int(n_lev), "nsteps": int(B), "steps": steps,
           "ms": {k: round(_median(v), 4) for k, v in times.items()},
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}}
    res["C_i16_over_f32"] = round(res["ms"]["C_i16"] / res["ms"]["C_f32"], 3)
    res["A_i16_over_f32"] = round(res["ms"]["A_i16"] / res["ms"]["A_f32"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the field")
    ap.add_argument("--full", action="store_true", help="75 levels x 120 time steps (BASELINE config 3; ~100 GB of host memory)")
    ap.add_argument("--steps", type=int, default=7, help="timed repetitions")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="host,kernel")
    ap.add_argument("--legs", default="i16,f32,f32b,f64,dec32,dec64")
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("medians need at least 7 steps")
    if args.full:
        args.levels, args.nsteps = 75, 120
    from smmregrid_amd import CFDecode
    grp, masks, ml = build_group(args.levels)
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    q = field(masks, args.nsteps)
    for block in args.only.split(","):
        if block.strip() == "host":
            res = bench_host(grp, ml, q, cf, args.steps, args.warmup, [s.strip() for s in args.legs.split(",")])
        else:
            # the kernel block keeps the field on the device four times over: at most 32 time steps of it
            res = bench_kernels(grp, ml, q[:32], cf, args.steps, args.warmup)
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
