"""Half-precision fields and results (float16 / bfloat16, SMM_F16 / SMM_BF16) against float32 -> float32 at the same
shape in the same run, on config-2 rows (r1440x721 -> r360x180 bilinear, single operator) and on a config-3-shaped level
group (conservative r1440x721 -> r360x180 weights on synthetic ocean masks).

One process, the legs interleaved step by step after a warm-up, medians of >= 7:
  kernel  device ms (HIP events) of kernel C (X (S, B)) on config 2 and of the grouped kernel C (X (n_lev, S, B)) on
          the group, f32->f32, f16->f16 and bf16->bf16 (a 2-byte Y at 64 and, _td16, at 16 destination rows per tile)
  host    smm_apply_host host to host on config 2, wall-clock ms, pageable input and output, the same three pairs, plus
          the H2D / D2H bytes (smm_debug_host_stats)
One JSON line per block, printed and appended to profiles/half_bench.jsonl.

  python tools/half_bench.py [--rows 512] [--levels 16] [--nsteps 32] [--steps 9] [--warmup 2] [--only kernel,group,host]
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

PAIRS = ("f32->f32", "f16->f16", "bf16->bf16")


def _median(v):
    return float(np.median(np.asarray(v)))


def _fields(shape, seed=20261018):
    """The same values as float32, float16 and bfloat16 (16 distinct rows, tiled along the first axis)."""
    from smmregrid_amd import to_bfloat16
    rng = np.random.default_rng(seed)
    blk = (250.0 + 30.0 * rng.standard_normal((16,) + tuple(shape[1:]))).astype(np.float32)
    x32 = np.ascontiguousarray(np.tile(blk, ((shape[0] + 15) // 16,) + (1,) * (len(shape) - 1))[:shape[0]])
    return {"f32": x32, "f16": x32.astype(np.float16), "bf16": to_bfloat16(x32)}


def _time_device(legs, steps, warmup):
    from smmregrid_amd.device import Event
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
    return times


def _result(block, name, rows, steps, times, digits=4):
    ms = {k: round(_median(v), digits) for k, v in times.items()}
    return {"block": block, "op": name, "rows": int(rows), "steps": steps, "ms": ms,
            "ms_min": {k: round(min(v), digits) for k, v in times.items()},
            "over_f32": {k: round(ms[k] / ms["f32->f32"], 3) for k in ms if k != "f32->f32"}}


def bench_kernel(op, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    xs = _fields((rows, op.n_src))
    legs = {}
    for pair in PAIRS:
        k = pair.split("->")[0]
        dxt = to_device(np.ascontiguousarray(xs[k].T), layout="sb")
        y = DeviceArray((rows, op.n_dst), xs[k].dtype)
        legs[pair] = lambda dxt=dxt, y=y: op.apply_sb(dxt, y=y, out_dtype=y.dtype)
        if k != "f32":
            def td16(dxt=dxt, y=y):
                with _lib.tuning(sb_packed_y_rows=16):
                    op.apply_sb(dxt, y=y, out_dtype=y.dtype)
            legs[pair + "_td16"] = td16
    return _result("kernel_c", "cfg2", rows, steps, _time_device(legs, steps, warmup))


def bench_group(n_lev, n_steps, steps, warmup):
    from smmregrid_amd import DeviceArray, to_device
    from tools.packed_levels_bench import build_group
    grp, _, ml = build_group(n_lev)
    lev = np.arange(n_lev, dtype=np.int32)
    xs = _fields((n_steps, n_lev, grp.n_src))
    legs = {}
    for pair in PAIRS:
        k = pair.split("->")[0]
        dxt = to_device(np.ascontiguousarray(xs[k].transpose(1, 2, 0)), layout="sb")        # (n_lev, S, B)
        y = DeviceArray((n_steps, n_lev, grp.n_dst), xs[k].dtype)
        legs[pair] = lambda dxt=dxt, y=y: grp.apply_sb(dxt, lev, ml, y=y, masked=True, remap_area_min=0.5,
                                                       out_dtype=y.dtype)
    res = _result("group_kernel_c", "cfg3", n_steps, steps, _time_device(legs, steps, warmup))
    res["levels"] = n_lev
    return res


def bench_host(op, rows, steps, warmup):
    from smmregrid_amd import _lib
    xs = _fields((rows, op.n_src))
    outs = {k: np.empty((rows, op.n_dst), v.dtype) for k, v in xs.items()}
    times = {p: [] for p in PAIRS}
    stats = {}
    for step in range(warmup + steps):
        for pair in PAIRS:
            k = pair.split("->")[0]
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            op.apply_host(xs[k], out=outs[k], out_dtype=outs[k].dtype, half=True)
            dt = (time.perf_counter() - t0) * 1e3
            stats[pair] = _lib.host_stats(reset=True)
            if step >= warmup:
                times[pair].append(dt)
    res = _result("host", "cfg2", rows, steps, times, digits=3)
    res["h2d_bytes"] = {p: int(s["h2d_bytes"]) for p, s in stats.items()}
    res["d2h_bytes"] = {p: int(s["d2h_bytes"]) for p, s in stats.items()}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32)
    ap.add_argument("--steps", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="kernel,group,host")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "half_bench.jsonl"))
    args = ap.parse_args()
    if args.steps < 7:
        ap.error("medians need at least 7 steps")
    from smmregrid_amd import SparseOperator, gridgen
    only = [b.strip() for b in args.only.split(",")]
    lines = []
    if "kernel" in only or "host" in only:
        w = gridgen.bilinear_weights("r1440x721", "r360x180")
        op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                            w["dst_address"].values, w["remap_matrix"].values, device=0)
        if "kernel" in only:
            lines.append(bench_kernel(op, args.rows, args.steps, args.warmup))
        if "host" in only:
            lines.append(bench_host(op, args.rows, args.steps, args.warmup))
        op.close()
    if "group" in only:
        lines.append(bench_group(args.levels, args.nsteps, args.steps, args.warmup))
    with open(args.out, "a") as f:
        for line in lines:
            print(json.dumps(line), flush=True)
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
