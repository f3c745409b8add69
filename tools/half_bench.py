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
import numpy as np

import benchlib
from bench_inputs import half_fields

PAIRS = ("f32->f32", "f16->f16", "bf16->bf16")


def _result(block, name, rows, steps, times, digits=4):
    res = {"block": block, "op": name, "rows": int(rows), "steps": steps, **benchlib.summary(times, digits)}
    ms = res["ms"]
    res["over_f32"] = {k: round(ms[k] / ms["f32->f32"], 3) for k in ms if k != "f32->f32"}
    return res


def bench_kernel(op, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    xs = half_fields((rows, op.n_src))
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
    return _result("kernel_c", "cfg2", rows, steps, benchlib.time_events(legs, steps, warmup))


def bench_group(n_lev, n_steps, steps, warmup):
    from smmregrid_amd import DeviceArray, to_device
    grp, _, ml = benchlib.build_group(n_lev)
    lev = np.arange(n_lev, dtype=np.int32)
    xs = half_fields((n_steps, n_lev, grp.n_src))
    legs = {}
    for pair in PAIRS:
        k = pair.split("->")[0]
        dxt = to_device(np.ascontiguousarray(xs[k].transpose(1, 2, 0)), layout="sb")        # (n_lev, S, B)
        y = DeviceArray((n_steps, n_lev, grp.n_dst), xs[k].dtype)
        legs[pair] = lambda dxt=dxt, y=y: grp.apply_sb(dxt, lev, ml, y=y, masked=True, remap_area_min=0.5,
                                                       out_dtype=y.dtype)
    res = _result("group_kernel_c", "cfg3", n_steps, steps, benchlib.time_events(legs, steps, warmup))
    res["levels"] = n_lev
    return res


def bench_host(op, rows, steps, warmup):
    from smmregrid_amd import _lib
    xs = half_fields((rows, op.n_src))
    outs = {k: np.empty((rows, op.n_dst), v.dtype) for k, v in xs.items()}
    legs = {pair: (lambda k=pair.split("->")[0]: op.apply_host(xs[k], out=outs[k], out_dtype=outs[k].dtype, half=True))
            for pair in PAIRS}
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats)
    res = _result("host", "cfg2", rows, steps, times, digits=3)
    res["h2d_bytes"] = {p: int(s[-1]["h2d_bytes"]) for p, s in stats.items()}
    res["d2h_bytes"] = {p: int(s[-1]["d2h_bytes"]) for p, s in stats.items()}
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=9, warmup=2, only="kernel,group,host", out="half_bench.jsonl", cfg_rows=False)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32)
    return ap


def main():
    args = benchlib.parse(parser(), least=7, why="medians need at least 7 steps")
    only = benchlib.split(args.only)
    lines = []
    if "kernel" in only or "host" in only:
        op = benchlib.build_operator("cfg2")
        if "kernel" in only:
            lines.append(bench_kernel(op, args.rows, args.steps, args.warmup))
        if "host" in only:
            lines.append(bench_host(op, args.rows, args.steps, args.warmup))
        op.close()
    if "group" in only:
        lines.append(bench_group(args.levels, args.nsteps, args.steps, args.warmup))
    for line in lines:
        benchlib.emit(line, args.out)


if __name__ == "__main__":
    main()
