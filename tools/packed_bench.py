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
import numpy as np

import benchlib
from bench_inputs import int16_rows


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
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats)
    res = {"block": "host", "rows": int(q.shape[0]), "steps": steps, **benchlib.summary(times, 3)}
    for name in ("i16", "f32", "f64"):
        res["stages_" + name] = benchlib.stage_split(stats[name])
        res["h2d_bytes_" + name] = int(stats[name][0]["h2d_bytes"])
    res["i16_over_f32"] = round(res["ms"]["i16"] / res["ms"]["f32"], 3)
    res["i16_over_f64"] = round(res["ms"]["i16"] / res["ms"]["f64"], 3)
    return res


def bench_kernels(op, q, cf, steps, warmup):
    from smmregrid_amd import _lib, to_device
    from smmregrid_amd.device import DeviceArray
    x32 = cf.decode(q)
    B = q.shape[0]
    dq, dx = to_device(q), to_device(x32)
    dqt = to_device(np.ascontiguousarray(q.T), layout="sb")
    dxt = to_device(np.ascontiguousarray(x32.T), layout="sb")
    y = DeviceArray((B, op.n_dst), np.float64)
    legs = {
        "A_i16": lambda: op.apply(dq, y=y, cf=cf),
        "A_f32": lambda: op.apply(dx, y=y, flags=_lib.APPLY_KERNEL_SELL),
        "tile_f32": lambda: op.apply(dx, y=y),
        "C_i16": lambda: op.apply_sb(dqt, y=y, cf=cf),
        "C_f32": lambda: op.apply_sb(dxt, y=y),
    }
    res = {"block": "kernel", "rows": int(B), "steps": steps, **benchlib.summary(benchlib.time_events(legs, steps, warmup), 4)}
    res["A_i16_over_f32"] = round(res["ms"]["A_i16"] / res["ms"]["A_f32"], 3)
    res["C_i16_over_f32"] = round(res["ms"]["C_i16"] / res["ms"]["C_f32"], 3)
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=9, warmup=2, only="host,kernel", cfg_rows=False)
    ap.add_argument("--rows", type=int, default=512)
    return ap


def main():
    args = benchlib.parse(parser(), least=7, why="medians need at least 7 steps")
    from smmregrid_amd import CFDecode
    op = benchlib.build_operator("cfg2")
    cf = CFDecode(1.9e-3, 2.7e2, (-32768,), np.float32)
    q = int16_rows(args.rows, op.n_src)
    for block in benchlib.split(args.only):
        benchlib.emit({"host": bench_host, "kernel": bench_kernels}[block](op, q, cf, args.steps, args.warmup))


if __name__ == "__main__":
    main()
