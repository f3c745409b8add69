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
import numpy as np

import benchlib
from bench_inputs import int16_rows


def bench_host(name, op, q, cf, enc, steps, warmup):
    from smmregrid_amd import _lib
    out16 = np.empty((q.shape[0], op.n_dst), np.int16)
    out64 = np.empty((q.shape[0], op.n_dst))
    legs = {
        "i16->i16": lambda: op.apply_host(q, out=out16, cf=cf, cf_out=enc),
        "i16->f64": lambda: op.apply_host(q, out=out64, cf=cf),
        "i16->f64+enc": lambda: enc.encode(op.apply_host(q, out=out64, cf=cf)),
    }
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats)
    res = {"block": "host", "op": name, "rows": int(q.shape[0]), "steps": steps, **benchlib.summary(times, 3)}
    for leg in ("i16->i16", "i16->f64"):
        res["stages_" + leg] = benchlib.stage_split(stats[leg])
        res["d2h_bytes_" + leg] = int(stats[leg][0]["d2h_bytes"])
        res["h2d_bytes_" + leg] = int(stats[leg][0]["h2d_bytes"])
    res["i16_over_f64"] = round(res["ms"]["i16->i16"] / res["ms"]["i16->f64"], 3)
    res["i16_over_f64_enc"] = round(res["ms"]["i16->i16"] / res["ms"]["i16->f64+enc"], 3)
    return res


def bench_kernels(name, op, q, cf, enc, steps, warmup):
    from smmregrid_amd import CFDecode, _lib, to_device
    from smmregrid_amd.device import DeviceArray
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
    res = {"block": "kernel", "op": name, "rows": int(B), "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup), 4)}
    ms = res["ms"]
    res["packed_over_f64"] = {k: round(ms[k] / ms[k.replace("->i16", "->f64").replace("_td16", "")], 3)
                              for k in ms if "->i16" in k}
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=9, warmup=2, only="host,kernel", cfg_rows=False)
    ap.add_argument("--rows", type=int, default=512)
    ap.add_argument("--ops", default="cfg2,cfg5")
    return ap


def main():
    ap = parser()
    args = benchlib.parse(ap, least=7, why="medians need at least 7 steps")
    from smmregrid_amd import CFDecode, CFEncode
    cf = CFDecode(1.9e-3, 2.7e2, (-32768,), np.float32)
    enc = CFEncode(1.9e-3, 2.7e2, -32768, np.int16)
    for name in benchlib.split(args.ops):
        if name not in ("cfg2", "cfg5"):
            ap.error(f"unknown operator {name}")
        op = benchlib.build_operator(name)
        q = int16_rows(args.rows, op.n_src)
        for block in benchlib.split(args.only):
            benchlib.emit({"host": bench_host, "kernel": bench_kernels}[block](name, op, q, cf, enc, args.steps, args.warmup))
        op.close()


if __name__ == "__main__":
    main()
