"""The categorical apply (`SparseOperator.apply_mode`, smm_apply_mode) HBM-resident, beside the two things it is measured
against, in the same run:

  mode       apply_mode on a field of class codes, uint16 and float32, 8 and 64 classes
  sell       the existing row-per-lane SELL apply on the same operator and batch (a float32 field, float64 result): it
             gathers the same cells once -- the floor
  indicator  the route apply_mode replaces: one existing apply per class on the float32 indicator field x == c (the
             indicator fields are resident before the clock starts), the C float64 results copied to the host, and the
             argmax there

on conservative geometries of short, middling and long rows: "cfg5" (r1440x721 -> r720x360, config 5's: 9 links a row),
"mid" (r1440x721 -> r360x180: 25) and "coarse" (r1440x721 -> r180x90: 81, the longest rows of the conservative cases and
past what the kernel's LDS form holds).  Each line says which form of
the kernel the geometry's slices took (smm_mode_launch_info).  The two device legs are timed by HIP events (device ms: at
a tenth of a millisecond the wall clock would time the Python call), interleaved step by step after a warm-up; the
indicator route, which ends on the host, by the wall clock in the same session.  Medians.  One JSON line per geometry and
class count, printed and appended to profiles/mode_bench.jsonl.

  python tools/mode_timing.py [--rows 8] [--steps 7] [--warmup 2] [--only cfg5,mid,coarse] [--classes 8,64]
"""
import numpy as np

import benchlib
from bench_inputs import class_fields

GEOMETRIES = {"cfg5": benchlib.GRIDS["cfg5"], "mid": ("r1440x721", "r360x180", "con"), "coarse": ("r1440x721", "r180x90", "con")}


def bench(name, op, rows, n_classes, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    from smmregrid_amd.device import synchronize
    xs = class_fields((rows, op.n_src), n_classes)
    dev = {k: to_device(v) for k, v in xs.items()}
    ys = {k: DeviceArray((rows, op.n_dst), v.dtype) for k, v in xs.items()}
    y64 = DeviceArray((rows, op.n_dst), np.float64)
    plain = to_device(np.nan_to_num(xs["f32"], nan=0.0))
    inds = [to_device((xs["u16"] == c).astype(np.float32)) for c in range(1, n_classes + 1)]
    host = np.empty((n_classes, rows, op.n_dst), dtype=np.float64)

    def mode(kind):
        kw = dict(fill=(65535,), fill_out=65535) if kind == "u16" else {}
        op.apply_mode(dev[kind], y=ys[kind], **kw)

    def indicator():
        for c, ind in enumerate(inds):
            op.apply(ind, y=y64, flags=_lib.APPLY_KERNEL_SELL).to_host(out=host[c])
        return host.argmax(axis=0)

    legs = {"mode_u16": lambda: mode("u16"), "mode_f32": lambda: mode("f32"),
            "sell_f32": lambda: op.apply(plain, y=y64, flags=_lib.APPLY_KERNEL_SELL)}
    times = benchlib.time_events(legs, steps, warmup)
    synchronize()
    times.update(benchlib.time_wall({"indicator": indicator}, steps, warmup))
    res = {"geometry": name, "grids": list(GEOMETRIES[name]), "rows": int(rows), "classes": int(n_classes), "steps": steps,
           "nnz": int(op.nnz), "max_row_nnz": int(op.max_row_nnz), "clock": {"mode_u16": "events", "mode_f32": "events",
                                                                            "sell_f32": "events", "indicator": "wall"},
           **benchlib.summary(times, 4)}
    ms = res["ms"]
    res["mode_over_sell"] = {k: round(ms[k] / ms["sell_f32"], 2) for k in ("mode_u16", "mode_f32")}
    res["indicator_over_mode"] = {k: round(ms["indicator"] / ms[k], 1) for k in ("mode_u16", "mode_f32")}
    res["form"] = {k: op.mode_launch_info(np.dtype(t)) for k, t in (("u16", np.uint16), ("f32", np.float32))}
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=7, warmup=2, only="cfg5,mid,coarse", out="mode_bench.jsonl", cfg_rows=False)
    ap.add_argument("--rows", type=int, default=8)
    ap.add_argument("--classes", default="8,64")
    return ap


def main():
    args = benchlib.parse(parser())
    for name in benchlib.split(args.only):
        op = benchlib.build_operator(GEOMETRIES[name])
        for n_classes in (int(v) for v in benchlib.split(args.classes)):
            benchlib.emit(bench(name, op, args.rows, n_classes, args.steps, args.warmup), args.out)
        op.close()


if __name__ == "__main__":
    main()
