"""Regrid results returned GRIB simple-packed (smm_apply_host_grib_pk, smm_grib_pack) against the road this data took
before -- the same call without `grib_out`, which brings float64 back -- on config-4 geometry (regular Gaussian n1280 ->
HEALPix 1024, bilinear) at B = 128 and on config-2 rows (r1440x721 -> r360x180) at 512, the input packed at 16 and at
12 bits and the result packed at the same width.

One process, the legs interleaved step by step after a warm-up, median and best of >= 5:
  host    host to host, wall-clock ms, pageable input and output: apply_host_grib(grib_out=GribEncode(w)) against
          apply_host_grib of the same streams, and the bytes each brings back (smm_debug_host_stats)
  kernel  HBM-resident, device ms from HIP events: grib_pack of the gather's float64 result (range + bitmap, rule, rank
          tables, pack -- with the allocation of its scratch and its upload of the row tables in the interval) against the
          gather smm_apply_grib that produces it
Row 0 of every packed result is compared byte for byte with GribEncode.encode of the float64 road's row before anything
is timed.  One JSON line per block, printed and appended to profiles/grib_out_bench.jsonl.

  python tools/grib_out_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 7] [--warmup 2] [--only cfg2,cfg4] [--blocks host,kernel]
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

from tools.grib_bench import _median, make_streams      # noqa: E402


def check_row0(name, what, field, y_row, enc):
    """Row 0 of a packed result against the numpy rule on the float64 row."""
    want = enc.encode(y_row[None, :])
    n = want.buf.size
    if field.rows[0].tobytes() != want.rows[0].tobytes() or field.bitmaps[0].tobytes() != want.bitmaps[0].tobytes() \
            or not np.array_equal(np.asarray(field.buf)[:n], want.buf):
        raise SystemExit(f"{name}: {what} differs from GribEncode.encode of the float64 result")


def bench_host(op, name, rows, steps, warmup):
    from smmregrid_amd import GribEncode, _lib
    S, D_ = op.n_src, op.n_dst
    streams = make_streams(S, rows, 0)
    print(f"# {name}: streams packed", file=sys.stderr, flush=True)
    y = np.empty((rows, D_), np.float64)
    legs, outs = {}, {}
    for w in (16, 12):
        enc = GribEncode(w)
        outs[w] = (enc, np.empty(enc.layout(D_, rows)[1], np.uint8))
        legs[f"f64_of_{w}"] = lambda w=w: op.apply_host_grib(streams[w][0], streams[w][1], out=y)
        legs[f"grib_out{w}"] = lambda w=w: op.apply_host_grib(streams[w][0], streams[w][1], grib_out=outs[w][0], out=outs[w][1])
    times, stats = {k: [] for k in legs}, {}
    for step in range(warmup + steps):
        print(f"# {name}: host step {step}", file=sys.stderr, flush=True)
        for leg, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            res = fn()
            dt = (time.perf_counter() - t0) * 1e3
            stats[leg] = _lib.host_stats(reset=True)
            if step >= warmup:
                times[leg].append(dt)
            if step == 0 and leg.startswith("grib_out"):      # the float64 leg of the same width ran just before
                check_row0(name, leg, res, y[0], outs[int(leg[8:])][0])
    out = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "h2d_bytes": {k: int(s["h2d_bytes"]) for k, s in stats.items()},
           "d2h_bytes": {k: int(s["d2h_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s["chunks"]) for k, s in stats.items()}, "row0_equals_numpy_rule": True}
    for w in (16, 12):
        out[f"f64_over_grib_out{w}"] = round(out["ms"][f"f64_of_{w}"] / out["ms"][f"grib_out{w}"], 3)
    return out


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, GribEncode, GribField, grib_pack, to_device
    from smmregrid_amd.device import Event
    S, D_ = op.n_src, op.n_dst
    legs, check = {}, {}
    for w in (16, 12):
        buf, table, _, *_ = make_streams(S, rows, 0, widths=(w,))[w]
        padded = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
        padded[:buf.size] = buf
        dx, y = to_device(padded), DeviceArray((rows, D_), np.float64)
        enc = GribEncode(w)
        out = DeviceArray((enc.layout(D_, rows)[1],), np.uint8)
        legs[f"gather{w}"] = lambda dx=dx, y=y, table=table, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y)
        legs[f"pack{w}"] = lambda y=y, enc=enc, out=out: grib_pack(y, enc, out=out)
        check[w] = (y, enc)
        del buf, padded
    e0, e1 = Event(), Event()
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        for leg, fn in legs.items():
            e0.record()
            res = fn()
            e1.record()
            e1.synchronize()
            if step >= warmup:
                times[leg].append(e0.elapsed_ms(e1))
            if step == 0 and leg.startswith("pack"):
                y, enc = check[int(leg[4:])]
                packed, prow, pbm = res
                n0 = enc.layout(D_, 1)[1]
                head = DeviceArray((n0,), np.uint8, ptr=packed.ptr, base=packed).to_host()
                check_row0(name, leg, GribField(head, prow[:1], (1, D_), D_, bitmaps=pbm[:1]), y.rows(0, 1).to_host()[0], enc)
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    out = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}, "row0_equals_numpy_rule": True}
    out["pack_over_gather"] = {str(w): round(ms[f"pack{w}"] / ms[f"gather{w}"], 3) for w in (16, 12)}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="host,kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_out_bench.jsonl"))
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("median and best need at least 5 timings")
    from smmregrid_amd import SparseOperator, gridgen
    cases = {"cfg4": ("n1280", "hp1024", args.cfg4_rows), "cfg2": ("r1440x721", "r360x180", args.cfg2_rows)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in [c.strip() for c in args.only.split(",")]:
        sgrid, tgrid, rows = cases[name]
        w = gridgen.generate_weights(sgrid, tgrid, method="bil")
        op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                            w["dst_address"].values, w["remap_matrix"].values, device=0)
        print(f"# {name}: operator built (S = {op.n_src}, D = {op.n_dst}), {rows} rows", file=sys.stderr, flush=True)
        for block in [b.strip() for b in args.blocks.split(",")]:
            res = (bench_host if block == "host" else bench_kernel)(op, name, rows, args.steps, args.warmup)
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        op.close()


if __name__ == "__main__":
    main()
