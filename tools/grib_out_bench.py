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
import sys

import numpy as np

import benchlib
from bench_inputs import make_streams, padded_upload


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

    def check(leg, res):
        if leg.startswith("grib_out"):      # the float64 leg of the same width ran just before
            check_row0(name, leg, res, y[0], outs[int(leg[8:])][0])
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, check=check,
                                      announce=f"# {name}: host step {{}}")
    out = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           **benchlib.summary(times, 3),
           "h2d_bytes": {k: int(s[-1]["h2d_bytes"]) for k, s in stats.items()},
           "d2h_bytes": {k: int(s[-1]["d2h_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s[-1]["chunks"]) for k, s in stats.items()}, "row0_equals_numpy_rule": True}
    for w in (16, 12):
        out[f"f64_over_grib_out{w}"] = round(out["ms"][f"f64_of_{w}"] / out["ms"][f"grib_out{w}"], 3)
    return out


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, GribEncode, GribField, grib_pack
    S, D_ = op.n_src, op.n_dst
    legs, checks = {}, {}
    for w in (16, 12):
        buf, table, _, *_ = make_streams(S, rows, 0, widths=(w,))[w]
        dx, y = padded_upload(buf), DeviceArray((rows, D_), np.float64)
        enc = GribEncode(w)
        out = DeviceArray((enc.layout(D_, rows)[1],), np.uint8)
        legs[f"gather{w}"] = lambda dx=dx, y=y, table=table, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y)
        legs[f"pack{w}"] = lambda y=y, enc=enc, out=out: grib_pack(y, enc, out=out)
        checks[w] = (y, enc)
        del buf

    def check(leg, res):
        if leg.startswith("pack"):
            y, enc = checks[int(leg[4:])]
            packed, prow, pbm = res
            n0 = enc.layout(D_, 1)[1]
            head = DeviceArray((n0,), np.uint8, ptr=packed.ptr, base=packed).to_host()
            check_row0(name, leg, GribField(head, prow[:1], (1, D_), D_, bitmaps=pbm[:1]), y.rows(0, 1).to_host()[0], enc)
    out = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup, check=check), 4), "row0_equals_numpy_rule": True}
    ms = out["ms"]
    out["pack_over_gather"] = {str(w): round(ms[f"pack{w}"] / ms[f"gather{w}"], 3) for w in (16, 12)}
    return out


def parser():
    return benchlib.parser(__doc__, steps=7, warmup=2, only="cfg2,cfg4", blocks="host,kernel", out="grib_out_bench.jsonl")


def main():
    args = benchlib.parse(parser())
    for name, op, rows in benchlib.operators(args):
        for block in benchlib.split(args.blocks):
            benchlib.emit((bench_host if block == "host" else bench_kernel)(op, name, rows, args.steps, args.warmup), args.out)


if __name__ == "__main__":
    main()
