"""Bitmapped GRIB fields regridded raw (smm_apply_grib_bm / smm_apply_host_grib_bm) against the only road such data had
before -- decode every message in numpy (griblite: unpack the values, unpack the bitmap, scatter into NaN), then regrid
the float32 field -- on config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, bilinear) at B = 128 and on config-2
rows (r1440x721 -> r360x180) at B = 512, with about 30 % of the cells missing (every cell drawn on its own), the same
integers packed at 16 and at 12 bits per value.

One process, the legs interleaved step by step after a warm-up, median and best of >= 5:
  host    (a) host to host, wall-clock ms, pageable input and output: apply_host_grib(bitmaps=) on the 16-bit and the
          12-bit streams; the parent road = griblite's decode of one bitmapped message (timed on its own, per row, and
          scaled to the batch) followed by apply_host on the float32 field; the bytes each ships
  kernel  (b) HBM-resident, device ms from HIP events: apply_grib(bitmaps=) as a whole (table build + gather); the table
          build on its own, taken from the same call on an operator of the same source grid with ONE link (its gather
          is one block of nothing); the gather as the difference of the two; against apply_grib without bitmaps on a
          full field of the same width and smm_apply with SMM_F32 X and SMM_APPLY_KERNEL_SELL on the decoded field
Every raw result is compared bit for bit with the decoded road's before anything is timed.  One JSON line per block,
printed and appended to profiles/grib_bitmap_bench.jsonl.

  python tools/grib_bitmap_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 7] [--warmup 2] [--only cfg2,cfg4] [--blocks host,kernel]
"""
import sys

import numpy as np

import benchlib
from bench_inputs import MISSING, make_bitmap_streams, make_streams, padded_upload
from benchlib import same_bits as same
from benchlib import time_decode_rule as time_decode


def bench_host(op, name, rows, steps, warmup):
    from smmregrid_amd import _lib
    S, D_ = op.n_src, op.n_dst
    streams = make_bitmap_streams(S, rows)
    print(f"# {name}: streams packed", file=sys.stderr, flush=True)
    y_raw, y_f32 = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)
    legs = {}
    for nbits in (16, 12):
        buf, table, bitmaps, field, _, _ = streams[nbits]
        legs[f"gribbm{nbits}"] = lambda buf=buf, table=table, bitmaps=bitmaps: op.apply_host_grib(buf, table, out=y_raw,
                                                                                                 bitmaps=bitmaps)
        legs[f"f32_of_{nbits}"] = lambda field=field: op.apply_host(field, out=y_f32)

    def check(leg, _):
        if leg.startswith("f32_of_") and not same(y_raw, y_f32):      # the raw leg ran just before
            raise SystemExit(f"{name}: apply_host_grib(bitmaps=) at {leg[7:]} bits differs from the decoded road")
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, check=check,
                                      announce=f"# {name}: host step {{}}")
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING,
           **benchlib.summary(times, 3),
           "h2d_bytes": {k: int(s[-1]["h2d_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s[-1]["chunks"]) for k, s in stats.items()}, "bits_equal_parent": True}
    for nbits in (16, 12):
        buf, _, _, _, rule, bm = streams[nbits]
        dec = time_decode(buf, rule, bm, S, max(5, steps))
        res[f"decode{nbits}_ms_per_row"] = benchlib.median_and_min(dec)
        parent = benchlib.median(dec) * rows + res["ms"][f"f32_of_{nbits}"]
        res[f"parent_road{nbits}_ms"] = round(parent, 1)          # decode of every row (one thread) + apply_host
        res[f"parent_over_gribbm{nbits}"] = round(parent / res["ms"][f"gribbm{nbits}"], 2)
        res[f"apply_host_f32_over_gribbm{nbits}"] = round(res["ms"][f"f32_of_{nbits}"] / res["ms"][f"gribbm{nbits}"], 3)
    return res


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    S, D_ = op.n_src, op.n_dst
    one = benchlib.one_link_operator(S)                                                   # the build, next to no gather
    legs, check = {}, {}
    y_one = DeviceArray((rows, 1), np.float64)
    for nbits in (16, 12):
        buf, table, bitmaps, field, _, _ = make_bitmap_streams(S, rows, widths=(nbits,))[nbits]
        dx, y = padded_upload(buf), DeviceArray((rows, D_), np.float64)
        legs[f"gribbm{nbits}_total"] = lambda dx=dx, y=y, t=table, b=bitmaps, n=buf.size: op.apply_grib(dx, t, x_bytes=n, y=y,
                                                                                                     bitmaps=b)
        legs[f"gribbm{nbits}_build"] = lambda dx=dx, t=table, b=bitmaps, n=buf.size: one.apply_grib(dx, t, x_bytes=n, y=y_one,
                                                                                                  bitmaps=b)
        dfield, y32 = to_device(field), DeviceArray((rows, D_), np.float64)
        legs[f"f32_sell_of_{nbits}"] = lambda dfield=dfield, y32=y32: op.apply(dfield, y=y32, flags=_lib.APPLY_KERNEL_SELL)
        check[nbits] = (y, y32)
        del buf, field
        fbuf, ftable, *_ = make_streams(S, rows, 0, widths=(nbits,))[nbits]            # a full field, no bitmap
        fx, fy = padded_upload(fbuf), DeviceArray((rows, D_), np.float64)
        legs[f"grib{nbits}_full"] = lambda fx=fx, fy=fy, t=ftable, n=fbuf.size: op.apply_grib(fx, t, x_bytes=n, y=fy)
        del fbuf

    def bits():
        for nbits, (y, y32) in check.items():
            if not same(y.to_host(), y32.to_host()):
                raise SystemExit(f"{name}: smm_apply_grib_bm at {nbits} bits differs from smm_apply on the decoded field")
    times = benchlib.time_events(legs, steps, warmup, after_first=bits)
    one.close()
    res = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING,
           **benchlib.summary(times, 4), "bits_equal_parent": True}
    ms = res["ms"]
    for nbits in (16, 12):
        gather = ms[f"gribbm{nbits}_total"] - ms[f"gribbm{nbits}_build"]
        res[f"gribbm{nbits}_gather_ms"] = round(gather, 4)                        # total - build
        res[f"gribbm{nbits}_gather_over_grib_full"] = round(gather / ms[f"grib{nbits}_full"], 3)
        res[f"gribbm{nbits}_total_over_grib_full"] = round(ms[f"gribbm{nbits}_total"] / ms[f"grib{nbits}_full"], 3)
        res[f"gribbm{nbits}_total_over_f32_sell"] = round(ms[f"gribbm{nbits}_total"] / ms[f"f32_sell_of_{nbits}"], 3)
    return res


def parser():
    return benchlib.parser(__doc__, steps=7, warmup=2, only="cfg2,cfg4", blocks="host,kernel", out="grib_bitmap_bench.jsonl")


def main():
    args = benchlib.parse(parser())
    for name, op, rows in benchlib.operators(args):
        for block in benchlib.split(args.blocks):
            benchlib.emit((bench_host if block == "host" else bench_kernel)(op, name, rows, args.steps, args.warmup), args.out)


if __name__ == "__main__":
    main()
