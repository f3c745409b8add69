"""Raw GRIB fields under skipna (the _na entries: apply_grib / apply_host_grib with skipna=True) against the roads such
a call had before, on the geometries of grib_bitmap_bench.py and grib_levels_bench.py with about 30 % of the cells
missing (every cell drawn on its own): config-4 geometry (n1280 -> HEALPix 1024, bilinear) at B = 128, config-2 rows
(r1440x721 -> r360x180) at B = 512, and 16 ocean levels x 32 steps of r1440x721 -> r360x180 (conservative weights per
level; a level's bitmaps are its source mask with a further 30 % of the cells cleared).  16-bit streams; --widths 16,12
adds the 12-bit ones.

One process, the legs interleaved step by step after a warm-up, in the order below on even steps and reversed on odd
ones, median and best:
  kernel  (a) HBM-resident, device ms from HIP events: apply_grib(bitmaps=, skipna=True) as a whole (table build + NA
          gather); the plain bitmapped apply_grib(bitmaps=) on the same bytes; the table build on its own (the same call
          on an operator of the same source grid with ONE link), so that either gather is its total minus the build; and
          smm_apply with SMM_F32 X, SMM_APPLY_SKIPNA and SMM_APPLY_KERNEL_SELL on the HBM-resident decoded field.  The
          levels: OperatorGroup.apply_grib with and without skipna and OperatorGroup.apply(skipna=True) the same way.
  host    (b) host to host, wall-clock ms (the calls return with their result complete), pageable input and output:
          apply_host_grib(skipna=True); apply_host(skipna=True) on the decoded float32 field alone; the parent road =
          griblite's decode of one bitmapped message (timed on its own, per row, scaled to the batch) plus that
          apply_host call -- what Regridder(packed=True, skipna=True) runs without packed_skipna.
--plain-only runs the plain bitmapped legs of the kernel block alone: what a library without the _na entries can run
(SMM_LIB_PATH names it, SMM_LIB_ALLOW_MISSING=1 lets it load), for a parent / branch comparison of the plain gather in
one session; --tag names the build in the record.
Every NA result is compared bit for bit with the decoded road's before anything is timed.  One JSON line per block,
printed and appended to profiles/grib_skipna_bench.jsonl.

  python tools/grib_skipna_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--levels 16] [--nsteps 32] [--steps 8] [--warmup 2]
                                    [--only cfg2,cfg4,levels] [--blocks kernel,host] [--widths 16] [--plain-only] [--tag branch]
"""
import sys

import numpy as np

import benchlib
from bench_inputs import MISSING, make_bitmap_streams, make_level_streams, padded_upload, thinned
from benchlib import same_bits as same


def summary(times, digits):
    s = benchlib.summary(times, digits)
    return s["ms"], s["ms_min"]


def bench_kernel(op, name, rows, args):
    from smmregrid_amd import DeviceArray, _lib, to_device
    S, D_ = op.n_src, op.n_dst
    one = benchlib.one_link_operator(S)                                                   # the build, next to no gather
    y_one = DeviceArray((rows, 1), np.float64)
    legs, check = {}, []
    for nbits in args.widths:
        buf, table, bitmaps, field, _, _ = make_bitmap_streams(S, rows, widths=(nbits,))[nbits]
        dx, n = padded_upload(buf), buf.size
        y_bm = DeviceArray((rows, D_), np.float64)
        if not args.plain_only:
            y_na, y32 = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
            dfield = to_device(field)
            legs[f"na{nbits}_total"] = lambda dx=dx, y=y_na, t=table, b=bitmaps, n=n: op.apply_grib(dx, t, x_bytes=n, y=y, bitmaps=b,
                                                                                                 skipna=True)
            legs[f"f32_sell_na_of_{nbits}"] = lambda x=dfield, y=y32: op.apply(x, y=y, flags=_lib.APPLY_KERNEL_SELL, skipna=True)
            check.append((nbits, y_na, y32))
        legs[f"bm{nbits}_total"] = lambda dx=dx, y=y_bm, t=table, b=bitmaps, n=n: op.apply_grib(dx, t, x_bytes=n, y=y, bitmaps=b)
        legs[f"bm{nbits}_build"] = lambda dx=dx, t=table, b=bitmaps, n=n: one.apply_grib(dx, t, x_bytes=n, y=y_one, bitmaps=b)
        del buf, field

    def bits():
        for nbits, y_na, y32 in check:
            if not same(y_na.to_host(), y32.to_host()):
                raise SystemExit(f"{name}: smm_apply_grib_na at {nbits} bits differs from smm_apply SKIPNA on the decoded field")

    ms, ms_min = summary(benchlib.time_events(legs, args.steps, args.warmup, after_first=bits, both_orders=True), 4)
    one.close()
    res = {"block": "kernel", "op": name, "build": args.tag, "rows": rows, "n_src": S, "n_dst": D_, "steps": args.steps,
           "missing": MISSING, "ms": ms, "ms_min": ms_min, "bits_equal_parent": not args.plain_only or None}
    for nbits in args.widths:
        res[f"bm{nbits}_gather_ms"] = round(ms[f"bm{nbits}_total"] - ms[f"bm{nbits}_build"], 4)
        if not args.plain_only:
            na = ms[f"na{nbits}_total"] - ms[f"bm{nbits}_build"]
            res[f"na{nbits}_gather_ms"] = round(na, 4)
            res[f"na{nbits}_gather_over_bm_gather"] = round(na / res[f"bm{nbits}_gather_ms"], 3)
            res[f"na{nbits}_total_over_bm_total"] = round(ms[f"na{nbits}_total"] / ms[f"bm{nbits}_total"], 3)
            res[f"na{nbits}_total_over_f32_sell_na"] = round(ms[f"na{nbits}_total"] / ms[f"f32_sell_na_of_{nbits}"], 3)
    return res


def bench_host(op, name, rows, args):
    S, D_ = op.n_src, op.n_dst
    streams = make_bitmap_streams(S, rows, widths=tuple(args.widths))
    y_raw, y_f32 = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)
    legs = {}
    for nbits in args.widths:
        buf, table, bitmaps, field, _, _ = streams[nbits]
        legs[f"grib_na{nbits}"] = lambda buf=buf, t=table, b=bitmaps: op.apply_host_grib(buf, t, out=y_raw, bitmaps=b, skipna=True)
        legs[f"f32_na_of_{nbits}"] = lambda field=field: op.apply_host(field, out=y_f32, skipna=True)
        legs[f"grib_na{nbits}"]()
        legs[f"f32_na_of_{nbits}"]()
        if not same(y_raw, y_f32):
            raise SystemExit(f"{name}: apply_host_grib(skipna=True) at {nbits} bits differs from the decoded road")
    ms, ms_min = summary(benchlib.time_wall(legs, args.steps, args.warmup, both_orders=True), 3)
    res = {"block": "host_to_host", "op": name, "build": args.tag, "rows": rows, "n_src": S, "n_dst": D_, "steps": args.steps,
           "missing": MISSING, "ms": ms, "ms_min": ms_min, "bits_equal_parent": True}
    for nbits in args.widths:
        buf, _, _, _, rule, bm = streams[nbits]
        dec = benchlib.time_decode_rule(buf, rule, bm, S, max(5, args.steps))
        res[f"decode{nbits}_ms_per_row"] = benchlib.median_and_min(dec)
        parent = benchlib.median(dec) * rows + ms[f"f32_na_of_{nbits}"]
        res[f"parent_road{nbits}_ms"] = round(parent, 1)          # decode of every row (one thread) + apply_host(skipna=True)
        res[f"parent_over_grib_na{nbits}"] = round(parent / ms[f"grib_na{nbits}"], 2)
        res[f"apply_host_f32_na_over_grib_na{nbits}"] = round(ms[f"f32_na_of_{nbits}"] / ms[f"grib_na{nbits}"], 3)   # < 1: raw loses
    return res


def bench_levels(grp, masks, ml, block, args):
    from smmregrid_amd import DeviceArray, _lib, to_device
    n_lev, S = masks.shape
    lev = np.arange(n_lev, dtype=np.int32)
    kw = dict(masked=True, remap_area_min=0.5)
    legs, streams = {}, {}
    for nbits in args.widths:
        buf, table, bitmaps, field, first = streams[nbits] = make_level_streams(thinned(masks), args.nsteps, nbits)
        if block == "host":
            legs[f"grib_na{nbits}"] = lambda buf=buf, t=table, b=bitmaps: grp.apply_host_grib(buf, t, lev, ml, bitmaps=b, skipna=True,
                                                                                           **kw)
            legs[f"f32_na_of_{nbits}"] = lambda field=field: grp.apply_host(field, lev, ml, skipna=True, **kw)
            got = legs[f"grib_na{nbits}"]().copy()                # results come from a recycled buffer
            if not same(got, legs[f"f32_na_of_{nbits}"]()):
                raise SystemExit(f"levels: apply_host_grib(skipna=True) at {nbits} bits differs from the decoded road")
        else:
            dx, n = padded_upload(buf), buf.size
            shape = (args.nsteps, 1, n_lev, grp.n_dst)
            y_bm = DeviceArray(shape, np.float64)
            if not args.plain_only:
                dfield, y_na, y32 = to_device(field), DeviceArray(shape, np.float64), DeviceArray(shape, np.float64)
                legs[f"na{nbits}"] = lambda dx=dx, t=table, b=bitmaps, n=n, y=y_na: grp.apply_grib(dx, t, lev, ml, bitmaps=b, y=y,
                                                                                                x_bytes=n, skipna=True, **kw)
                legs[f"f32_sell_na_of_{nbits}"] = lambda x=dfield, y=y32: grp.apply(x, lev, ml, y=y, flags=_lib.APPLY_KERNEL_SELL,
                                                                                  skipna=True, **kw)
                if not same(legs[f"na{nbits}"]().to_host(), legs[f"f32_sell_na_of_{nbits}"]().to_host()):
                    raise SystemExit(f"levels: smm_group_apply_grib_na at {nbits} bits differs from the decoded field's result")
            legs[f"bm{nbits}"] = lambda dx=dx, t=table, b=bitmaps, n=n, y=y_bm: grp.apply_grib(dx, t, lev, ml, bitmaps=b, y=y,
                                                                                            x_bytes=n, **kw)
    host = block == "host"
    timer = benchlib.time_wall if host else benchlib.time_events
    ms, ms_min = summary(timer(legs, args.steps, args.warmup, both_orders=True), 3 if host else 4)
    res = {"block": "host_to_host" if host else "kernel", "op": "levels", "build": args.tag, "levels": int(n_lev),
           "nsteps": int(args.nsteps), "n_src": int(S), "n_dst": int(grp.n_dst), "steps": args.steps, "missing": MISSING,
           "present_share": round(float((thinned(masks) != 0).mean()), 4), "ms": ms, "ms_min": ms_min,
           "bits_equal_parent": not args.plain_only or None}
    for nbits in args.widths:
        if host:
            dec = benchlib.time_level_decode(streams[nbits][0], streams[nbits][4], S, max(5, args.steps)) * args.nsteps
            res[f"decode{nbits}_ms"] = round(dec, 1)
            res[f"parent_road{nbits}_ms"] = round(dec + ms[f"f32_na_of_{nbits}"], 1)
            res[f"parent_over_grib_na{nbits}"] = round((dec + ms[f"f32_na_of_{nbits}"]) / ms[f"grib_na{nbits}"], 2)
            res[f"apply_host_f32_na_over_grib_na{nbits}"] = round(ms[f"f32_na_of_{nbits}"] / ms[f"grib_na{nbits}"], 3)
        elif not args.plain_only:                                   # totals: the table build is in both raw legs
            res[f"na{nbits}_over_bm{nbits}"] = round(ms[f"na{nbits}"] / ms[f"bm{nbits}"], 3)
            res[f"na{nbits}_over_f32_sell_na"] = round(ms[f"na{nbits}"] / ms[f"f32_sell_na_of_{nbits}"], 3)
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=8, warmup=2, only="cfg2,cfg4,levels", blocks="kernel,host", out="grib_skipna_bench.jsonl",
                         steps_help="timed repetitions (half in either order)")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the levels variable")
    ap.add_argument("--widths", default="16")
    ap.add_argument("--plain-only", action="store_true")
    ap.add_argument("--tag", default="branch")
    return ap


def main():
    args = benchlib.parse(parser(), least=6, both_orders=True,
                          why="an even number of at least 6 timed steps after an even warm-up: both orders get the same share")
    args.widths = [int(w) for w in args.widths.split(",")]
    blocks = ["kernel"] if args.plain_only else benchlib.split(args.blocks)
    cases = benchlib.split(args.only)
    args.only = ",".join(c for c in cases if c != "levels")
    for name, op, rows in benchlib.operators(args) if args.only else ():
        for block in blocks:
            benchlib.emit((bench_host if block == "host" else bench_kernel)(op, name, rows, args), args.out)
    if "levels" in cases:                                   # the operators first, the group behind them
        grp, masks, ml = benchlib.build_group(args.levels)
        print(f"# levels: group built, S = {grp.n_src}, D = {grp.n_dst}", file=sys.stderr, flush=True)
        for block in blocks:
            benchlib.emit(bench_levels(grp, masks, ml, block, args), args.out)
        grp.close()


if __name__ == "__main__":
    main()
