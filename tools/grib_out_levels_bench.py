"""Regrid results on masked-level (3-D) weights returned GRIB simple-packed (smm_group_apply_host_grib_pk) against the road
this data took before -- `OperatorGroup.apply_host_grib` without `grib_out`, which brings float64 back -- on the workload
of tools/grib_levels_bench.py: 16 synthetic ocean levels x 32 steps of r1440x721 -> r360x180, conservative weights per
level, every field with a bitmap that equals its level's source mask, the input packed at 16 and at 12 bits and the
result packed at the same width.

One process, host to host, wall-clock ms, pageable input and output, masked epilogue with remap_area_min = 0.5; after a
warm-up the legs run interleaved step by step, in the order below on even steps and in the reverse order on odd ones:
  f64_of_16 / f64_of_12     apply_host_grib on the 16-bit / 12-bit streams, the float64 result into a reused array
  grib_out16 / grib_out12   the same call with grib_out=GribEncode(width), the packed result into a reused buffer
  ..._cache                 the four again without `out`: the result lands in the library's recycled page-locked result
                            cache, straight from the device -- what `Regridder` does
with the median and the best of every leg, the stage split and the bytes each ships up and brings back
(smm_debug_host_stats).  The rows of the first and of the last outer index of every packed result are compared byte for
byte with `GribEncode.encode` of the float64 road's rows before anything is timed.  One JSON line, printed and appended
to profiles/grib_out_levels_bench.jsonl.

  python tools/grib_out_levels_bench.py [--levels 16] [--nsteps 32] [--steps 8] [--warmup 2]
"""
import sys

import numpy as np

import benchlib
from bench_inputs import make_level_streams


def check_outer(what, field, y, enc_w, o, n_lev):
    """The n_lev rows of outer index o of a packed result against the numpy rule on the float64 rows (transpose=True,
    n_inner = 1: y is (n_outer, 1, n_lev, D))."""
    from smmregrid_amd import GRIB_NO_BITMAP, GribEncode
    want = GribEncode(enc_w).encode(y[o, 0])
    r0 = o * n_lev
    base = r0 * (want.buf.size // n_lev)                             # one width: every slot has the same size
    got_rows, got_bm = field.rows[r0:r0 + n_lev].copy(), field.bitmaps[r0:r0 + n_lev].copy()
    got_rows["byte_off"] -= np.uint64(base)
    has = got_bm["bitmap_off"] != np.uint64(GRIB_NO_BITMAP)
    got_bm["bitmap_off"][has] -= np.uint64(base)
    if got_rows.tobytes() != want.rows.tobytes() or got_bm.tobytes() != want.bitmaps.tobytes() \
            or not np.array_equal(np.asarray(field.buf)[base:base + want.buf.size], want.buf):
        raise SystemExit(f"{what}: outer index {o} differs from GribEncode.encode of the float64 result")


def bench(grp, masks, ml, n_steps, steps, warmup):
    from smmregrid_amd import GribEncode, _lib
    n_lev, S = masks.shape
    D = grp.n_dst
    lev = np.arange(n_lev, dtype=np.int32)
    kw = dict(masked=True, remap_area_min=0.5)
    streams = {w: make_level_streams(masks, n_steps, w)[:3] for w in (16, 12)}
    print("# streams packed", file=sys.stderr, flush=True)
    n_rows = n_steps * n_lev
    y = np.empty((n_steps, 1, n_lev, D), np.float64)
    legs, outs = {}, {}
    for w in (16, 12):
        buf, table, bitmaps = streams[w]
        enc = GribEncode(w)
        outs[w] = (enc, np.empty(enc.layout(D, n_rows)[1], np.uint8))
        legs[f"f64_of_{w}"] = lambda buf=buf, table=table, bitmaps=bitmaps: grp.apply_host_grib(
            buf, table, lev, ml, bitmaps=bitmaps, out=y, **kw)
        legs[f"grib_out{w}"] = lambda buf=buf, table=table, bitmaps=bitmaps, w=w: grp.apply_host_grib(
            buf, table, lev, ml, bitmaps=bitmaps, grib_out=outs[w][0], out=outs[w][1], **kw)
        legs[f"f64_of_{w}_cache"] = lambda buf=buf, table=table, bitmaps=bitmaps: grp.apply_host_grib(
            buf, table, lev, ml, bitmaps=bitmaps, **kw)
        legs[f"grib_out{w}_cache"] = lambda buf=buf, table=table, bitmaps=bitmaps, w=w: grp.apply_host_grib(
            buf, table, lev, ml, bitmaps=bitmaps, grib_out=outs[w][0], **kw)
    # bytes first: the first and the last outer index of each packed result against the float64 road of the same width
    for w in (16, 12):
        legs[f"f64_of_{w}"]()
        field = legs[f"grib_out{w}"]()
        for o in (0, n_steps - 1):
            check_outer(f"grib_out{w}", field, y, w, o, n_lev)
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, both_orders=True, announce="# step {}")
    fwd, rev = benchlib.by_order(times, warmup)
    res = {"block": "host_to_host", "levels": int(n_lev), "nsteps": int(n_steps), "n_src": int(S), "n_dst": int(D),
           "steps": steps, "present_share": round(float((masks != 0).mean()), 4), **benchlib.summary(times, 3),
           "ms_fwd": benchlib.summary(fwd, 3)["ms"], "ms_rev": benchlib.summary(rev, 3)["ms"],
           "h2d_bytes": {k: int(s[0]["h2d_bytes"]) for k, s in stats.items()},
           "d2h_bytes": {k: int(s[0]["d2h_bytes"]) for k, s in stats.items()},
           "stages": {k: benchlib.stage_split(s) for k, s in stats.items()},
           "first_and_last_outer_equal_numpy_rule": True}
    for w in (16, 12):
        res[f"f64_over_grib_out{w}"] = round(res["ms"][f"f64_of_{w}"] / res["ms"][f"grib_out{w}"], 3)   # < 1: nothing is won
        res[f"f64_over_grib_out{w}_cache"] = round(res["ms"][f"f64_of_{w}_cache"] / res["ms"][f"grib_out{w}_cache"], 3)
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=8, warmup=2, out="grib_out_levels_bench.jsonl", cfg_rows=False,
                         steps_help="timed repetitions (half in either order)")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the variable")
    return ap


def main():
    args = benchlib.parse(parser(), least=8, both_orders=True,
                          why="an even number of at least 8 timed steps after an even warm-up: both orders get the same share")
    grp, masks, ml = benchlib.build_group(args.levels)
    print(f"# group built: {args.levels} levels, S = {grp.n_src}, D = {grp.n_dst}", file=sys.stderr, flush=True)
    benchlib.emit(bench(grp, masks, ml, args.nsteps, args.steps, args.warmup), args.out)


if __name__ == "__main__":
    main()
