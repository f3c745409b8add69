"""Raw GRIB fields on masked-level (3-D) weights (smm_group_apply_host_grib) against the two roads such data has without
it, on the shape of the `packed_levels` figures: 16 synthetic ocean levels x 32 steps of r1440x721 -> r360x180,
conservative weights per level.  Every field carries a bitmap that equals its level's source mask, so its stream holds
the ocean cells only; the same integers are packed at 16 and at 12 bits per value.

One process, host to host, wall-clock ms, pageable input, masked epilogue with remap_area_min = 0.5; after a warm-up the
legs run interleaved step by step, in the order below on even steps and in the reverse order on odd ones (both orders of
the A/B; the medians of either order are reported beside the overall median and the best):
  grib16 / grib12   OperatorGroup.apply_host_grib on the 16-bit / 12-bit streams
  f32               (b) OperatorGroup.apply_host on the decoded float32 field alone (it packs the used cells on the host)
  parent road       (a) the numpy decode of every message (griblite, timed per level on its own and summed over the batch)
                    plus leg f32: what Regridder(packed=True) without packed_levels runs
and the bytes each ships over PCIe (smm_debug_host_stats).  Every raw result is compared bit for bit with the decoded
road's before anything is timed.  One JSON line, printed and appended to profiles/grib_levels_bench.jsonl.

  python tools/grib_levels_bench.py [--levels 16] [--nsteps 32] [--steps 8] [--warmup 2]
"""
import sys

import numpy as np

import benchlib
from bench_inputs import make_level_streams
from benchlib import same_bits as same


def bench(grp, masks, ml, n_steps, steps, warmup):
    from smmregrid_amd import _lib
    n_lev, S = masks.shape
    lev = np.arange(n_lev, dtype=np.int32)
    kw = dict(masked=True, remap_area_min=0.5)
    streams = {nbits: make_level_streams(masks, n_steps, nbits) for nbits in (16, 12)}
    print("# streams packed", file=sys.stderr, flush=True)
    legs = {}
    for nbits in (16, 12):
        buf, table, bitmaps, _, _ = streams[nbits]
        legs[f"grib{nbits}"] = lambda buf=buf, table=table, bitmaps=bitmaps: grp.apply_host_grib(buf, table, lev, ml,
                                                                                                bitmaps=bitmaps, **kw)
    field = streams[16][3]
    legs["f32"] = lambda: grp.apply_host(field, lev, ml, **kw)
    # bits first: each raw road against the decoded road on its own field
    for nbits in (16, 12):
        want = grp.apply_host(streams[nbits][3], lev, ml, **kw).copy()
        if not same(legs[f"grib{nbits}"](), want):
            raise SystemExit(f"apply_host_grib at {nbits} bits differs from apply_host on the decoded field")
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, both_orders=True, announce="# step {}")
    fwd, rev = benchlib.by_order(times, warmup)
    res = {"block": "host_to_host", "levels": int(n_lev), "nsteps": int(n_steps), "n_src": int(S), "n_dst": int(grp.n_dst),
           "steps": steps, "present_share": round(float((masks != 0).mean()), 4), **benchlib.summary(times, 3),
           "ms_fwd": benchlib.summary(fwd, 3)["ms"], "ms_rev": benchlib.summary(rev, 3)["ms"],
           "h2d_bytes": {k: int(s[0]["h2d_bytes"]) for k, s in stats.items()},
           "stages": {k: benchlib.stage_split(s) for k, s in stats.items()}, "bits_equal_parent": True}
    ms = res["ms"]
    for nbits in (16, 12):
        dec = benchlib.time_level_decode(streams[nbits][0], streams[nbits][4], S, max(5, steps)) * n_steps
        res[f"decode{nbits}_ms"] = round(dec, 1)                                   # every message of the variable, one thread
        res[f"parent_road{nbits}_ms"] = round(dec + ms["f32"], 1)                  # (a) decode + apply_host
        res[f"parent_over_grib{nbits}"] = round((dec + ms["f32"]) / ms[f"grib{nbits}"], 2)
        res[f"apply_host_f32_over_grib{nbits}"] = round(ms["f32"] / ms[f"grib{nbits}"], 3)      # (b): < 1 = the raw road loses
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=8, warmup=2, out="grib_levels_bench.jsonl", cfg_rows=False,
                         steps_help="timed repetitions (half in either order)")
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the variable")
    return ap


def main():
    args = benchlib.parse(parser(), least=6, both_orders=True,
                          why="an even number of at least 6 timed steps after an even warm-up: both orders get the same share")
    grp, masks, ml = benchlib.build_group(args.levels)
    print(f"# group built: {args.levels} levels, S = {grp.n_src}, D = {grp.n_dst}", file=sys.stderr, flush=True)
    benchlib.emit(bench(grp, masks, ml, args.nsteps, args.steps, args.warmup), args.out)


if __name__ == "__main__":
    main()
