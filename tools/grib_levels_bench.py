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
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.grib_bench import DISTINCT, _median, pack12, pack16      # noqa: E402
from tools.packed_levels_bench import build_group                    # noqa: E402

STAGES = ("stage_in_ms", "h2d_ms", "kernel_ms", "d2h_ms", "copy_out_ms", "wait_ms", "chunks")


def make_level_streams(masks, n_steps, nbits, seed=20261019):
    """The buffer -- message after message in (step, level) order: a gap of 117 bytes, the level's bitmap, a gap of 11,
    the packed values of its present cells -- the row table and the bitmap records shaped (n_steps, n_lev, 1), the float32
    field (n_steps, n_lev, 1, S) griblite decodes from it (DISTINCT distinct steps, tiled) and the rule and bitmap of
    each level's first message for the decode timing."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _decode_rule
    rng = np.random.default_rng(seed)
    n_lev, S = masks.shape
    pack, E = (pack16, -6) if nbits == 16 else (pack12, -2)
    present = [masks[l] != 0 for l in range(n_lev)]
    bmbytes = [np.packbits(m.astype(np.uint8)).tobytes() for m in present]
    # pack12 writes pairs: an odd count gets one value more, which no row's n_values reaches
    blocks = [[pack(rng.integers(0, 1 << nbits, size=int(m.sum()) + int(m.sum()) % 2, dtype=np.uint32)) for m in present]
              for _ in range(DISTINCT)]
    table = np.zeros((n_steps, n_lev, 1), dtype=GRIB_ROW_DTYPE)
    bitmaps = np.zeros((n_steps, n_lev, 1), dtype=GRIB_BITMAP_DTYPE)
    pieces, pos = [], 0
    for t in range(n_steps):
        for l in range(n_lev):
            pieces.append(bytes(117))
            pos += 117
            bitmaps[t, l, 0] = (pos, int(present[l].sum()))
            pieces.append(bmbytes[l])
            pos += len(bmbytes[l])
            pieces.append(bytes(11))
            pos += 11
            table[t, l, 0] = (pos, float(np.float32(220.0 + l + t % DISTINCT)), 2.0 ** E, 1.0, nbits, 0)
            pieces.append(blocks[t % DISTINCT][l])
            pos += len(blocks[t % DISTINCT][l])
    buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
    del pieces
    rule = lambda t, l: (int(table[t, l, 0]["byte_off"]), float(table[t, l, 0]["ref"]), float(table[t, l, 0]["bscale"]), 1.0, nbits)  # noqa: E731
    bm = lambda t, l: (int(bitmaps[t, l, 0]["bitmap_off"]), int(bitmaps[t, l, 0]["n_values"]))                                       # noqa: E731
    dec = np.empty((min(DISTINCT, n_steps), n_lev, 1, S), dtype=np.float32)
    for t in range(dec.shape[0]):
        for l in range(n_lev):
            dec[t, l, 0] = _decode_rule(buf, rule(t, l), S, bm(t, l))
    field = np.ascontiguousarray(np.tile(dec, ((n_steps + DISTINCT - 1) // DISTINCT, 1, 1, 1))[:n_steps])
    return buf, table, bitmaps, field, [(rule(0, l), bm(0, l)) for l in range(n_lev)]


def time_decode(buf, first, S, steps):
    """griblite's decode of one bitmapped message per level, as open_grib runs it, with the float32 store: the median
    per level, summed over the levels = one time step of the variable"""
    from smmregrid_amd.griblite import _decode_rule
    row = np.empty(S, dtype=np.float32)
    total = 0.0
    for rule, bm in first:
        times = []
        for _ in range(steps):
            t0 = time.perf_counter()
            row[:] = _decode_rule(buf, rule, S, bm)
            times.append((time.perf_counter() - t0) * 1e3)
        total += _median(times)
    return total


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


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
    names = list(legs)
    times = {k: {"fwd": [], "rev": []} for k in legs}
    stats = {k: [] for k in legs}
    for step in range(warmup + steps):
        print(f"# step {step}", file=sys.stderr, flush=True)
        order = "fwd" if step % 2 == 0 else "rev"
        for leg in (names if order == "fwd" else names[::-1]):
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            legs[leg]()
            dt = (time.perf_counter() - t0) * 1e3
            st = _lib.host_stats(reset=True)
            if step >= warmup:
                times[leg][order].append(dt)
                stats[leg].append(st)
    both = {k: v["fwd"] + v["rev"] for k, v in times.items()}
    res = {"block": "host_to_host", "levels": int(n_lev), "nsteps": int(n_steps), "n_src": int(S), "n_dst": int(grp.n_dst),
           "steps": steps, "present_share": round(float((masks != 0).mean()), 4),
           "ms": {k: round(_median(v), 3) for k, v in both.items()},
           "ms_min": {k: round(min(v), 3) for k, v in both.items()},
           "ms_fwd": {k: round(_median(v["fwd"]), 3) for k, v in times.items()},
           "ms_rev": {k: round(_median(v["rev"]), 3) for k, v in times.items()},
           "h2d_bytes": {k: int(s[0]["h2d_bytes"]) for k, s in stats.items()},
           "stages": {k: {n: round(_median([st[n] for st in s]), 3) for n in STAGES} for k, s in stats.items()},
           "bits_equal_parent": True}
    ms = res["ms"]
    for nbits in (16, 12):
        dec = time_decode(streams[nbits][0], streams[nbits][4], S, max(5, steps)) * n_steps
        res[f"decode{nbits}_ms"] = round(dec, 1)                                   # every message of the variable, one thread
        res[f"parent_road{nbits}_ms"] = round(dec + ms["f32"], 1)                  # (a) decode + apply_host
        res[f"parent_over_grib{nbits}"] = round((dec + ms["f32"]) / ms[f"grib{nbits}"], 2)
        res[f"apply_host_f32_over_grib{nbits}"] = round(ms["f32"] / ms[f"grib{nbits}"], 3)      # (b): < 1 = the raw road loses
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--levels", type=int, default=16)
    ap.add_argument("--nsteps", type=int, default=32, help="time steps of the variable")
    ap.add_argument("--steps", type=int, default=8, help="timed repetitions (half in either order)")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_levels_bench.jsonl"))
    args = ap.parse_args()
    if args.steps < 6 or args.steps % 2 or args.warmup % 2:
        ap.error("an even number of at least 6 timed steps after an even warm-up: both orders get the same share")
    grp, masks, ml = build_group(args.levels)
    print(f"# group built: {args.levels} levels, S = {grp.n_src}, D = {grp.n_dst}", file=sys.stderr, flush=True)
    res = bench(grp, masks, ml, args.nsteps, args.steps, args.warmup)
    print(json.dumps(res), flush=True)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a") as f:
        f.write(json.dumps(res) + "\n")


if __name__ == "__main__":
    main()
