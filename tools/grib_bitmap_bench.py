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
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.grib_bench import DISTINCT, _median, make_streams, pack12, pack16      # noqa: E402

MISSING = 0.3


def make_bitmap_streams(S, rows, widths=(16, 12), seed=20261019):
    """Per width: the buffer -- message after message: a gap of 117 bytes, the bitmap, a gap of 11, the packed present
    values -- the row table, the bitmap records, the float32 field griblite decodes (NaN where the bitmap is 0), and the
    rule and bitmap of message 0 for the decode timing."""
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _decode_rule
    rng = np.random.default_rng(seed)
    masks = []
    for i in range(DISTINCT):
        m = rng.random(S) >= MISSING
        if m.sum() % 2:                       # pack12 writes pairs
            m[np.flatnonzero(~m)[0]] = True
        masks.append(m)
    out = {}
    for nbits, pack in ((16, pack16), (12, pack12)):
        if nbits not in widths:
            continue
        E = -6 if nbits == 16 else -2
        blocks = [pack(rng.integers(0, 1 << nbits, size=int(m.sum()), dtype=np.uint32)) for m in masks]
        bmbytes = [np.packbits(m.astype(np.uint8)).tobytes() for m in masks]
        refs = [float(np.float32(220.0 + i)) for i in range(DISTINCT)]
        table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
        bitmaps = np.zeros(rows, dtype=GRIB_BITMAP_DTYPE)
        pieces, pos = [], 0
        for b in range(rows):
            i = b % DISTINCT
            pieces.append(bytes(117))
            pos += 117
            bitmaps[b] = (pos, int(masks[i].sum()))
            pieces.append(bmbytes[i])
            pos += len(bmbytes[i])
            pieces.append(bytes(11))
            pos += 11
            table[b] = (pos, refs[i], 2.0 ** E, 1.0, nbits, 0)
            pieces.append(blocks[i])
            pos += len(blocks[i])
        buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        del pieces
        rule = lambda b: (int(table[b]["byte_off"]), float(table[b]["ref"]), float(table[b]["bscale"]), 1.0, nbits)   # noqa: E731
        bm = lambda b: (int(bitmaps[b]["bitmap_off"]), int(bitmaps[b]["n_values"]))                                  # noqa: E731
        dec = np.empty((DISTINCT, S), dtype=np.float32)
        for i in range(DISTINCT):
            dec[i] = _decode_rule(buf, rule(i), S, bm(i))
        field = np.ascontiguousarray(np.tile(dec, ((rows + DISTINCT - 1) // DISTINCT, 1))[:rows])
        out[nbits] = (buf, table, bitmaps, field, rule(0), bm(0))
    return out


def time_decode(buf, rule, bm, S, steps):
    """griblite's decode of one bitmapped message, as open_grib runs it, with the float32 store"""
    from smmregrid_amd.griblite import _decode_rule
    row = np.empty(S, dtype=np.float32)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        row[:] = _decode_rule(buf, rule, S, bm)
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def same(a, b):
    return np.array_equal(np.asarray(a).view(np.uint64), np.asarray(b).view(np.uint64))


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
    times, stats = {k: [] for k in legs}, {}
    for step in range(warmup + steps):
        print(f"# {name}: host step {step}", file=sys.stderr, flush=True)
        for leg, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            stats[leg] = _lib.host_stats(reset=True)
            if step >= warmup:
                times[leg].append(dt)
            if step == 0 and leg.startswith("f32_of_") and not same(y_raw, y_f32):      # the raw leg ran just before
                raise SystemExit(f"{name}: apply_host_grib(bitmaps=) at {leg[7:]} bits differs from the decoded road")
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "h2d_bytes": {k: int(s["h2d_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s["chunks"]) for k, s in stats.items()}, "bits_equal_parent": True}
    for nbits in (16, 12):
        buf, _, _, _, rule, bm = streams[nbits]
        dec = time_decode(buf, rule, bm, S, max(5, steps))
        res[f"decode{nbits}_ms_per_row"] = {"median": round(_median(dec), 3), "min": round(min(dec), 3)}
        parent = _median(dec) * rows + res["ms"][f"f32_of_{nbits}"]
        res[f"parent_road{nbits}_ms"] = round(parent, 1)          # decode of every row (one thread) + apply_host
        res[f"parent_over_gribbm{nbits}"] = round(parent / res["ms"][f"gribbm{nbits}"], 2)
        res[f"apply_host_f32_over_gribbm{nbits}"] = round(res["ms"][f"f32_of_{nbits}"] / res["ms"][f"gribbm{nbits}"], 3)
    return res


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, SparseOperator, _lib, to_device
    from smmregrid_amd.device import Event
    S, D_ = op.n_src, op.n_dst
    one = SparseOperator(S, 1, np.array([1]), np.array([1]), np.array([1.0]), device=0)     # the build, next to no gather
    legs, check = {}, {}
    y_one = DeviceArray((rows, 1), np.float64)
    for nbits in (16, 12):
        buf, table, bitmaps, field, _, _ = make_bitmap_streams(S, rows, widths=(nbits,))[nbits]
        padded = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
        padded[:buf.size] = buf
        dx, y = to_device(padded), DeviceArray((rows, D_), np.float64)
        legs[f"gribbm{nbits}_total"] = lambda dx=dx, y=y, t=table, b=bitmaps, n=buf.size: op.apply_grib(dx, t, x_bytes=n, y=y,
                                                                                                     bitmaps=b)
        legs[f"gribbm{nbits}_build"] = lambda dx=dx, t=table, b=bitmaps, n=buf.size: one.apply_grib(dx, t, x_bytes=n, y=y_one,
                                                                                                  bitmaps=b)
        dfield, y32 = to_device(field), DeviceArray((rows, D_), np.float64)
        legs[f"f32_sell_of_{nbits}"] = lambda dfield=dfield, y32=y32: op.apply(dfield, y=y32, flags=_lib.APPLY_KERNEL_SELL)
        check[nbits] = (y, y32)
        del buf, field, padded
        fbuf, ftable, *_ = make_streams(S, rows, 0, widths=(nbits,))[nbits]            # a full field, no bitmap
        fpad = np.zeros((fbuf.size + 3) // 4 * 4, np.uint8)
        fpad[:fbuf.size] = fbuf
        fx, fy = to_device(fpad), DeviceArray((rows, D_), np.float64)
        legs[f"grib{nbits}_full"] = lambda fx=fx, fy=fy, t=ftable, n=fbuf.size: op.apply_grib(fx, t, x_bytes=n, y=fy)
        del fbuf, fpad
    e0, e1 = Event(), Event()
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        for leg, fn in legs.items():
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            if step >= warmup:
                times[leg].append(e0.elapsed_ms(e1))
        if step == 0:
            for nbits, (y, y32) in check.items():
                if not same(y.to_host(), y32.to_host()):
                    raise SystemExit(f"{name}: smm_apply_grib_bm at {nbits} bits differs from smm_apply on the decoded field")
    one.close()
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    res = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING, "ms": ms,
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}, "bits_equal_parent": True}
    for nbits in (16, 12):
        gather = ms[f"gribbm{nbits}_total"] - ms[f"gribbm{nbits}_build"]
        res[f"gribbm{nbits}_gather_ms"] = round(gather, 4)                        # total - build
        res[f"gribbm{nbits}_gather_over_grib_full"] = round(gather / ms[f"grib{nbits}_full"], 3)
        res[f"gribbm{nbits}_total_over_grib_full"] = round(ms[f"gribbm{nbits}_total"] / ms[f"grib{nbits}_full"], 3)
        res[f"gribbm{nbits}_total_over_f32_sell"] = round(ms[f"gribbm{nbits}_total"] / ms[f"f32_sell_of_{nbits}"], 3)
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="host,kernel")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_bitmap_bench.jsonl"))
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
