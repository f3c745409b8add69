"""GRIB simple-packed fields regridded raw (smm_apply_grib / smm_apply_host_grib) against the road such data took
before -- decode every message in numpy (griblite), then regrid the float32 field -- on config-4 geometry (regular
Gaussian n1280 -> HEALPix 1024, bilinear: nearly every source cell is used, the host pack does not apply) at B = 128
and on config-2 rows (r1440x721 -> r360x180).  The same integers are packed at 16 and at 12 bits per value.

One process, the legs interleaved step by step after a warm-up, median and best of >= 5:
  host    (a) host to host, wall-clock ms, pageable input and output: apply_host_grib on the 16-bit and the 12-bit
          streams; the parent road = griblite's numpy decode of one message (timed on its own, per row, and scaled to
          the batch) followed by apply_host on the float32 field; the bytes each ships (smm_debug_host_stats)
  kernel  (b) HBM-resident, device ms from HIP events: smm_apply_grib without and with the f64 division (D = 0 / D = 1)
          against smm_apply with SMM_F32 X and SMM_APPLY_KERNEL_SELL on the decoded field
  open    (c) file to result on config-2 geometry: a GRIB-1 file of --open-rows 16-bit messages (written with the test
          suite's encoder) through io.open_dataset + apply_host (the parent road: open_grib decodes every message) against
          open_dataset(decode=False) + apply_host_grib (nothing is unpacked on the host), wall-clock ms, with the open alone
Every grib result is compared bit for bit with the parent road's before anything is timed.  One JSON line per block,
printed and appended to profiles/grib_bench.jsonl.

  python tools/grib_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 7] [--warmup 2] [--only cfg2,cfg4] [--blocks host,kernel,open]
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

DISTINCT = 4        # distinct rows; the batch tiles them


def _median(v):
    return float(np.median(np.asarray(v)))


def pack16(q):
    return q.astype(">u2").tobytes()


def pack12(q):
    """Two 12-bit values in three bytes, big-endian bit order (q.size even)."""
    a, b = q[0::2].astype(np.uint16), q[1::2].astype(np.uint16)
    out = np.empty((a.size, 3), dtype=np.uint8)
    out[:, 0] = a >> 4
    out[:, 1] = ((a & 15) << 4) | (b >> 8)
    out[:, 2] = b & 255
    return out.tobytes()


def make_streams(S, rows, D, widths=(16, 12), seed=20261018):
    """The packed streams of `rows` fields of S values at 16 and at 12 bits -- message after message with a gap of 117
    bytes between them, as sections 0 - 3 would leave -- their row tables, and the float32 field griblite decodes from
    them (the parent road's input)."""
    from smmregrid_amd import GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import _unpack_bits
    assert S % 2 == 0
    rng = np.random.default_rng(seed)
    out = {}
    for nbits, pack in ((16, pack16), (12, pack12)):
        if nbits not in widths:
            continue
        blocks, refs = [], []
        for i in range(DISTINCT):
            q = rng.integers(0, 1 << nbits, size=S, dtype=np.uint32)
            blocks.append(pack(q))
            refs.append(float(np.float32(220.0 + i)))
        E = -6 if nbits == 16 else -2          # ~ 0.016 K / 0.25 K steps over a 1000-K span
        table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
        pieces, pos = [], 0
        for b in range(rows):
            pieces.append(bytes(117))
            pos += 117
            table[b] = (pos, refs[b % DISTINCT], 2.0 ** E, 10.0 ** D, nbits, 0)
            pieces.append(blocks[b % DISTINCT])
            pos += len(blocks[b % DISTINCT])
        buf = np.frombuffer(b"".join(pieces), dtype=np.uint8)
        dec = np.empty((DISTINCT, S), dtype=np.float32)
        for i in range(DISTINCT):
            dec[i] = (refs[i] + _unpack_bits(blocks[i], nbits, S) * 2.0 ** E) / 10.0 ** D
        field = np.ascontiguousarray(np.tile(dec, ((rows + DISTINCT - 1) // DISTINCT, 1))[:rows])
        out[nbits] = (buf, table, field, blocks[0], refs[0], E)
    return out


def time_decode(block, nbits, S, ref, E, D, steps):
    """griblite's decode of one message, as open_grib runs it: unpack, the float64 statement, the float32 store."""
    from smmregrid_amd.griblite import _unpack_bits
    row = np.empty(S, dtype=np.float32)
    times = []
    for _ in range(steps):
        t0 = time.perf_counter()
        row[:] = (ref + _unpack_bits(block, nbits, S) * 2.0 ** E) / 10.0 ** D
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def bench_host(op, name, rows, steps, warmup):
    from smmregrid_amd import _lib
    S, D_ = op.n_src, op.n_dst
    streams = make_streams(S, rows, 0)
    print(f"# {name}: streams packed", file=sys.stderr, flush=True)
    y_raw, y_f32 = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)
    legs = {"grib16": lambda: op.apply_host_grib(streams[16][0], streams[16][1], out=y_raw),
            "f32_of_16": lambda: op.apply_host(streams[16][2], out=y_f32),
            "grib12": lambda: op.apply_host_grib(streams[12][0], streams[12][1], out=y_raw),
            "f32_of_12": lambda: op.apply_host(streams[12][2], out=y_f32)}
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
            if step == 0 and leg.startswith("f32_of_"):      # the raw leg of the same width ran just before
                if not np.array_equal(y_raw.view(np.uint64), y_f32.view(np.uint64)):
                    raise SystemExit(f"{name}: apply_host_grib at {leg[7:]} bits differs from the parent road")
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           "ms": {k: round(_median(v), 3) for k, v in times.items()},
           "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "h2d_bytes": {k: int(s["h2d_bytes"]) for k, s in stats.items()},
           "d2h_bytes": {k: int(s["d2h_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s["chunks"]) for k, s in stats.items()}, "bits_equal_parent": True}
    for nbits in (16, 12):
        _, _, _, block, ref, E = streams[nbits]
        dec = time_decode(block, nbits, S, ref, E, 0, max(5, steps))
        res[f"decode{nbits}_ms_per_row"] = {"median": round(_median(dec), 3), "min": round(min(dec), 3)}
        parent = _median(dec) * rows + res["ms"][f"f32_of_{nbits}"]
        res[f"parent_road{nbits}_ms"] = round(parent, 1)          # decode of every row (one thread, as today) + apply_host
        res[f"parent_over_grib{nbits}"] = round(parent / res["ms"][f"grib{nbits}"], 2)
        res[f"apply_host_f32_over_grib{nbits}"] = round(res["ms"][f"f32_of_{nbits}"] / res["ms"][f"grib{nbits}"], 3)
    return res


def bench_open(op, name, rows, steps, warmup):
    """File to result: what a user of io.open_dataset pays on either road (r1440x721 lon/lat messages at 16 bits)."""
    import tempfile
    from smmregrid_amd.io import open_dataset
    from tests.test_griblite import encode
    ni, nj = 1440, 721
    assert op.n_src == ni * nj
    rng = np.random.default_rng(20261018)
    base = 250.0 + 30.0 * rng.standard_normal((nj, ni))
    msgs = [encode(base + day, 0, ni, nj, 90, 0, -90, 359.75, 250, param=167, date=(2021, 1 + day // 28, 1 + day % 28, 12),
                   nbits=16) for day in range(rows)]
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "t2m.grib")
    with open(path, "wb") as f:
        f.write(b"".join(msgs))
    print(f"# {name}: GRIB file of {rows} messages written", file=sys.stderr, flush=True)
    y_raw, y_f32 = np.empty((rows, op.n_dst), np.float64), np.empty((rows, op.n_dst), np.float64)
    times = {k: [] for k in ("open_decoded", "apply_host_f32", "open_raw", "apply_host_grib")}
    for step in range(warmup + steps):
        t0 = time.perf_counter()
        field = open_dataset(path)["t2m"].data
        t1 = time.perf_counter()
        op.apply_host(field.reshape(rows, -1), out=y_f32)
        t2 = time.perf_counter()
        raw = open_dataset(path, decode=False)["t2m"].data
        t3 = time.perf_counter()
        op.apply_host_grib(raw.buf, raw.rows, out=y_raw)
        t4 = time.perf_counter()
        if step == 0 and not np.array_equal(y_raw.view(np.uint64), y_f32.view(np.uint64)):
            raise SystemExit(f"{name}: the raw road differs from the parent road on the file")
        if step >= warmup:
            for k, dt in zip(times, (t1 - t0, t2 - t1, t3 - t2, t4 - t3)):
                times[k].append(dt * 1e3)
    os.remove(path)
    os.rmdir(tmp)
    ms = {k: round(_median(v), 3) for k, v in times.items()}
    parent, rawroad = ms["open_decoded"] + ms["apply_host_f32"], ms["open_raw"] + ms["apply_host_grib"]
    return {"block": "file_to_result", "op": name, "rows": rows, "n_src": op.n_src, "n_dst": op.n_dst, "steps": steps,
            "nbits": 16, "ms": ms, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
            "parent_road_ms": round(parent, 3), "raw_road_ms": round(rawroad, 3),
            "parent_over_raw": round(parent / rawroad, 2), "bits_equal_parent": True}


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    from smmregrid_amd.device import Event
    S, D_ = op.n_src, op.n_dst
    legs, check = {}, {}
    y_div = DeviceArray((rows, D_), np.float64)                 # the legs with the division share one result
    for nbits in (16, 12):
        buf, table, field, *_ = make_streams(S, rows, 0, widths=(nbits,))[nbits]
        padded = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
        padded[:buf.size] = buf
        dx, y = to_device(padded), DeviceArray((rows, D_), np.float64)
        table_div = table.copy()
        table_div["ddiv"] = 10.0                                # the same bits with D = 1
        legs[f"grib{nbits}_nodiv"] = lambda dx=dx, y=y, table=table, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y)
        legs[f"grib{nbits}_div"] = lambda dx=dx, table=table_div, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y_div)
        dfield, y32 = to_device(field), DeviceArray((rows, D_), np.float64)
        legs[f"f32_sell_of_{nbits}"] = lambda dfield=dfield, y32=y32: op.apply(dfield, y=y32, flags=_lib.APPLY_KERNEL_SELL)
        check[nbits] = (y, y32)
        del buf, field, padded
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
                if not np.array_equal(y.rows(0, 2).to_host().view(np.uint64), y32.rows(0, 2).to_host().view(np.uint64)):
                    raise SystemExit(f"{name}: smm_apply_grib at {nbits} bits differs from smm_apply on the decoded field")
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    res = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
           "ms_min": {k: round(min(v), 4) for k, v in times.items()}, "bits_equal_parent": True}
    res["over_f32_sell"] = {k: round(ms[k] / ms[f"f32_sell_of_{k[4:6]}"], 3) for k in ms if k.startswith("grib")}
    return res


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--open-rows", type=int, default=16)
    ap.add_argument("--blocks", default="host,kernel,open")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_bench.jsonl"))
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
            if block == "open":
                if name != "cfg2":          # the file's messages are r1440x721 lon/lat fields
                    continue
                res = bench_open(op, name, args.open_rows, args.steps, args.warmup)
            else:
                res = (bench_host if block == "host" else bench_kernel)(op, name, rows, args.steps, args.warmup)
            res["used_src_share"] = round(op.n_used_src / op.n_src, 4)
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        op.close()


if __name__ == "__main__":
    main()
