"""CCSDS-packed GRIB-2 fields regridded raw (`apply_host_grib(ccsds=)`: smm_grib_aec_unpack ahead of the GRIB gather)
against the two roads the same data could take -- the same integers simple-packed through apply_host_grib, and a
one-thread host decode (smm_grib_aec_decode_host, as `GribField.decode` runs it) followed by apply_host on the float32
field -- on config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, bilinear) at B = 128 and on config-2 rows
(r1440x721 -> r360x180) at B = 512.  The fields are synthetic and smooth (a few waves plus noise of a few counts at 16
bits); the streams are written by the small encoder below (preprocessor on, J = 32, rsi = 128: what ecCodes asks of
libaec; split-sample and uncompressed options only) and decoded back by the library's host decoder before anything is timed.

One process, the legs interleaved step by step after a warm-up, median and best of >= 5:
  host    host to host, wall-clock ms, pageable input and output: the three roads, the bytes each ships to the device
  kernel  HBM-resident, device ms from HIP events: the transcode (`grib_unpack`: parse, inverse, store; its scratch is
          allocated and freed inside the call, which the figure includes) beside the gather it feeds (apply_grib on its output)
Every CCSDS result is compared bit for bit with the simple-packed road's.  One JSON line per block, printed and appended
to profiles/grib_ccsds_bench.jsonl.

  python tools/grib_ccsds_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 5] [--warmup 1] [--only cfg2,cfg4] [--blocks host,kernel]
                                   [--chunk-rows 0]    rows per chunk of the CCSDS leg (0: the entry's own sizing by bytes)
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

DISTINCT = 4        # distinct rows; the batch points at them in turn
NBITS, BLOCK, RSI = 16, 32, 128
FLAGS = 8 | 4 | 2   # AEC_DATA_PREPROCESS | AEC_DATA_MSB | AEC_DATA_3BYTE: ecCodes' ccsdsFlags


def _median(v):
    return float(np.median(np.asarray(v)))


def encode_ccsds(x, nbits=NBITS, J=BLOCK, rsi=RSI):
    """A CCSDS 121.0-B stream of the unsigned integers x with the preprocessor on, vectorised over blocks: per block
    the shortest of the split-sample options and the uncompressed one (no zero-block, no second extension -- a valid
    stream, not the shortest one).  Returns uint8 bytes."""
    x = np.asarray(x, dtype=np.int64)
    n = x.size
    pad = (-n) % J
    if pad:
        x = np.concatenate([x, np.full(pad, x[-1])])
    xmax = (1 << nbits) - 1
    idl = 5 if nbits > 16 else 4 if nbits > 8 else 3
    id_raw = (1 << idl) - 1
    prev = np.concatenate([x[:1], x[:-1]])
    delta, theta = x - prev, np.minimum(prev, xmax - prev)
    d = np.where((delta >= 0) & (delta <= theta), 2 * delta,
                 np.where((delta < 0) & (-delta <= theta), -2 * delta - 1, theta + np.abs(delta)))
    d = d.reshape(-1, J)
    nblk = d.shape[0]
    ref = (np.arange(nblk) % rsi) == 0
    refval = x.reshape(-1, J)[:, 0]
    d[ref, 0] = 0
    nc = J - ref.astype(np.int64)
    ks = np.arange(0, min(id_raw - 2, nbits - 1) + 1)
    lens = np.stack([(d >> k).sum(axis=1) + nc * (k + 1) for k in ks], axis=1)
    best = lens.argmin(axis=1)
    split_len = lens[np.arange(nblk), best]
    raw = split_len >= nc * nbits
    k = np.where(raw, 0, ks[best])
    ids = np.where(raw, id_raw, k + 1)
    body = np.where(raw, nc * nbits, split_len)
    head = idl + ref * nbits
    start = np.concatenate([[0], np.cumsum(head + body)])
    bits = np.zeros(int(start[-1]), dtype=np.uint8)
    start = start[:-1]
    for j in range(idl):
        bits[start + j] = (ids >> (idl - 1 - j)) & 1
    rb = np.flatnonzero(ref)
    for j in range(nbits):
        bits[start[rb] + idl + j] = (refval[rb] >> (nbits - 1 - j)) & 1
    at = start + head                                     # first bit of the coded part
    coded = np.ones_like(d, dtype=bool)
    coded[ref, 0] = False
    # split-sample: the terminating ones of the fundamental sequences, then the k-bit remainders
    sp = np.flatnonzero(~raw)
    q = (d[sp] >> k[sp, None]) + 1
    q[~coded[sp]] = 0
    ends = at[sp, None] + np.cumsum(q, axis=1) - 1
    bits[ends[coded[sp]]] = 1
    fs_len = q.sum(axis=1)
    slot = np.cumsum(coded[sp], axis=1) - 1                 # the sample's place among the coded ones
    for kk in np.unique(k[sp]):
        if kk == 0:
            continue
        m = k[sp] == kk
        rows_, pos = sp[m], (at[sp][m] + fs_len[m])[:, None] + slot[m] * kk
        for j in range(kk):
            bits[(pos + j)[coded[rows_]]] = ((d[rows_] >> (kk - 1 - j)) & 1)[coded[rows_]]
    # uncompressed: the coded samples as they are (the reference stands in front of them already)
    rw = np.flatnonzero(raw)
    slot_r = np.cumsum(coded[rw], axis=1) - 1
    for j in range(nbits):
        pos = at[rw, None] + slot_r * nbits + j
        bits[pos[coded[rw]]] = ((d[rw] >> (nbits - 1 - j)) & 1)[coded[rw]]
    return np.packbits(bits)


def smooth_field(S, i, rng):
    """16-bit integers of a smooth field: a few waves over the index, noise of a few counts."""
    t = np.arange(S) / S
    f = 32768 + 18000 * np.sin(2 * np.pi * (3 + i) * t) * np.cos(2 * np.pi * 41 * t) + 4000 * np.sin(2 * np.pi * 977 * t)
    return np.clip(np.rint(f + rng.normal(0.0, 3.0, S)), 0, 65535).astype(np.uint32)


def make_streams(S, rows, seed=20261019):
    """(coded buffer, row table, CCSDS records), (simple-packed buffer, row table), the float32 field, the distinct streams"""
    from smmregrid_amd import GRIB_AEC_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import aec_decode
    rng = np.random.default_rng(seed)
    E = -6
    coded, simple, dec, refs = [], [], [], []
    for i in range(DISTINCT):
        q = smooth_field(S, i, rng)
        stream = encode_ccsds(q)
        rec = np.array((0, stream.size, S, NBITS, BLOCK, RSI, FLAGS, 0), dtype=GRIB_AEC_DTYPE)
        if not np.array_equal(aec_decode(stream, rec), q):
            raise SystemExit("the tool's encoder wrote a stream the host decoder reads differently")
        coded.append(stream)
        simple.append(np.frombuffer(q.astype(">u2").tobytes(), dtype=np.uint8))
        refs.append(float(np.float32(220.0 + i)))
        dec.append(((refs[i] + q.astype(np.float64) * 2.0 ** E) / 1.0).astype(np.float32))

    def table(blocks):
        offs, pos = [], 117
        for b in blocks:
            offs.append(pos)
            pos += b.size + 117
        buf = np.zeros(pos, dtype=np.uint8)
        for o, b in zip(offs, blocks):
            buf[o:o + b.size] = b
        rows_t = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
        for r in range(rows):
            rows_t[r] = (offs[r % DISTINCT], refs[r % DISTINCT], 2.0 ** E, 1.0, NBITS, 0)
        return buf, rows_t, offs
    cbuf, crows, coffs = table(coded)
    aec = np.zeros(rows, dtype=GRIB_AEC_DTYPE)
    for r in range(rows):
        aec[r] = (coffs[r % DISTINCT], coded[r % DISTINCT].size, S, NBITS, BLOCK, RSI, FLAGS, 0)
    sbuf, srows, _ = table(simple)
    field = np.ascontiguousarray(np.stack([dec[r % DISTINCT] for r in range(rows)]))
    return (cbuf, crows, aec), (sbuf, srows), field, coded, refs, E


def bench_host(op, name, rows, steps, warmup, chunk_rows=0):
    from smmregrid_amd import GRIB_AEC_DTYPE, _lib
    from smmregrid_amd.griblite import aec_decode
    S, D_ = op.n_src, op.n_dst
    (cbuf, crows, aec), (sbuf, srows), field, coded, refs, E = make_streams(S, rows)
    print(f"# {name}: streams written, {coded[0].size / (2.0 * S):.3f} of the simple-packed bytes", file=sys.stderr, flush=True)
    y_c, y_o = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)      # the CCSDS road's, the other roads'
    legs = {"ccsds16": lambda: op.apply_host_grib(cbuf, crows, ccsds=aec, out=y_c, chunk_rows=chunk_rows),
            "grib16": lambda: op.apply_host_grib(sbuf, srows, out=y_o),
            "f32": lambda: op.apply_host(field, out=y_o)}
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
            if step == 0 and leg != "ccsds16" and not np.array_equal(y_c.view(np.uint64), y_o.view(np.uint64)):
                raise SystemExit(f"{name}: the CCSDS road differs from the {'simple-packed' if leg == 'grib16' else 'decoded'} road")
    rec = np.array((0, coded[0].size, S, NBITS, BLOCK, RSI, FLAGS, 0), dtype=GRIB_AEC_DTYPE)
    row, dec = np.empty(S, np.float32), []
    for _ in range(max(5, steps)):
        t0 = time.perf_counter()
        row[:] = (refs[0] + aec_decode(coded[0], rec).astype(np.float64) * 2.0 ** E) / 1.0
        dec.append((time.perf_counter() - t0) * 1e3)
    ms = {k: round(_median(v), 3) for k, v in times.items()}
    staged = int(sum((int(n) + 3) // 4 * 4 for n in aec["byte_len"]))
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
           "ccsds_chunk_rows": chunk_rows, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "h2d_bytes": {"ccsds16": staged, "grib16": int(stats["grib16"]["h2d_bytes"]), "f32": int(stats["f32"]["h2d_bytes"])},
           "ccsds_over_simple_bytes": round(coded[0].size / (2.0 * S), 4),
           "host_decode_ms_per_row": {"median": round(_median(dec), 3), "min": round(min(dec), 3)},
           "bits_equal_simple_packed": True}
    res["decoded_road_ms"] = round(_median(dec) * rows + ms["f32"], 1)       # one-thread decode of every row + apply_host
    res["grib16_over_ccsds16"] = round(ms["grib16"] / ms["ccsds16"], 3)
    res["decoded_road_over_ccsds16"] = round(res["decoded_road_ms"] / ms["ccsds16"], 2)
    return res


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, grib_unpack, to_device
    from smmregrid_amd.device import Event
    S, D_ = op.n_src, op.n_dst
    rows = min(rows, 16)                                   # 4 B of scratch per sample: a chunk's worth of rows
    (cbuf, crows, aec), (sbuf, srows), _, _, _, _ = make_streams(S, rows)

    def dev(buf):
        padded = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
        padded[:buf.size] = buf
        return to_device(padded)
    dc, ds = dev(cbuf), dev(sbuf)
    out = DeviceArray(((2 * S + 3) // 4 * 4 * rows,), np.uint8)
    y, y_s = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
    _, rows_out = grib_unpack(dc, crows, aec, x_bytes=cbuf.size, out=out)
    legs = {"transcode": lambda: grib_unpack(dc, crows, aec, x_bytes=cbuf.size, out=out),
            "gather_of_transcoded": lambda: op.apply_grib(out, rows_out, y=y),
            "gather_of_simple": lambda: op.apply_grib(ds, srows, x_bytes=sbuf.size, y=y_s)}
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
        if step == 0 and not np.array_equal(y.rows(0, 2).to_host().view(np.uint64), y_s.rows(0, 2).to_host().view(np.uint64)):
            raise SystemExit(f"{name}: the gather of the transcoded streams differs from the gather of the simple-packed ones")
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    return {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
            "ms_min": {k: round(min(v), 4) for k, v in times.items()},
            "transcode_over_gather": round(ms["transcode"] / ms["gather_of_transcoded"], 3),
            "coded_bytes": int(aec["byte_len"].sum()), "bits_equal_simple_packed": True}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="host,kernel")
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_ccsds_bench.jsonl"))
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
            res = bench_host(op, name, rows, args.steps, args.warmup, args.chunk_rows) if block == "host" else \
                bench_kernel(op, name, rows, args.steps, args.warmup)
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        op.close()


if __name__ == "__main__":
    main()
