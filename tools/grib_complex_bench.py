"""Complex-packed GRIB-2 fields (templates 5.2 / 5.3) regridded raw (`apply_host_grib(cpx=)`: smm_grib_cpx_unpack ahead
of the GRIB gather) against the two roads the same data could take -- the same integers simple-packed through
apply_host_grib, and a one-thread host decode (smm_grib_cpx_decode_host, as `GribField.decode` runs it) followed by
apply_host on the float32 field -- on config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, bilinear) at B = 128 and
on config-2 rows (r1440x721 -> r360x180) at B = 512.  The fields are synthetic and smooth (a few waves plus noise of a few
counts at 16 bits); the streams are written by the small encoder below (order 2, three octets per descriptor, groups of a
fixed 32 values, each with its own minimal width: a valid stream, not the grouping an NCEP encoder would search for) and
decoded back by the library's host decoder before anything is timed.

One process, the legs interleaved step by step after a warm-up, median and best of >= 5:
  host    host to host, wall-clock ms, pageable input and output: the three roads
  kernel  HBM-resident, device ms from HIP events: the transcode (`grib_unpack_cpx`; its scratch is allocated and freed
          inside the call, which the figure includes) beside the gather it feeds (apply_grib on its output), the gather of
          the simple-packed twin, and `grib_pack` at 16 bits of float64 rows of the same length (at most 32 of them;
          compared per row)
  --profile-run  the transcode alone, a few times, nothing written: what `rocprofv3 --kernel-trace --stats -- python
          tools/grib_complex_bench.py --profile-run --only cfg2` is pointed at for the split over the kernels
Every result of the complex-packed road is compared bit for bit with the simple-packed road's before anything is timed.
One JSON line per block, printed and appended to profiles/grib_complex_bench.jsonl.

  python tools/grib_complex_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 5] [--warmup 1] [--only cfg2,cfg4]
                                     [--blocks host,kernel] [--chunk-rows 0] [--profile-run]
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
NBITS, GROUP, N_OCT = 16, 32, 3


def _median(v):
    return float(np.median(np.asarray(v)))


def _bit_length(v):
    """bit lengths of non-negative integers below 2^53"""
    return np.where(v > 0, np.frexp(np.maximum(v, 1).astype(np.float64))[1], 0).astype(np.int64)


def _pack(values, widths):
    """values[i] in widths[i] bits, big-endian, back to back, padded to an octet"""
    start = np.cumsum(widths) - widths
    bits = np.zeros(int(widths.sum()), dtype=np.uint8)
    for b in range(int(widths.max()) if widths.size else 0):
        sel = np.flatnonzero(widths > b)
        bits[start[sel] + b] = (values[sel] >> (widths[sel] - 1 - b)) & 1
    return np.packbits(bits)


def _sm(v, n_oct):
    return (abs(int(v)) | ((1 << (8 * n_oct - 1)) if v < 0 else 0)).to_bytes(n_oct, "big")


def encode_complex(q, group=GROUP, n_oct=N_OCT):
    """(stream, the fields of a GRIB_CPX_DTYPE record from n_groups to n_oct) for the unsigned integers q: template 5.3,
    order 2, groups of `group` values (the last one shorter), every group with its own minimal width."""
    x = np.asarray(q, dtype=np.int64)
    n = x.size
    d = np.zeros(n, dtype=np.int64)
    d[2:] = x[2:] - 2 * x[1:-1] + x[:-2]
    g = int(d[2:].min())
    z = d - g
    z[:2] = 0
    ng = (n + group - 1) // group
    zz = np.concatenate([z, np.full(ng * group - n, z[-1])]).reshape(ng, group)
    ref = zz.min(axis=1)
    w = _bit_length(zz.max(axis=1) - ref)
    nbits, width_ref = int(_bit_length(ref.max())), int(w.min())
    width_bits = int(_bit_length(w.max() - width_ref))
    stream = _sm(x[0], n_oct) + _sm(x[1], n_oct) + _sm(g, n_oct) + _pack(ref, np.full(ng, nbits)).tobytes() + \
        _pack(w - width_ref, np.full(ng, width_bits)).tobytes() + _pack((zz - ref[:, None]).ravel()[:n], np.repeat(w, group)[:n]).tobytes()
    return np.frombuffer(stream, dtype=np.uint8), (ng, nbits, width_ref, width_bits, group, 1, n - (ng - 1) * group, 0, 2, n_oct)


def smooth_field(S, i, rng):
    """16-bit integers of a smooth field: a few waves over the index, noise of a few counts."""
    t = np.arange(S) / S
    f = 32768 + 18000 * np.sin(2 * np.pi * (3 + i) * t) * np.cos(2 * np.pi * 41 * t) + 4000 * np.sin(2 * np.pi * 977 * t)
    return np.clip(np.rint(f + rng.normal(0.0, 3.0, S)), 0, 65535).astype(np.uint32)


def make_streams(S, rows, seed=20261020):
    """(coded buffer, row table, complex-packing records), (simple-packed buffer, row table), the float32 field, the
    distinct streams and their records"""
    from smmregrid_amd import GRIB_CPX_DTYPE, GRIB_ROW_DTYPE
    from smmregrid_amd.griblite import cpx_decode
    rng = np.random.default_rng(seed)
    E = -6
    coded, params, simple, dec, refs = [], [], [], [], []
    for i in range(DISTINCT):
        q = smooth_field(S, i, rng)
        stream, p = encode_complex(q)
        rec = np.array((0, stream.size, S) + p + (0,), dtype=GRIB_CPX_DTYPE)
        if not np.array_equal(cpx_decode(stream, rec), q):
            raise SystemExit("the tool's encoder wrote a stream the host decoder reads differently")
        coded.append(stream)
        params.append(p)
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
    cpx = np.zeros(rows, dtype=GRIB_CPX_DTYPE)
    for r in range(rows):
        cpx[r] = (coffs[r % DISTINCT], coded[r % DISTINCT].size, S) + params[r % DISTINCT] + (0,)
    sbuf, srows, _ = table(simple)
    field = np.ascontiguousarray(np.stack([dec[r % DISTINCT] for r in range(rows)]))
    return (cbuf, crows, cpx), (sbuf, srows), field, coded, params, refs, E


def bench_host(op, name, rows, steps, warmup, chunk_rows=0):
    from smmregrid_amd import GRIB_CPX_DTYPE
    from smmregrid_amd.griblite import cpx_decode
    S, D_ = op.n_src, op.n_dst
    (cbuf, crows, cpx), (sbuf, srows), field, coded, params, refs, E = make_streams(S, rows)
    ratio = coded[0].size / (2.0 * S)
    print(f"# {name}: streams written, {ratio:.3f} of the simple-packed bytes", file=sys.stderr, flush=True)
    y_c, y_o = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)      # the complex road's, the other roads'
    legs = {"complex16": lambda: op.apply_host_grib(cbuf, crows, cpx=cpx, out=y_c, chunk_rows=chunk_rows),
            "grib16": lambda: op.apply_host_grib(sbuf, srows, out=y_o),
            "f32": lambda: op.apply_host(field, out=y_o)}
    times = {k: [] for k in legs}
    for step in range(warmup + steps):
        print(f"# {name}: host step {step}", file=sys.stderr, flush=True)
        for leg, fn in legs.items():
            t0 = time.perf_counter()
            fn()
            dt = (time.perf_counter() - t0) * 1e3
            if step >= warmup:
                times[leg].append(dt)
            if step == 0 and leg != "complex16" and not np.array_equal(y_c.view(np.uint64), y_o.view(np.uint64)):
                raise SystemExit(f"{name}: the complex-packed road differs from the {'simple-packed' if leg == 'grib16' else 'decoded'} road")
    rec = np.array((0, coded[0].size, S) + params[0] + (0,), dtype=GRIB_CPX_DTYPE)
    row, dec = np.empty(S, np.float32), []
    for _ in range(max(5, steps)):
        t0 = time.perf_counter()
        row[:] = (refs[0] + cpx_decode(coded[0], rec).astype(np.float64) * 2.0 ** E) / 1.0
        dec.append((time.perf_counter() - t0) * 1e3)
    ms = {k: round(_median(v), 3) for k, v in times.items()}
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
           "complex_chunk_rows": chunk_rows, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
           "complex_over_simple_bytes": round(ratio, 4),
           "host_decode_ms_per_row": {"median": round(_median(dec), 3), "min": round(min(dec), 3)},
           "bits_equal_simple_packed": True}
    res["decoded_road_ms"] = round(_median(dec) * rows + ms["f32"], 1)       # one-thread decode of every row + apply_host
    res["grib16_over_complex16"] = round(ms["grib16"] / ms["complex16"], 3)
    res["decoded_road_over_complex16"] = round(res["decoded_road_ms"] / ms["complex16"], 2)
    return res


def _device_setup(op, rows):
    from smmregrid_amd import DeviceArray, to_device
    S = op.n_src
    (cbuf, crows, cpx), (sbuf, srows), field, coded, _, _, _ = make_streams(S, rows)

    def dev(buf):
        padded = np.zeros((buf.size + 3) // 4 * 4, np.uint8)
        padded[:buf.size] = buf
        return to_device(padded)
    return dev(cbuf), cbuf.size, crows, cpx, dev(sbuf), sbuf.size, srows, field, coded, DeviceArray((4 * S * rows,), np.uint8)


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, GribEncode, grib_pack, grib_unpack_cpx, to_device
    from smmregrid_amd.device import Event
    S, D_ = op.n_src, op.n_dst
    dc, c_bytes, crows, cpx, ds, s_bytes, srows, field, coded, out = _device_setup(op, rows)
    y, y_s = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
    _, rows_out = grib_unpack_cpx(dc, crows, cpx, x_bytes=c_bytes, out=out)
    pack_rows = min(rows, 32)                                # float64 values of that many rows (8 B each on host and device)
    values = to_device(field[:pack_rows].astype(np.float64))
    enc = GribEncode(NBITS, 0)
    legs = {"transcode": lambda: grib_unpack_cpx(dc, crows, cpx, x_bytes=c_bytes, out=out),
            "gather_of_transcoded": lambda: op.apply_grib(out, rows_out, y=y),
            "gather_of_simple": lambda: op.apply_grib(ds, srows, x_bytes=s_bytes, y=y_s),
            "grib_pack": lambda: grib_pack(values, enc)}
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
        if step == 0 and not np.array_equal(y.to_host().view(np.uint64), y_s.to_host().view(np.uint64)):
            raise SystemExit(f"{name}: the gather of the transcoded streams differs from the gather of the simple-packed ones")
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    return {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "ms": ms,
            "ms_min": {k: round(min(v), 4) for k, v in times.items()},
            "transcode_over_gather": round(ms["transcode"] / ms["gather_of_transcoded"], 3),
            "grib_pack_rows": pack_rows,
            "transcode_over_grib_pack_per_row": round((ms["transcode"] / rows) / (ms["grib_pack"] / pack_rows), 3),
            "transcode_gvalues_per_s": round(rows * S / ms["transcode"] / 1e6, 2),
            "coded_bytes": int(cpx["byte_len"].sum()), "stored_width": int(rows_out["nbits"][0]), "bits_equal_simple_packed": True}


def profile_run(op, rows):
    from smmregrid_amd import grib_unpack_cpx
    dc, c_bytes, crows, cpx, _, _, _, _, _, out = _device_setup(op, rows)
    for _ in range(4):
        grib_unpack_cpx(dc, crows, cpx, x_bytes=c_bytes, out=out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="host,kernel")
    ap.add_argument("--chunk-rows", type=int, default=0)
    ap.add_argument("--profile-run", action="store_true")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_complex_bench.jsonl"))
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
        if args.profile_run:
            profile_run(op, rows)
            op.close()
            continue
        for block in [b.strip() for b in args.blocks.split(",")]:
            res = bench_host(op, name, rows, args.steps, args.warmup, args.chunk_rows) if block == "host" else \
                bench_kernel(op, name, rows, args.steps, args.warmup)
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        op.close()


if __name__ == "__main__":
    main()
