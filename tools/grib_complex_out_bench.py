"""Regrid results returned complex-packed (`grib_cpx_pack`: smm_grib_cpx_pack behind smm_grib_pack;
`apply_host_grib(grib_out=GribEncode(w, cpx=True))`) against the simple-packed and the CCSDS result roads, on config-2
rows (r1440x721 -> r360x180, B = 512) and config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, B = 128), at 16
bits.  The source fields are the smooth synthetic ones of tools/grib_complex_bench.py, simple-packed.

One process, the legs interleaved step by step after a warm-up, medians of >= 5:
  kernel  HBM-resident, device ms from HIP events: the gather (apply_grib), the four passes of grib_pack behind it, and
          behind those grib_cpx_pack (order 2, groups of 32) and grib_aec_pack (32 / 128 / preprocessor) on the same
          rows (each one's scratch is allocated and freed inside the call, which the figure includes); the bytes used
          against the simple-packed streams' bytes and against the CCSDS streams'
  sizes   no timing: the complex-packed bytes at every order and group length over the simple-packed bytes
  host    host to host, wall-clock ms, pageable input: grib_out=GribEncode(w, cpx=True) (a synchronous Python chunk loop)
          against grib_out=GribEncode(w) (the pipelined C entry) and against the same call without grib_out (float64
          back), the bytes each brings back over PCIe
Before anything is timed the coded result is decoded (first, second and last row) and compared bit for bit with the
simple-packed result.  One JSON line per block, printed and appended to profiles/grib_complex_out_bench.jsonl.

  python tools/grib_complex_out_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 5] [--warmup 1] [--only cfg2,cfg4]
                                         [--blocks kernel,sizes,host] [--width 16]
"""
import argparse
import importlib.util
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
_spec = importlib.util.spec_from_file_location("grib_complex_bench", os.path.join(ROOT, "tools", "grib_complex_bench.py"))
_in = importlib.util.module_from_spec(_spec)
_spec.loader.exec_module(_in)


def _median(v):
    return float(np.median(np.asarray(v)))


def source(S, rows):
    """DISTINCT smooth 16-bit fields simple-packed in one buffer, `rows` records pointing at them in turn."""
    from smmregrid_amd import GRIB_ROW_DTYPE
    rng = np.random.default_rng(20261020)
    blocks = [np.frombuffer(_in.smooth_field(S, i, rng).astype(">u2").tobytes(), dtype=np.uint8) for i in range(_in.DISTINCT)]
    offs, pos = [], 116
    for b in blocks:
        offs.append(pos)
        pos += b.size + 116
    buf = np.zeros((pos + 3) // 4 * 4, dtype=np.uint8)
    for o, b in zip(offs, blocks):
        buf[o:o + b.size] = b
    table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    for r in range(rows):
        table[r] = (offs[r % _in.DISTINCT], float(np.float32(220.0 + r % _in.DISTINCT)), 2.0 ** -6, 1.0, 16, 0)
    return buf, table


def sample_rows(field, idx):
    from smmregrid_amd import GribField
    return GribField(field.buf, field.rows[idx], (len(idx), field.n_points), field.n_points, bitmaps=field.bitmaps[idx],
                     ccsds=None if field.ccsds is None else field.ccsds[idx],
                     cpx=None if field.cpx is None else field.cpx[idx]).decode()


def _packed(op, rows, width):
    from smmregrid_amd import DeviceArray, GribEncode, grib_pack, to_device
    buf, table = source(op.n_src, rows)
    x = to_device(buf)
    y = DeviceArray((rows, op.n_dst), np.float64)
    op.apply_grib(x, table, y=y)
    packed, rows_p, bms = grib_pack(y, GribEncode(width, 0))
    simple = int(sum((op.n_dst * int(w) + 7) // 8 for w in rows_p["nbits"]))
    return x, table, y, packed, rows_p, bms, simple


def bench_kernel(op, name, rows, width, steps, warmup):
    from smmregrid_amd import DeviceArray, GribEncode, GribField, grib_aec_pack, grib_cpx_pack, grib_pack
    from smmregrid_amd.device import Event
    x, table, y, packed, rows_p, bms, simple = _packed(op, rows, width)
    enc, enc_aec, plain = GribEncode(width, 0, cpx=True), GribEncode(width, 0, ccsds=True), GribEncode(width, 0)
    want = enc.cpx_records(rows, bms["n_values"], rows_p["nbits"])
    want_aec = enc_aec.ccsds_records(rows, bms["n_values"], rows_p["nbits"])
    bound = DeviceArray((max(enc.cpx_bound(op.n_dst, rows), 4),), np.uint8)
    bound_aec = DeviceArray((max(enc_aec.ccsds_bound(op.n_dst, rows), 4),), np.uint8)
    coded, rows_c, recs = grib_cpx_pack(packed, rows_p, want, out=bound)
    _, _, recs_aec = grib_aec_pack(packed, rows_p, want_aec, out=bound_aec)
    idx = sorted({0, 1, rows - 1})
    got = sample_rows(GribField(coded.to_host(), rows_c, (rows, op.n_dst), op.n_dst, bitmaps=bms, cpx=recs), idx)
    ref = sample_rows(GribField(packed.to_host(), rows_p, (rows, op.n_dst), op.n_dst, bitmaps=bms), idx)
    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
        raise SystemExit(f"{name}: the coded result decodes to other bits than the simple-packed one")
    legs = {"gather": lambda: op.apply_grib(x, table, y=y), "grib_pack": lambda: grib_pack(y, plain, out=packed),
            "grib_cpx_pack": lambda: grib_cpx_pack(packed, rows_p, want, out=bound),
            "grib_aec_pack": lambda: grib_aec_pack(packed, rows_p, want_aec, out=bound_aec)}
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
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    cpx_bytes, aec_bytes = int(recs["byte_len"].sum()), int(recs_aec["byte_len"].sum())
    return {"block": "kernel", "op": name, "rows": rows, "nbits": width, "n_src": op.n_src, "n_dst": op.n_dst, "steps": steps,
            "ms": ms, "ms_min": {k: round(min(v), 4) for k, v in times.items()},
            "cpx_pack_over_aec_pack": round(ms["grib_cpx_pack"] / ms["grib_aec_pack"], 3),
            "cpx_pack_over_grib_pack": round(ms["grib_cpx_pack"] / ms["grib_pack"], 3),
            "cpx_pack_over_gather": round(ms["grib_cpx_pack"] / ms["gather"], 3),
            "cpx_bytes": cpx_bytes, "ccsds_bytes": aec_bytes, "simple_bytes": simple, "bound_bytes": bound.nbytes,
            "cpx_over_simple_bytes": round(cpx_bytes / max(simple, 1), 4), "cpx_over_ccsds_bytes": round(cpx_bytes / max(aec_bytes, 1), 4),
            "orders_coded": sorted(set(recs["order"].tolist())),
            "values_per_us": round(rows * op.n_dst / (ms["grib_cpx_pack"] * 1e3), 1), "bits_equal_simple_packed": True}


def bench_sizes(op, name, rows, width):
    from smmregrid_amd import GribEncode, grib_cpx_pack
    _, _, _, packed, rows_p, bms, simple = _packed(op, rows, width)
    ratios = {}
    for order in (0, 1, 2):
        for L in (8, 16, 32, 64):
            want = GribEncode(width, 0, cpx=(order, L)).cpx_records(rows, bms["n_values"], rows_p["nbits"])
            _, _, recs = grib_cpx_pack(packed, rows_p, want)
            ratios[f"o{order}_L{L}"] = round(int(recs["byte_len"].sum()) / max(simple, 1), 4)
    return {"block": "sizes", "op": name, "rows": rows, "nbits": width, "n_dst": op.n_dst, "simple_bytes": simple,
            "cpx_over_simple_bytes": ratios}


def bench_host(op, name, rows, width, steps, warmup):
    from smmregrid_amd import GribEncode, _lib
    buf, table = source(op.n_src, rows)
    simple_enc, coded_enc = GribEncode(width, 0), GribEncode(width, 0, cpx=True)
    res = {}
    legs = {"cpx": lambda: op.apply_host_grib(buf, table, grib_out=coded_enc),
            "simple": lambda: op.apply_host_grib(buf, table, grib_out=simple_enc),
            "float64": lambda: op.apply_host_grib(buf, table)}
    times, d2h = {k: [] for k in legs}, {}
    for step in range(warmup + steps):
        print(f"# {name} {width} bits: host step {step}", file=sys.stderr, flush=True)
        for leg, fn in legs.items():
            _lib.host_stats(reset=True)
            t0 = time.perf_counter()
            res[leg] = fn()
            dt = (time.perf_counter() - t0) * 1e3
            stats = _lib.host_stats(reset=True)
            d2h[leg] = int(res[leg].buf.size) if leg == "cpx" else int(stats["d2h_bytes"])
            if step >= warmup:
                times[leg].append(dt)
        if step == 0:
            idx = sorted({0, 1, rows - 1})
            if not np.array_equal(sample_rows(res["cpx"], idx).view(np.uint32), sample_rows(res["simple"], idx).view(np.uint32)):
                raise SystemExit(f"{name}: the coded result decodes to other bits than the simple-packed one")
    ms = {k: round(_median(v), 3) for k, v in times.items()}
    return {"block": "host_to_host", "op": name, "rows": rows, "nbits": width, "n_src": op.n_src, "n_dst": op.n_dst,
            "steps": steps, "ms": ms, "ms_min": {k: round(min(v), 3) for k, v in times.items()},
            "d2h_bytes": d2h, "float64_bytes": rows * op.n_dst * 8,
            "cpx_over_simple_ms": round(ms["cpx"] / ms["simple"], 3), "cpx_over_float64_ms": round(ms["cpx"] / ms["float64"], 3),
            "cpx_over_simple_d2h_bytes": round(d2h["cpx"] / max(d2h["simple"], 1), 4), "bits_equal_simple_packed": True}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="kernel,sizes,host")
    ap.add_argument("--width", type=int, default=16)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_complex_out_bench.jsonl"))
    args = ap.parse_args()
    if args.steps < 5:
        ap.error("medians need at least 5 timings")
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
            if block == "kernel":
                res = bench_kernel(op, name, rows, args.width, args.steps, args.warmup)
            elif block == "sizes":
                res = bench_sizes(op, name, rows, args.width)
            else:
                res = bench_host(op, name, rows, args.width, args.steps, args.warmup)
            print(json.dumps(res), flush=True)
            with open(args.out, "a") as f:
                f.write(json.dumps(res) + "\n")
        op.close()


if __name__ == "__main__":
    main()
