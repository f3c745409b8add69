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
import functools

import benchlib
import coded_benches
from smmregrid_amd.griblite import CPX

bench_kernel = functools.partial(coded_benches.out_kernel, CPX)
bench_host = functools.partial(coded_benches.out_host, CPX)


def bench_sizes(op, name, rows, width):
    from smmregrid_amd import GribEncode, grib_cpx_pack
    _, _, _, packed, rows_p, bms, simple = coded_benches.packed_result(CPX, op, rows, GribEncode(width, 0))
    ratios = {}
    for order in (0, 1, 2):
        for L in (8, 16, 32, 64):
            want = GribEncode(width, 0, cpx=(order, L)).coded_records(rows, bms["n_values"], rows_p["nbits"], codec=CPX)
            _, _, recs = grib_cpx_pack(packed, rows_p, want)
            ratios[f"o{order}_L{L}"] = round(int(recs["byte_len"].sum()) / max(simple, 1), 4)
    return {"block": "sizes", "op": name, "rows": rows, "nbits": width, "n_dst": op.n_dst, "simple_bytes": simple,
            "cpx_over_simple_bytes": ratios}


def parser():
    ap = benchlib.parser(__doc__, steps=5, warmup=1, only="cfg2,cfg4", blocks="kernel,sizes,host", out="grib_complex_out_bench.jsonl")
    ap.add_argument("--width", type=int, default=16)
    return ap


def main():
    args = benchlib.parse(parser(), why="medians need at least 5 timings")
    for name, op, rows in benchlib.operators(args):
        for block in benchlib.split(args.blocks):
            if block == "sizes":
                res = bench_sizes(op, name, rows, args.width)
            else:
                res = (bench_kernel if block == "kernel" else bench_host)(op, name, rows, args.width, args.steps, args.warmup)
            benchlib.emit(res, args.out)


if __name__ == "__main__":
    main()
