"""Regrid results returned CCSDS-packed (`grib_aec_pack`: smm_grib_aec_pack behind smm_grib_pack;
`apply_host_grib(grib_out=GribEncode(w, ccsds=True))`) against the simple-packed result road, on config-2 rows
(r1440x721 -> r360x180, B = 512) and config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, B = 128), at 16 and 12
bits.  The source fields are the smooth synthetic ones of tools/grib_ccsds_bench.py, simple-packed.

One process, the legs interleaved step by step after a warm-up, medians of >= 5:
  kernel  HBM-resident, device ms from HIP events: the gather (apply_grib), the four passes of grib_pack behind it and
          grib_aec_pack behind those (its scratch is allocated and freed inside the call, which the figure includes);
          the bytes used against the simple-packed streams' bytes
  host    host to host, wall-clock ms, pageable input: grib_out=GribEncode(w, ccsds=True) (a synchronous Python chunk
          loop) against grib_out=GribEncode(w) (the pipelined C entry), the bytes each brings back over PCIe
Before anything is timed the coded result is decoded (first, second and last row) and compared bit for bit with the
simple-packed result.  One JSON line per block, printed and appended to profiles/grib_ccsds_out_bench.jsonl.

  python tools/grib_ccsds_out_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 5] [--warmup 1] [--only cfg2,cfg4]
                                       [--blocks kernel,host] [--widths 16,12]
"""
import functools

import benchlib
import coded_benches
from smmregrid_amd.griblite import CCSDS

bench_kernel = functools.partial(coded_benches.out_kernel, CCSDS)
bench_host = functools.partial(coded_benches.out_host, CCSDS)


def parser():
    ap = benchlib.parser(__doc__, steps=5, warmup=1, only="cfg2,cfg4", blocks="kernel,host", out="grib_ccsds_out_bench.jsonl")
    ap.add_argument("--widths", default="16,12")
    return ap


def main():
    args = benchlib.parse(parser(), why="medians need at least 5 timings")
    for name, op, rows in benchlib.operators(args):
        for block in benchlib.split(args.blocks):
            for width in [int(v) for v in args.widths.split(",")]:
                benchlib.emit((bench_kernel if block == "kernel" else bench_host)(op, name, rows, width, args.steps, args.warmup),
                              args.out)


if __name__ == "__main__":
    main()
