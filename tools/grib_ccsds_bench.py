"""CCSDS-packed GRIB-2 fields regridded raw (`apply_host_grib(ccsds=)`: smm_grib_aec_unpack ahead of the GRIB gather)
against the two roads the same data could take -- the same integers simple-packed through apply_host_grib, and a
one-thread host decode (smm_grib_aec_decode_host, as `GribField.decode` runs it) followed by apply_host on the float32
field -- on config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, bilinear) at B = 128 and on config-2 rows
(r1440x721 -> r360x180) at B = 512.  The fields are synthetic and smooth (a few waves plus noise of a few counts at 16
bits); the streams are written by `bench_inputs.encode_ccsds` (preprocessor on, J = 32, rsi = 128: what ecCodes asks of
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
import functools

import benchlib
import coded_benches
from smmregrid_amd.griblite import CCSDS

bench_host = functools.partial(coded_benches.in_host, CCSDS)
bench_kernel = functools.partial(coded_benches.in_kernel, CCSDS)


def parser():
    return coded_benches.in_parser(CCSDS, __doc__)


def main():
    coded_benches.in_run(CCSDS, benchlib.parse(parser()))


if __name__ == "__main__":
    main()
