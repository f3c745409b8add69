"""Complex-packed GRIB-2 fields (templates 5.2 / 5.3) regridded raw (`apply_host_grib(cpx=)`: smm_grib_cpx_unpack ahead
of the GRIB gather) against the two roads the same data could take -- the same integers simple-packed through
apply_host_grib, and a one-thread host decode (smm_grib_cpx_decode_host, as `GribField.decode` runs it) followed by
apply_host on the float32 field -- on config-4 geometry (regular Gaussian n1280 -> HEALPix 1024, bilinear) at B = 128 and
on config-2 rows (r1440x721 -> r360x180) at B = 512.  The fields are synthetic and smooth (a few waves plus noise of a few
counts at 16 bits); the streams are written by `bench_inputs.encode_complex` (order 2, three octets per descriptor, groups of a
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
import functools

import benchlib
import coded_benches
from smmregrid_amd.griblite import CPX

bench_host = functools.partial(coded_benches.in_host, CPX)
bench_kernel = functools.partial(coded_benches.in_kernel, CPX)
profile_run = functools.partial(coded_benches.in_profile_run, CPX)


def parser():
    return coded_benches.in_parser(CPX, __doc__)


def main():
    coded_benches.in_run(CPX, benchlib.parse(parser()))


if __name__ == "__main__":
    main()
