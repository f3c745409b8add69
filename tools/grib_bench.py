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
import os
import sys
import tempfile

import numpy as np

import benchlib
from bench_inputs import lonlat_messages, make_streams, padded_upload


def time_decode(block, nbits, S, ref, E, D, steps):
    """griblite's decode of one message, as open_grib runs it: unpack, the float64 statement, the float32 store."""
    from smmregrid_amd.griblite import _unpack_bits
    row = np.empty(S, dtype=np.float32)

    def decode():
        row[:] = (ref + _unpack_bits(block, nbits, S) * 2.0 ** E) / 10.0 ** D
    return benchlib.time_calls(decode, steps)


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

    def check(leg, _):
        if leg.startswith("f32_of_") and not benchlib.same_bits(y_raw, y_f32):      # the raw leg of the same width ran just before
            raise SystemExit(f"{name}: apply_host_grib at {leg[7:]} bits differs from the parent road")
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, check=check,
                                      announce=f"# {name}: host step {{}}")
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           **benchlib.summary(times, 3),
           "h2d_bytes": {k: int(s[-1]["h2d_bytes"]) for k, s in stats.items()},
           "d2h_bytes": {k: int(s[-1]["d2h_bytes"]) for k, s in stats.items()},
           "chunks": {k: int(s[-1]["chunks"]) for k, s in stats.items()}, "bits_equal_parent": True}
    for nbits in (16, 12):
        _, _, _, block, ref, E = streams[nbits]
        dec = time_decode(block, nbits, S, ref, E, 0, max(5, steps))
        res[f"decode{nbits}_ms_per_row"] = benchlib.median_and_min(dec)
        parent = benchlib.median(dec) * rows + res["ms"][f"f32_of_{nbits}"]
        res[f"parent_road{nbits}_ms"] = round(parent, 1)          # decode of every row (one thread, as today) + apply_host
        res[f"parent_over_grib{nbits}"] = round(parent / res["ms"][f"grib{nbits}"], 2)
        res[f"apply_host_f32_over_grib{nbits}"] = round(res["ms"][f"f32_of_{nbits}"] / res["ms"][f"grib{nbits}"], 3)
    return res


def bench_open(op, name, rows, steps, warmup):
    """File to result: what a user of io.open_dataset pays on either road (r1440x721 lon/lat messages at 16 bits)."""
    from smmregrid_amd.io import open_dataset
    ni, nj = 1440, 721
    assert op.n_src == ni * nj
    tmp = tempfile.mkdtemp()
    path = os.path.join(tmp, "t2m.grib")
    with open(path, "wb") as f:
        f.write(b"".join(lonlat_messages(rows, ni, nj)))
    print(f"# {name}: GRIB file of {rows} messages written", file=sys.stderr, flush=True)
    y_raw, y_f32 = np.empty((rows, op.n_dst), np.float64), np.empty((rows, op.n_dst), np.float64)
    got = {}
    legs = {"open_decoded": lambda: got.update(field=open_dataset(path)["t2m"].data),
            "apply_host_f32": lambda: op.apply_host(got["field"].reshape(rows, -1), out=y_f32),
            "open_raw": lambda: got.update(raw=open_dataset(path, decode=False)["t2m"].data),
            "apply_host_grib": lambda: op.apply_host_grib(got["raw"].buf, got["raw"].rows, out=y_raw)}

    def bits():
        if not benchlib.same_bits(y_raw, y_f32):
            raise SystemExit(f"{name}: the raw road differs from the parent road on the file")
    times = benchlib.time_wall(legs, steps, warmup, after_first=bits)
    os.remove(path)
    os.rmdir(tmp)
    res = benchlib.summary(times, 3)
    ms = res["ms"]
    parent, rawroad = ms["open_decoded"] + ms["apply_host_f32"], ms["open_raw"] + ms["apply_host_grib"]
    return {"block": "file_to_result", "op": name, "rows": rows, "n_src": op.n_src, "n_dst": op.n_dst, "steps": steps,
            "nbits": 16, **res, "parent_road_ms": round(parent, 3), "raw_road_ms": round(rawroad, 3),
            "parent_over_raw": round(parent / rawroad, 2), "bits_equal_parent": True}


def bench_kernel(op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, _lib, to_device
    S, D_ = op.n_src, op.n_dst
    legs, check = {}, {}
    y_div = DeviceArray((rows, D_), np.float64)                 # the legs with the division share one result
    for nbits in (16, 12):
        buf, table, field, *_ = make_streams(S, rows, 0, widths=(nbits,))[nbits]
        dx, y = padded_upload(buf), DeviceArray((rows, D_), np.float64)
        table_div = table.copy()
        table_div["ddiv"] = 10.0                                # the same bits with D = 1
        legs[f"grib{nbits}_nodiv"] = lambda dx=dx, y=y, table=table, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y)
        legs[f"grib{nbits}_div"] = lambda dx=dx, table=table_div, n=buf.size: op.apply_grib(dx, table, x_bytes=n, y=y_div)
        dfield, y32 = to_device(field), DeviceArray((rows, D_), np.float64)
        legs[f"f32_sell_of_{nbits}"] = lambda dfield=dfield, y32=y32: op.apply(dfield, y=y32, flags=_lib.APPLY_KERNEL_SELL)
        check[nbits] = (y, y32)
        del buf, field

    def bits():
        for nbits, (y, y32) in check.items():
            if not benchlib.same_bits(y.rows(0, 2).to_host(), y32.rows(0, 2).to_host()):
                raise SystemExit(f"{name}: smm_apply_grib at {nbits} bits differs from smm_apply on the decoded field")
    res = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup, after_first=bits), 4), "bits_equal_parent": True}
    ms = res["ms"]
    res["over_f32_sell"] = {k: round(ms[k] / ms[f"f32_sell_of_{k[4:6]}"], 3) for k in ms if k.startswith("grib")}
    return res


def parser():
    ap = benchlib.parser(__doc__, steps=7, warmup=2, only="cfg2,cfg4", blocks="host,kernel,open", out="grib_bench.jsonl")
    ap.add_argument("--open-rows", type=int, default=16)
    return ap


def main():
    args = benchlib.parse(parser())
    for name, op, rows in benchlib.operators(args):
        for block in benchlib.split(args.blocks):
            if block == "open":
                if name != "cfg2":          # the file's messages are r1440x721 lon/lat fields
                    continue
                res = bench_open(op, name, args.open_rows, args.steps, args.warmup)
            else:
                res = (bench_host if block == "host" else bench_kernel)(op, name, rows, args.steps, args.warmup)
            res["used_src_share"] = round(op.n_used_src / op.n_src, 4)
            benchlib.emit(res, args.out)


if __name__ == "__main__":
    main()
