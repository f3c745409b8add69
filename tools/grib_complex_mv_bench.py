"""Complex-packed GRIB-2 fields with missing values coded inside the groups (missing value management 1) on the device:
the step that turns them into a bitmap plus the compacted integers (`grib_unpack_cpx_mv`) against the step for the same
integers coded with missing value management 0 beside a section-6 bitmap (`grib_unpack_cpx`), and the gather behind
each (`apply_grib(bitmaps=)`).  Config-2 rows (r1440x721 -> r360x180) at B = 512 and config-4 geometry (n1280 -> hp1024) at
B = 128; the smooth synthetic 16-bit fields of tools/grib_complex_bench.py with 30 % of the cells missing at random; order
2, groups of 32 positions.  The streams are written by `bench_inputs.encode_complex_mv` and decoded back by the library's host
decoder before anything is timed; the two roads' results are compared bit for bit before anything is timed, and the
tool stops if they differ.  The legs are interleaved step by step after a warm-up, median and best:
  kernel  HBM-resident, device ms from HIP events: the two device steps and the gather behind each
  host    host to host, wall-clock ms, pageable input and output: `apply_host_grib(cpx=, cpx_missing=)` against
          `apply_host_grib(cpx=, bitmaps=)`
  parent  with --parent-lib: smm_grib_cpx_unpack on rows with mvm 0 (the smooth fields with no cell missing) called
          through this build's library and through a library built from the parent commit, both loaded into this
          process, wall-clock ms around the call (it synchronises before it returns).  Per step: parent, this, parent
          again -- `spread` is the relative difference of the two parent medians, `this_over_parent` this build's median
          over the median of all parent runs.  The path gains no pass, so "unchanged" is the expectation; a ratio
          beyond the spread is said so in DESIGN.  Building the parent's library: its csrc and include folders checked
          out elsewhere, `make OUT=<path>` there.

One JSON line per block and geometry, printed and appended to profiles/grib_complex_mv_bench.jsonl.

  python tools/grib_complex_mv_bench.py [--cfg4-rows 128] [--cfg2-rows 512] [--steps 5] [--warmup 1] [--only cfg2,cfg4]
                                        [--blocks kernel,host,parent] [--parent-lib PATH]
"""
import ctypes

import numpy as np

import benchlib
from bench_inputs import MISSING, make_mv_streams, make_plain_complex_streams


def bench(op, name, rows, steps, warmup, blocks):
    from smmregrid_amd import DeviceArray, _lib, grib_unpack_cpx, grib_unpack_cpx_mv, to_device
    S, D_ = op.n_src, op.n_dst
    buf, table, cpx_mv, cpx_0, bms = make_mv_streams(S, rows)
    x = to_device(buf)
    missing = np.ones(rows, dtype=np.uint8)
    out_mv, rows_mv, bms_mv = grib_unpack_cpx_mv(x, table, cpx_mv, missing)
    out_0, rows_0 = grib_unpack_cpx(x, table, cpx_0)
    # the mvm-0 road's bitmaps stay in x: its gather reads x and the transcoded streams as one buffer
    both = DeviceArray((x.nbytes + out_0.nbytes,), np.uint8)
    rows_b = rows_0.copy()
    rows_b["byte_off"] += np.uint64(x.nbytes)
    _lib.call("smm_memcpy_d2d", ctypes.c_void_p(both.ptr), ctypes.c_void_p(x.ptr), x.nbytes, None)
    _lib.call("smm_memcpy_d2d", ctypes.c_void_p(both.ptr + x.nbytes), ctypes.c_void_p(out_0.ptr), out_0.nbytes, None)
    y, y_0 = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
    legs = {"unpack_mvm1": lambda: grib_unpack_cpx_mv(x, table, cpx_mv, missing, out=out_mv),
            "unpack_mvm0_with_bitmap": lambda: grib_unpack_cpx(x, table, cpx_0, out=out_0),
            "gather_of_mvm1": lambda: op.apply_grib(out_mv, rows_mv, bitmaps=bms_mv, y=y),
            "gather_of_mvm0_with_bitmap": lambda: op.apply_grib(both, rows_b, bitmaps=bms, y=y_0)}

    def bits():
        if not benchlib.same_bits(y.to_host(), y_0.to_host()):
            raise SystemExit(f"{name}: the gather behind the mvm-1 rows differs from the gather of the bitmapped mvm-0 rows")
    kernel = benchlib.summary(benchlib.time_events(legs, steps, warmup, after_first=bits), 4)
    ms = kernel["ms"]
    common = {"op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING}
    lines = []
    if "kernel" in blocks:
        lines.append(dict(common, block="kernel", **kernel,
                          mvm1_over_mvm0_with_bitmap=round(ms["unpack_mvm1"] / ms["unpack_mvm0_with_bitmap"], 3),
                          unpack_mvm1_gpositions_per_s=round(rows * S / ms["unpack_mvm1"] / 1e6, 2),
                          coded_bytes_mvm1=int(cpx_mv["byte_len"].sum()), coded_bytes_mvm0=int(cpx_0["byte_len"].sum())))
    if "host" in blocks:
        want = y.to_host()
        for a in (y, y_0, both, out_mv, out_0):
            a.free()
        y_h = np.empty((rows, D_), np.float64)        # both legs write it: one result of cfg4 is 13 GB
        hlegs = {"apply_host_grib_mvm1": lambda: op.apply_host_grib(buf, table, cpx=cpx_mv, cpx_missing=missing, out=y_h),
                 "apply_host_grib_mvm0_with_bitmap": lambda: op.apply_host_grib(buf, table, cpx=cpx_0, bitmaps=bms, out=y_h)}

        def check(leg, _):
            if not benchlib.same_bits(y_h, want):
                raise SystemExit(f"{name}: the result of {leg} differs from the device gather's")
        host = benchlib.summary(benchlib.time_wall(hlegs, steps, warmup, check=check), 3)
        hms = host["ms"]
        lines.append(dict(common, block="host", **host,
                          mvm1_over_mvm0_with_bitmap=round(hms["apply_host_grib_mvm1"] / hms["apply_host_grib_mvm0_with_bitmap"], 3)))
    return lines


def bench_parent(name, S, rows, steps, warmup, parent_path):
    """smm_grib_cpx_unpack on mvm-0 rows through this build's library and the parent's."""
    from smmregrid_amd import GRIB_ROW_DTYPE, DeviceArray, _lib, to_device
    buf, cpx = make_plain_complex_streams(S, rows)
    table, table_out = np.zeros(rows, dtype=GRIB_ROW_DTYPE), np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    x = to_device(buf)
    outs = {"this": DeviceArray((4 * S * rows,), np.uint8), "parent": DeviceArray((4 * S * rows,), np.uint8)}
    libs = {"this": _lib.load(), "parent": ctypes.CDLL(parent_path)}
    libs["parent"].smm_grib_cpx_unpack.argtypes = _lib.SIGNATURES["smm_grib_cpx_unpack"]
    libs["parent"].smm_grib_cpx_unpack.restype = ctypes.c_int

    def call(which):
        rc = libs[which].smm_grib_cpx_unpack(0, ctypes.c_void_p(x.ptr), buf.size, ctypes.cast(cpx.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct)),
                                             ctypes.cast(table.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)), rows,
                                             ctypes.c_void_p(outs[which].ptr), outs[which].nbytes,
                                             ctypes.cast(table_out.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)), None)
        if rc != 0:
            raise SystemExit(f"{name}: smm_grib_cpx_unpack of the {which} library returned {rc}")
    legs = {"parent_first": lambda: call("parent"), "this": lambda: call("this"), "parent_again": lambda: call("parent")}

    def bits():
        used = (S * int(table_out["nbits"][0]) + 7) // 8
        a = DeviceArray((used,), np.uint8, ptr=outs["this"].ptr, base=outs["this"]).to_host()
        b = DeviceArray((used,), np.uint8, ptr=outs["parent"].ptr, base=outs["parent"]).to_host()
        if not np.array_equal(a, b):
            raise SystemExit(f"{name}: the two libraries wrote different bytes for row 0")
    times = benchlib.time_wall(legs, steps, warmup, after_first=bits)
    res = benchlib.summary(times, 4)
    ms = res["ms"]
    parent = benchlib.median(times["parent_first"] + times["parent_again"])
    return {"block": "parent", "op": name, "rows": rows, "n_src": S, "steps": steps, **res,
            "spread": round(abs(ms["parent_first"] - ms["parent_again"]) / min(ms["parent_first"], ms["parent_again"]), 4),
            "this_over_parent": round(ms["this"] / parent, 4)}


def parser():
    ap = benchlib.parser(__doc__, steps=5, warmup=1, only="cfg2,cfg4", blocks="kernel,host,parent", out="grib_complex_mv_bench.jsonl")
    ap.add_argument("--parent-lib", default=None, help="a libsmmregrid_hip.so built from the parent commit (block parent)")
    return ap


def main():
    args = parser().parse_args()
    blocks = benchlib.split(args.blocks)
    for name, op, rows in benchlib.operators(args, announce=False):
        lines = bench(op, name, rows, args.steps, args.warmup, blocks) if {"kernel", "host"} & set(blocks) else []
        if "parent" in blocks and args.parent_lib:
            lines.append(bench_parent(name, op.n_src, rows, args.steps, args.warmup, args.parent_lib))
        for line in lines:
            benchlib.emit(line, args.out)


if __name__ == "__main__":
    main()
