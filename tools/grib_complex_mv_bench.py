"""Complex-packed GRIB-2 fields with missing values coded inside the groups (missing value management 1) on the device:
the step that turns them into a bitmap plus the compacted integers (`grib_unpack_cpx_mv`) against the step for the same
integers coded with missing value management 0 beside a section-6 bitmap (`grib_unpack_cpx`), and the gather behind
each (`apply_grib(bitmaps=)`).  Config-2 rows (r1440x721 -> r360x180) at B = 512 and config-4 geometry (n1280 -> hp1024) at
B = 128; the smooth synthetic 16-bit fields of tools/grib_complex_bench.py with 30 % of the cells missing at random; order
2, groups of 32 positions.  The streams are written by the small encoder below and decoded back by the library's host
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
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from tools.grib_complex_bench import DISTINCT, GROUP, N_OCT, _bit_length, _median, _pack, _sm, encode_complex, smooth_field  # noqa: E402

MISSING = 0.3


def encode_complex_mv(q, present, group=GROUP, n_oct=N_OCT):
    """(stream, the fields of a GRIB_CPX_DTYPE record from n_groups to n_oct) of a row of present.size positions under
    missing value management 1: the present ones hold the integers q in order (order 2 over them), a missing one holds
    2^w - 1 of its group, every group wide enough to keep its values below that code."""
    x = np.asarray(q, dtype=np.int64)
    d = np.zeros(x.size, dtype=np.int64)
    d[2:] = x[2:] - 2 * x[1:-1] + x[:-2]
    g = int(d[2:].min())
    zc = d - g
    zc[:2] = 0
    n = present.size
    ng = (n + group - 1) // group
    there = np.concatenate([present, np.zeros(ng * group - n, dtype=bool)]).reshape(ng, group)
    z = np.zeros(ng * group, dtype=np.int64)
    z[np.flatnonzero(there.ravel())] = zc
    z = z.reshape(ng, group)
    if not there.any(axis=1).all():
        raise SystemExit("a group without a present position: the tool's encoder does not write those")
    ref = np.where(there, z, np.iinfo(np.int64).max).min(axis=1)
    w = _bit_length(np.where(there, z, 0).max(axis=1) - ref + 1)          # span < 2^w - 1
    stored = np.where(there, z - ref[:, None], (np.int64(1) << w)[:, None] - 1)
    nbits, width_ref = int(_bit_length(ref.max() + 1)), int(w.min())
    width_bits = int(_bit_length(w.max() - width_ref))
    stream = _sm(x[0], n_oct) + _sm(x[1], n_oct) + _sm(g, n_oct) + _pack(ref, np.full(ng, nbits)).tobytes() + \
        _pack(w - width_ref, np.full(ng, width_bits)).tobytes() + _pack(stored.ravel()[:n], np.repeat(w, group)[:n]).tobytes()
    return np.frombuffer(stream, dtype=np.uint8), (ng, nbits, width_ref, width_bits, group, 1, n - (ng - 1) * group, 0, 2, n_oct)


def bench(op, name, rows, steps, warmup, blocks):
    from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_ROW_DTYPE, DeviceArray, grib_unpack_cpx, grib_unpack_cpx_mv, to_device
    from smmregrid_amd.device import Event
    from smmregrid_amd.griblite import cpx_decode, cpx_decode_mv
    S, D_ = op.n_src, op.n_dst
    rng = np.random.default_rng(20261020)
    parts, at, mv_at, plain_at, bm_at, counts = [], 0, [], [], [], []

    def put(data):
        nonlocal at
        off = at
        parts.append(np.asarray(data, np.uint8))
        parts.append(np.zeros(-data.size % 4 + 4, np.uint8))
        at += parts[-2].size + parts[-1].size
        return off
    for i in range(DISTINCT):
        present = rng.random(S) >= MISSING
        q = smooth_field(S, i, rng)[present]
        s_mv, p_mv = encode_complex_mv(q, present)
        s_0, p_0 = encode_complex(q)
        got, there = cpx_decode_mv(s_mv, np.array((0, s_mv.size, S) + p_mv + (0,), dtype=GRIB_CPX_DTYPE), 1)
        if not (np.array_equal(got, q) and np.array_equal(there, present) and
                np.array_equal(cpx_decode(s_0, np.array((0, s_0.size, q.size) + p_0 + (0,), dtype=GRIB_CPX_DTYPE)), q)):
            raise SystemExit("the tool's encoder wrote a stream the host decoder reads differently")
        mv_at.append((put(s_mv), s_mv.size, p_mv))
        plain_at.append((put(s_0), s_0.size, p_0))
        bm_at.append(put(np.packbits(present)))
        counts.append(int(q.size))
    buf = np.concatenate(parts)
    table = np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    cpx_mv, cpx_0 = np.zeros(rows, dtype=GRIB_CPX_DTYPE), np.zeros(rows, dtype=GRIB_CPX_DTYPE)
    bms = np.zeros(rows, dtype=GRIB_BITMAP_DTYPE)
    for r in range(rows):
        k = r % DISTINCT
        table[r] = (0, 220.0 + k, 2.0 ** -6, 1.0, 16, 0)
        cpx_mv[r] = (mv_at[k][0], mv_at[k][1], S) + mv_at[k][2] + (0,)
        cpx_0[r] = (plain_at[k][0], plain_at[k][1], counts[k]) + plain_at[k][2] + (0,)
        bms[r] = (bm_at[k], counts[k])
    x = to_device(buf)
    missing = np.ones(rows, dtype=np.uint8)
    out_mv, rows_mv, bms_mv = grib_unpack_cpx_mv(x, table, cpx_mv, missing)
    out_0, rows_0 = grib_unpack_cpx(x, table, cpx_0)
    # the mvm-0 road's bitmaps stay in x: its gather reads x and the transcoded streams as one buffer
    both = DeviceArray((x.nbytes + out_0.nbytes,), np.uint8)
    rows_b = rows_0.copy()
    rows_b["byte_off"] += np.uint64(x.nbytes)
    from smmregrid_amd import _lib
    _lib.call("smm_memcpy_d2d", ctypes.c_void_p(both.ptr), ctypes.c_void_p(x.ptr), x.nbytes, None)
    _lib.call("smm_memcpy_d2d", ctypes.c_void_p(both.ptr + x.nbytes), ctypes.c_void_p(out_0.ptr), out_0.nbytes, None)
    y, y_0 = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
    legs = {"unpack_mvm1": lambda: grib_unpack_cpx_mv(x, table, cpx_mv, missing, out=out_mv),
            "unpack_mvm0_with_bitmap": lambda: grib_unpack_cpx(x, table, cpx_0, out=out_0),
            "gather_of_mvm1": lambda: op.apply_grib(out_mv, rows_mv, bitmaps=bms_mv, y=y),
            "gather_of_mvm0_with_bitmap": lambda: op.apply_grib(both, rows_b, bitmaps=bms, y=y_0)}
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
        if step == 0 and not np.array_equal(y.to_host().view(np.uint64), y_0.to_host().view(np.uint64)):
            raise SystemExit(f"{name}: the gather behind the mvm-1 rows differs from the gather of the bitmapped mvm-0 rows")
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    common = {"op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps, "missing": MISSING}
    lines = []
    if "kernel" in blocks:
        lines.append(dict(common, block="kernel", ms=ms, ms_min={k: round(min(v), 4) for k, v in times.items()},
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
        htimes = {k: [] for k in hlegs}
        for step in range(warmup + steps):
            for leg, fn in hlegs.items():
                t0 = time.perf_counter()
                fn()
                if step >= warmup:
                    htimes[leg].append(1e3 * (time.perf_counter() - t0))
                if step == 0 and not np.array_equal(y_h.view(np.uint64), want.view(np.uint64)):
                    raise SystemExit(f"{name}: the result of {leg} differs from the device gather's")
        hms = {k: round(_median(v), 3) for k, v in htimes.items()}
        lines.append(dict(common, block="host", ms=hms, ms_min={k: round(min(v), 3) for k, v in htimes.items()},
                          mvm1_over_mvm0_with_bitmap=round(hms["apply_host_grib_mvm1"] / hms["apply_host_grib_mvm0_with_bitmap"], 3)))
    return lines


def bench_parent(name, S, rows, steps, warmup, parent_path):
    """smm_grib_cpx_unpack on mvm-0 rows through this build's library and the parent's."""
    from smmregrid_amd import GRIB_CPX_DTYPE, GRIB_ROW_DTYPE, DeviceArray, _lib, to_device
    rng = np.random.default_rng(20261020)
    parts, offs, pars = [], [], []
    at = 0
    for i in range(DISTINCT):
        stream, p = encode_complex(smooth_field(S, i, rng))
        parts += [stream, np.zeros(-stream.size % 4 + 4, np.uint8)]
        offs.append((at, stream.size))
        pars.append(p)
        at += parts[-2].size + parts[-1].size
    buf = np.concatenate(parts)
    table, table_out = np.zeros(rows, dtype=GRIB_ROW_DTYPE), np.zeros(rows, dtype=GRIB_ROW_DTYPE)
    cpx = np.zeros(rows, dtype=GRIB_CPX_DTYPE)
    for r in range(rows):
        k = r % DISTINCT
        cpx[r] = (offs[k][0], offs[k][1], S) + pars[k] + (0,)
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
    legs = [("parent_first", "parent"), ("this", "this"), ("parent_again", "parent")]
    times = {k: [] for k, _ in legs}
    for step in range(warmup + steps):
        for leg, which in legs:
            t0 = time.perf_counter()
            call(which)
            if step >= warmup:
                times[leg].append(1e3 * (time.perf_counter() - t0))
        if step == 0:
            used = (S * int(table_out["nbits"][0]) + 7) // 8
            a = DeviceArray((used,), np.uint8, ptr=outs["this"].ptr, base=outs["this"]).to_host()
            b = DeviceArray((used,), np.uint8, ptr=outs["parent"].ptr, base=outs["parent"]).to_host()
            if not np.array_equal(a, b):
                raise SystemExit(f"{name}: the two libraries wrote different bytes for row 0")
    ms = {k: round(_median(v), 4) for k, v in times.items()}
    parent = _median(times["parent_first"] + times["parent_again"])
    return {"block": "parent", "op": name, "rows": rows, "n_src": S, "steps": steps, "ms": ms,
            "ms_min": {k: round(min(v), 4) for k, v in times.items()},
            "spread": round(abs(ms["parent_first"] - ms["parent_again"]) / min(ms["parent_first"], ms["parent_again"]), 4),
            "this_over_parent": round(ms["this"] / parent, 4)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--cfg4-rows", type=int, default=128)
    ap.add_argument("--cfg2-rows", type=int, default=512)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--only", default="cfg2,cfg4")
    ap.add_argument("--blocks", default="kernel,host,parent")
    ap.add_argument("--parent-lib", default=None, help="a libsmmregrid_hip.so built from the parent commit (block parent)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "grib_complex_mv_bench.jsonl"))
    args = ap.parse_args()
    from smmregrid_amd import SparseOperator, gridgen
    cases = {"cfg4": ("n1280", "hp1024", args.cfg4_rows), "cfg2": ("r1440x721", "r360x180", args.cfg2_rows)}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    for name in [c.strip() for c in args.only.split(",")]:
        sgrid, tgrid, rows = cases[name]
        w = gridgen.generate_weights(sgrid, tgrid, method="bil")
        op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                            w["dst_address"].values, w["remap_matrix"].values, device=0)
        blocks = [b.strip() for b in args.blocks.split(",")]
        lines = bench(op, name, rows, args.steps, args.warmup, blocks) if {"kernel", "host"} & set(blocks) else []
        if "parent" in blocks and args.parent_lib:
            lines.append(bench_parent(name, op.n_src, rows, args.steps, args.warmup, args.parent_lib))
        for line in lines:
            print(json.dumps(line), flush=True)
            with open(args.out, "a") as fh:
                fh.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
