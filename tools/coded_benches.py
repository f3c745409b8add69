"""The bodies of the four coded-GRIB tools, one per direction, driven by the `griblite.CODECS` entry of the codec:
grib_ccsds_bench.py / grib_complex_bench.py (coded input regridded raw) and grib_ccsds_out_bench.py /
grib_complex_out_bench.py (results returned coded) are entry points that name their codec, carry their docstring and
add their own options.  What a codec needs beside its CODECS entry stands in IN and OUT below, by the entry's name.
"""
import sys

import numpy as np

import benchlib
from bench_inputs import NBITS, SEEDS, coded_record, make_coded_streams, padded_upload, source

# coded input: the leg's name and the road's name in messages, the device bytes of a transcoded row, whether the host
# block counts the bytes shipped, the rows the kernel block keeps (None: all) and compares, and the complex tool's
# extra legs
IN = {"ccsds": dict(leg="ccsds16", road="CCSDS", out_bytes=lambda S: (2 * S + 3) // 4 * 4, h2d=True, kernel_rows=16,
                    compare_rows=2, extras=False),
      "cpx": dict(leg="complex16", road="complex-packed", out_bytes=lambda S: 4 * S, h2d=False, kernel_rows=None,
                  compare_rows=None, extras=True)}


def unpack_of(codec):
    import smmregrid_amd
    return {"ccsds": smmregrid_amd.grib_unpack, "cpx": smmregrid_amd.grib_unpack_cpx}[codec.name]


def in_host(codec, op, name, rows, steps, warmup, chunk_rows=0):
    from smmregrid_amd import _lib
    d = IN[codec.name]
    leg, prefix = d["leg"], d["leg"][:-2]
    S, D_ = op.n_src, op.n_dst
    (cbuf, crows, recs), (sbuf, srows), field, coded, params, refs, E = make_coded_streams(codec, S, rows)
    ratio = coded[0].size / (2.0 * S)
    print(f"# {name}: streams written, {ratio:.3f} of the simple-packed bytes", file=sys.stderr, flush=True)
    y_c, y_o = np.empty((rows, D_), np.float64), np.empty((rows, D_), np.float64)      # the coded road's, the other roads'
    legs = {leg: lambda: op.apply_host_grib(cbuf, crows, out=y_c, chunk_rows=chunk_rows, **{codec.name: recs}),
            "grib16": lambda: op.apply_host_grib(sbuf, srows, out=y_o),
            "f32": lambda: op.apply_host(field, out=y_o)}

    def check(which, _):
        if which != leg and not benchlib.same_bits(y_c, y_o):
            raise SystemExit(f"{name}: the {d['road']} road differs from the {'simple-packed' if which == 'grib16' else 'decoded'} road")
    timed = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats if d["h2d"] else None, check=check,
                               announce=f"# {name}: host step {{}}")
    times, stats = timed if d["h2d"] else (timed, None)
    rec = coded_record(codec, 0, coded[0], S, params[0])
    row = np.empty(S, np.float32)

    def decode():
        row[:] = (refs[0] + codec.decode(coded[0], rec, 0)[0].astype(np.float64) * 2.0 ** E) / 1.0
    dec = benchlib.time_calls(decode, max(5, steps))
    res = {"block": "host_to_host", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           f"{prefix}_chunk_rows": chunk_rows, **benchlib.summary(times, 3)}
    ms = res["ms"]
    if d["h2d"]:
        staged = int(sum((int(n) + 3) // 4 * 4 for n in recs["byte_len"]))
        res["h2d_bytes"] = {leg: staged, "grib16": int(stats["grib16"][-1]["h2d_bytes"]), "f32": int(stats["f32"][-1]["h2d_bytes"])}
    res.update({f"{prefix}_over_simple_bytes": round(ratio, 4), "host_decode_ms_per_row": benchlib.median_and_min(dec),
                "bits_equal_simple_packed": True})
    res["decoded_road_ms"] = round(benchlib.median(dec) * rows + ms["f32"], 1)       # one-thread decode of every row + apply_host
    res[f"grib16_over_{leg}"] = round(ms["grib16"] / ms[leg], 3)
    res[f"decoded_road_over_{leg}"] = round(res["decoded_road_ms"] / ms[leg], 2)
    return res


def _in_device(codec, op, rows):
    from smmregrid_amd import DeviceArray
    S = op.n_src
    (cbuf, crows, recs), (sbuf, srows), field, _, _, _, _ = make_coded_streams(codec, S, rows)
    out = DeviceArray((IN[codec.name]["out_bytes"](S) * rows,), np.uint8)
    return padded_upload(cbuf), cbuf.size, crows, recs, padded_upload(sbuf), sbuf.size, srows, field, out


def in_kernel(codec, op, name, rows, steps, warmup):
    from smmregrid_amd import DeviceArray, GribEncode, grib_pack, to_device
    d, unpack = IN[codec.name], unpack_of(codec)
    S, D_ = op.n_src, op.n_dst
    if d["kernel_rows"]:
        rows = min(rows, d["kernel_rows"])                   # 4 B of scratch per sample: a chunk's worth of rows
    dc, c_bytes, crows, recs, ds, s_bytes, srows, field, out = _in_device(codec, op, rows)
    y, y_s = DeviceArray((rows, D_), np.float64), DeviceArray((rows, D_), np.float64)
    _, rows_out = unpack(dc, crows, recs, x_bytes=c_bytes, out=out)
    legs = {"transcode": lambda: unpack(dc, crows, recs, x_bytes=c_bytes, out=out),
            "gather_of_transcoded": lambda: op.apply_grib(out, rows_out, y=y),
            "gather_of_simple": lambda: op.apply_grib(ds, srows, x_bytes=s_bytes, y=y_s)}
    if d["extras"]:
        pack_rows = min(rows, 32)                            # float64 values of that many rows (8 B each on host and device)
        values, enc = to_device(field[:pack_rows].astype(np.float64)), GribEncode(NBITS, 0)
        legs["grib_pack"] = lambda: grib_pack(values, enc)

    def bits():
        n = d["compare_rows"]
        a, b = (y.rows(0, n), y_s.rows(0, n)) if n else (y, y_s)
        if not benchlib.same_bits(a.to_host(), b.to_host()):
            raise SystemExit(f"{name}: the gather of the transcoded streams differs from the gather of the simple-packed ones")
    res = {"block": "kernel", "op": name, "rows": rows, "n_src": S, "n_dst": D_, "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup, after_first=bits), 4)}
    ms = res["ms"]
    res["transcode_over_gather"] = round(ms["transcode"] / ms["gather_of_transcoded"], 3)
    if d["extras"]:
        res.update({"grib_pack_rows": pack_rows,
                    "transcode_over_grib_pack_per_row": round((ms["transcode"] / rows) / (ms["grib_pack"] / pack_rows), 3),
                    "transcode_gvalues_per_s": round(rows * S / ms["transcode"] / 1e6, 2)})
    res["coded_bytes"] = int(recs["byte_len"].sum())
    if d["extras"]:
        res["stored_width"] = int(rows_out["nbits"][0])
    res["bits_equal_simple_packed"] = True
    return res


def in_profile_run(codec, op, rows):
    dc, c_bytes, crows, recs, _, _, _, _, out = _in_device(codec, op, rows)
    for _ in range(4):
        unpack_of(codec)(dc, crows, recs, x_bytes=c_bytes, out=out)


def in_parser(codec, doc):
    """the options of a coded-input tool; --profile-run where the codec's tool has it"""
    ap = benchlib.parser(doc, steps=5, warmup=1, only="cfg2,cfg4", blocks="host,kernel",
                         out=f"grib_{IN[codec.name]['leg'][:-2]}_bench.jsonl")
    ap.add_argument("--chunk-rows", type=int, default=0)
    if IN[codec.name]["extras"]:
        ap.add_argument("--profile-run", action="store_true")
    return ap


def in_run(codec, args):
    for name, op, rows in benchlib.operators(args):
        if getattr(args, "profile_run", False):
            in_profile_run(codec, op, rows)
            continue
        for block in benchlib.split(args.blocks):
            benchlib.emit(in_host(codec, op, name, rows, args.steps, args.warmup, args.chunk_rows) if block == "host" else
                          in_kernel(codec, op, name, rows, args.steps, args.warmup), args.out)


# ------------------------------------------------------------------------------------------------ coded results
# per codec, what its result tool measured beside the common legs:
#   leg         the device pack step and its leg's name          short   that step in the result's keys
#   word        what the coded bytes are called in the keys      rate    what a value is called in the rate
#   pack_coded  the kernel block's grib_pack runs under the coded rule, not the plain one
#   beside      a second codec whose pack step runs on the same rows, for the comparison
#   host        the coded leg of the host block    float64_leg   the same call without grib_out runs beside it
#   h2d         the host block reports the bytes shipped up
OUT = {"ccsds": dict(leg="grib_aec_pack", short="aec_pack", word="coded", rate="samples_per_us", pack_coded=True, beside=None,
                     host="ccsds", float64_leg=False, h2d=True),
       "cpx": dict(leg="grib_cpx_pack", short="cpx_pack", word="cpx", rate="values_per_us", pack_coded=False, beside="ccsds",
                   host="cpx", float64_leg=True, h2d=False)}


def pack_of(codec):
    import smmregrid_amd
    return getattr(smmregrid_amd, OUT[codec.name]["leg"])


def sample_rows(field, idx):
    from smmregrid_amd import GribField
    return GribField(field.buf, field.rows[idx], (len(idx), field.n_points), field.n_points, bitmaps=field.bitmaps[idx],
                     ccsds=None if field.ccsds is None else field.ccsds[idx],
                     cpx=None if field.cpx is None else field.cpx[idx]).decode()


def packed_result(codec, op, rows, enc):
    """the source on the device, its gather's result and that result simple-packed under the rule enc"""
    from smmregrid_amd import DeviceArray, grib_pack, to_device
    buf, table = source(op.n_src, rows, SEEDS[codec.name])
    x = to_device(buf)
    y = DeviceArray((rows, op.n_dst), np.float64)
    op.apply_grib(x, table, y=y)
    packed, rows_p, bms = grib_pack(y, enc)
    simple = int(sum((op.n_dst * int(w) + 7) // 8 for w in rows_p["nbits"]))
    return x, table, y, packed, rows_p, bms, simple


def coded_step(codec, enc, op, rows, packed, rows_p, bms):
    """(the pack leg, the bound buffer, the coded result of one call) of `codec` under the rule enc"""
    from smmregrid_amd import DeviceArray
    want = enc.coded_records(rows, bms["n_values"], rows_p["nbits"], codec=codec)
    bound = DeviceArray((max(int(enc.coded_bounds(op.n_dst, rows, codec).sum()), 4),), np.uint8)
    pack = pack_of(codec)
    return (lambda: pack(packed, rows_p, want, out=bound)), bound, pack(packed, rows_p, want, out=bound)


def out_kernel(codec, op, name, rows, width, steps, warmup):
    from smmregrid_amd import GribEncode, GribField, grib_pack
    from smmregrid_amd.griblite import CODECS
    d = OUT[codec.name]
    beside = {c.name: c for c in CODECS}.get(d["beside"])
    enc = GribEncode(width, 0, **{codec.name: True})
    plain = enc if d["pack_coded"] else GribEncode(width, 0)
    x, table, y, packed, rows_p, bms, simple = packed_result(codec, op, rows, plain)
    leg, bound, (coded, rows_c, recs) = coded_step(codec, enc, op, rows, packed, rows_p, bms)
    idx = sorted({0, 1, rows - 1})
    got = sample_rows(GribField(coded.to_host(), rows_c, (rows, op.n_dst), op.n_dst, bitmaps=bms, **{codec.name: recs}), idx)
    ref = sample_rows(GribField(packed.to_host(), rows_p, (rows, op.n_dst), op.n_dst, bitmaps=bms), idx)
    if not np.array_equal(got.view(np.uint32), ref.view(np.uint32)):
        raise SystemExit(f"{name}: the coded result decodes to other bits than the simple-packed one")
    legs = {"gather": lambda: op.apply_grib(x, table, y=y), "grib_pack": lambda: grib_pack(y, plain, out=packed), d["leg"]: leg}
    if beside:
        b = OUT[beside.name]
        legs[b["leg"]], _, (_, _, recs_b) = coded_step(beside, GribEncode(width, 0, **{beside.name: True}), op, rows, packed, rows_p, bms)
    res = {"block": "kernel", "op": name, "rows": rows, "nbits": width, "n_src": op.n_src, "n_dst": op.n_dst, "steps": steps,
           **benchlib.summary(benchlib.time_events(legs, steps, warmup), 4)}
    ms, used, short, word = res["ms"], int(recs["byte_len"].sum()), d["short"], d["word"]
    if beside:
        res[f"{short}_over_{b['short']}"] = round(ms[d["leg"]] / ms[b["leg"]], 3)
    res[f"{short}_over_grib_pack"] = round(ms[d["leg"]] / ms["grib_pack"], 3)
    res[f"{short}_over_gather"] = round(ms[d["leg"]] / ms["gather"], 3)
    res.update({f"{word}_bytes": used, "simple_bytes": simple, "bound_bytes": bound.nbytes,
                f"{word}_over_simple_bytes": round(used / max(simple, 1), 4)})
    if beside:
        used_b = int(recs_b["byte_len"].sum())
        res.update({f"{beside.name}_bytes": used_b, f"{word}_over_{beside.name}_bytes": round(used / max(used_b, 1), 4)})
    if "order" in recs.dtype.names:
        res["orders_coded"] = sorted(set(recs["order"].tolist()))
    res[d["rate"]] = round(rows * op.n_dst / (ms[d["leg"]] * 1e3), 1)
    res["bits_equal_simple_packed"] = True
    return res


def out_host(codec, op, name, rows, width, steps, warmup):
    from smmregrid_amd import GribEncode, _lib
    key, float64_leg, h2d = (OUT[codec.name][k] for k in ("host", "float64_leg", "h2d"))
    buf, table = source(op.n_src, rows, SEEDS[codec.name])
    simple_enc, coded_enc = GribEncode(width, 0), GribEncode(width, 0, **{codec.name: True})
    legs = {key: lambda: op.apply_host_grib(buf, table, grib_out=coded_enc),
            "simple": lambda: op.apply_host_grib(buf, table, grib_out=simple_enc)}
    if float64_leg:
        legs["float64"] = lambda: op.apply_host_grib(buf, table)
    first = {}

    def bits():
        idx = sorted({0, 1, rows - 1})
        if not np.array_equal(sample_rows(first[key], idx).view(np.uint32), sample_rows(first["simple"], idx).view(np.uint32)):
            raise SystemExit(f"{name}: the coded result decodes to other bits than the simple-packed one")
    times, stats = benchlib.time_wall(legs, steps, warmup, host_stats=_lib.host_stats, check=first.__setitem__, after_first=bits,
                                      announce=f"# {name} {width} bits: host step {{}}")
    # the coded road is a Python chunk loop: its bytes are those of its result and of every row staged and shipped
    d2h = {k: int(first[k].buf.size) if k == key else int(stats[k][-1]["d2h_bytes"]) for k in legs}
    res = {"block": "host_to_host", "op": name, "rows": rows, "nbits": width, "n_src": op.n_src, "n_dst": op.n_dst,
           "steps": steps, **benchlib.summary(times, 3)}
    ms = res["ms"]
    if h2d:
        staged = int(sum((op.n_src * int(w) + 7) // 8 + (-((op.n_src * int(w) + 7) // 8)) % 4 for w in table["nbits"]))
        res["h2d_bytes"] = {k: staged if k == key else int(stats[k][-1]["h2d_bytes"]) for k in legs}
    res.update({"d2h_bytes": d2h, "float64_bytes": rows * op.n_dst * 8, f"{key}_over_simple_ms": round(ms[key] / ms["simple"], 3)})
    if float64_leg:
        res[f"{key}_over_float64_ms"] = round(ms[key] / ms["float64"], 3)
    res[f"{key}_over_simple_d2h_bytes"] = round(d2h[key] / max(d2h["simple"], 1), 4)
    res["bits_equal_simple_packed"] = True
    return res
