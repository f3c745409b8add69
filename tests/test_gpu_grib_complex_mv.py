"""Complex-packed GRIB-2 fields whose missing values are coded inside the groups (missing value management 1 / 2) on the
GPU: smm_grib_cpx_unpack_mv (`grib_unpack_cpx_mv`) and the gather behind it (`apply_grib(cpx=, cpx_missing=)`,
`apply_host_grib(cpx=, cpx_missing=)`).  Every comparison is bit for bit: against the cases' integers and bitmaps
(tests/complex_mv_cases.py, coded by its numpy encoder) and against the same call on the simple-packed twin -- the
compacted integers at their own width plus the bitmap.  Malformed streams are the business of
tests/test_grib_complex_mv.py and its host harness."""
import numpy as np
import pytest

from smmregrid_amd import GRIB_CPX_DTYPE, GRIB_NO_BITMAP, _lib, grib_unpack_cpx, grib_unpack_cpx_mv, to_device
from tests import ccsds_cases as cc
from tests import complex_cases as xc
from tests import complex_mv_cases as mv
from tests.test_gpu_grib_complex import device_bytes, operator, same_bits

pytestmark = pytest.mark.gpu
SENTINEL = 0xC3


def all_cases_call():
    """Every case as a row of one call, streams at odd offsets with garbage between them: (buf, rows, records, missing,
    cases)."""
    cs = mv.cases()
    rows = cc.rules(len(cs), seed=2)
    recs = np.zeros(len(cs), dtype=GRIB_CPX_DTYPE)
    parts, at = [], 0
    for i, c in enumerate(cs):
        pad = 1 + 2 * (i % 2)
        parts.append(np.full(pad, 0xA5, np.uint8))
        at += pad
        rows["nbits"][i] = c.params["nbits"]
        recs[i] = c.record(at)
        parts.append(c.stream)
        at += c.stream.size
    return np.concatenate(parts), rows, recs, np.array([c.m for c in cs], dtype=np.uint8), cs


def check_unpacked(host, rows, rows_out, bitmaps_out, cs):
    """Slots, bitmap slots and both record tables against the numpy decode; what the contract does not write keeps the
    sentinel.  Returns the layout's end."""
    end = 0
    for i, c in enumerate(cs):
        r, b = rows_out[i], bitmaps_out[i]
        assert (r["ref"], r["bscale"], r["ddiv"]) == (rows[i]["ref"], rows[i]["bscale"], rows[i]["ddiv"]), c
        assert int(r["nbits"]) == c.width, (c, int(r["nbits"]), c.width)
        off, bm_off = int(r["byte_off"]), int(b["bitmap_off"])
        assert off == end and bm_off == off + 4 * c.n_values and int(b["n_values"]) == c.P, (c, off, bm_off, end, b)
        assert np.array_equal(host[off:off + c.packed.size], c.packed), c
        assert (host[off + c.packed.size:bm_off] == SENTINEL).all(), c          # the rest of the slot is not touched
        assert np.array_equal(host[bm_off:bm_off + c.bitmap_slot.size], c.bitmap_slot), c
        end = bm_off + c.bitmap_slot.size
    return end


def test_grib_unpack_cpx_mv_gives_every_cases_integers_and_bitmap_in_one_call(hip):
    buf, rows, recs, missing, cs = all_cases_call()
    total = sum(4 * c.n_values + c.bitmap_slot.size for c in cs)
    filled = to_device(np.full(total + 64, SENTINEL, dtype=np.uint8))
    out, rows_out, bitmaps_out = grib_unpack_cpx_mv(device_bytes(buf), rows, recs, missing, x_bytes=buf.size, out=filled)
    host = out.to_host()
    assert check_unpacked(host, rows, rows_out, bitmaps_out, cs) == total
    assert (host[total:] == SENTINEL).all()
    assert {0, 32} <= {int(w) for w in rows_out["nbits"]} and {0, 1, 2, mv.S} <= {int(p) for p in bitmaps_out["n_values"]}


def test_grib_unpack_cpx_mv_with_split_launch_grids_gives_the_same_bytes(hip):
    """smm_debug_set_grid_limit(61): every kernel's grid is cut into launches of at most 61 workgroups (a 70000-value row
    alone needs 274), rows and blocks falling on either side of a cut."""
    buf, rows, recs, missing, cs = all_cases_call()
    x = device_bytes(buf)
    total = sum(4 * c.n_values + c.bitmap_slot.size for c in cs)
    _lib.call("smm_debug_set_grid_limit", 61)
    try:
        cut, rows_cut, bm_cut = grib_unpack_cpx_mv(x, rows, recs, missing, x_bytes=buf.size,
                                                   out=to_device(np.full(total, SENTINEL, dtype=np.uint8)))
        cut = cut.to_host()
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    assert check_unpacked(cut, rows, rows_cut, bm_cut, cs) == total


def test_rows_without_missing_values_keep_their_bytes_in_a_mixed_call(hip):
    """mvm 0, 1 and 2 and a row marked simple-packed in one call: the mvm-0 rows' slots hold what grib_unpack_cpx gives
    for those rows alone, and their bitmap records say "none"."""
    plain = [xc.case(n) for n in ("order2_noct3", "order0_widths_0_1_31_32", "order1_noct2")]
    coded = [mv.case(n) for n in ("order2_third_m1", "order1_edge_runs_m2")]
    order = [plain[0], coded[0], None, plain[1], coded[1], plain[2]]
    rows = cc.rules(len(order), seed=4)
    recs = np.zeros(len(order), dtype=GRIB_CPX_DTYPE)
    missing = np.array([0, 1, 2, 0, 2, 0], dtype=np.uint8)          # the marked row's value is not looked at
    parts, at = [], 0
    for i, c in enumerate(order):
        parts.append(np.full(3, 0xA5, np.uint8))
        at += 3
        if c is None:
            rows["nbits"][i], rows["byte_off"][i], recs[i] = 12, 12345, xc.simple_record()
            continue
        rows["nbits"][i], recs[i] = c.params["nbits"], c.record(at)
        parts.append(c.stream)
        at += c.stream.size
    buf = np.concatenate(parts)
    x = device_bytes(buf)
    out, rows_out, bms = grib_unpack_cpx_mv(x, rows, recs, missing, x_bytes=buf.size)
    host = out.to_host()
    idx = [0, 3, 5]
    alone, rows_alone = grib_unpack_cpx(x, rows[idx], recs[idx], x_bytes=buf.size)
    alone = alone.to_host()
    for k, i in enumerate(idx):
        c = order[i]
        a, b = int(rows_out["byte_off"][i]), int(rows_alone["byte_off"][k])
        written = (c.n_values * c.width + 7) // 8
        assert np.array_equal(host[a:a + written], alone[b:b + written]) and int(rows_out["nbits"][i]) == int(rows_alone["nbits"][k])
        assert int(bms["bitmap_off"][i]) == GRIB_NO_BITMAP and int(bms["n_values"][i]) == c.n_values
    assert rows_out[2].tobytes() == rows[2].tobytes() and int(bms["bitmap_off"][2]) == GRIB_NO_BITMAP
    for i in (1, 4):
        c = order[i]
        a, b = int(rows_out["byte_off"][i]), int(bms["bitmap_off"][i])
        assert np.array_equal(host[a:a + c.packed.size], c.packed) and int(bms["n_values"][i]) == c.P
        assert np.array_equal(host[b:b + c.bitmap_slot.size], c.bitmap_slot)
    # and with missing=None the call is grib_unpack_cpx on the same rows
    out0, rows0, bms0 = grib_unpack_cpx_mv(x, rows[idx], recs[idx], None, x_bytes=buf.size)
    assert rows0.tobytes() == rows_alone.tobytes() and (bms0["bitmap_off"] == GRIB_NO_BITMAP).all()


ROWS = ["order2_third_m1", "order1_third_m2", "order0_third_m1", "order2_none_missing_m2", "all_missing_nbits5_m1", "order2_P1_m2",
        "order2_first3_missing_m1", "order1_edge_runs_m2", "order0_width32_group_m1", "order0_width0_present_and_missing_m2"]


@pytest.mark.parametrize("skipna", [False, True])
def test_apply_grib_and_apply_host_grib_have_the_bits_of_the_simple_packed_twin(hip, skipna):
    """B = 10 rows of 2048 positions in one call, plain and under skipna, masked on and off; the host form with
    chunk_rows=3 (four chunks).  The twin: the compacted integers at their own width plus the bitmap."""
    op = operator()
    (buf, rows, cpx, missing), (tbuf, trows, tbms) = mv.build([mv.case(n) for n in ROWS])
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
        want = op.apply_grib(device_bytes(tbuf), trows, x_bytes=tbuf.size, bitmaps=tbms, **common).to_host()
        assert np.isfinite(want).any() and np.isnan(want).any()
        got = op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, cpx=cpx, cpx_missing=missing, **common).to_host()
        same_bits(got, want, f"apply_grib {common}")
        for chunk_rows in (0, 3):
            got = op.apply_host_grib(buf, rows, cpx=cpx, cpx_missing=missing, chunk_rows=chunk_rows, **common)
            same_bits(got, want, f"apply_host_grib chunk_rows={chunk_rows} {common}")


# ------------------------------------------------------------------------------------------------ Regridder
FILE_ROWS = ["order2_third_m1", "order1_third_m2", "order0_width32_group_m2"]
FILE_RULES = [(270.0, -4, 0), (0.0, 2, 2), (-12.5, -6, 1)]


@pytest.fixture(scope="module")
def mv_file(tmp_path_factory):
    """Three levels with missing values inside their groups and one plain complex-packed level."""
    fields = []
    for k, (name, (R, E, D)) in enumerate(zip(FILE_ROWS, FILE_RULES)):
        c = mv.case(name)
        fields.append(dict(cpx=(c.stream, c.params, c.n_values), s5=xc.section5(c.n_values, c.params, R, E, D, mvm=c.m),
                           level=(85000, 50000, 25000)[k]))
    plain = xc.case("order1_noct2")
    path = str(tmp_path_factory.mktemp("complex_mv") / "t_mv.grib2")
    with open(path, "wb") as fh:
        fh.write(xc.grib2_message(fields) + xc.grib2_message([dict(cpx=(plain.stream, plain.params, plain.n_values), level=10000)]))
    return path


def test_regridder_ships_a_variable_with_missing_values_inside_its_groups_raw(hip, mv_file, caplog, monkeypatch):
    from smmregrid_amd import CdoGenerate, GribEncode, GribField, Regridder
    from smmregrid_amd.io import open_dataset
    from smmregrid_amd.lazy import LazyArray
    dec = open_dataset(mv_file, cpx_missing=True)
    raw = open_dataset(mv_file, decode=False, cpx_missing=True)
    src = raw["t"].data
    assert isinstance(src, GribField) and src.cpx_missing.tolist() == [0, 2, 2, 1] and np.isnan(dec["t"].values).any()
    w = CdoGenerate(dec["t"], "r16x8").weights(method="con")
    want = Regridder(weights=w).regrid(dec["t"])
    assert want.dtype == np.float64 and np.isfinite(want.values).any() and np.isnan(want.values).any()
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, loglevel="INFO").regrid(raw["t"])
    assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
    assert names.count("smm_grib_cpx_unpack_mv") == 1 and names.count("smm_apply_grib_bm") == 1
    assert "smm_grib_cpx_decode_host_mv" not in names and "smm_apply_host" not in names
    same_bits(got.values, want.values, "packed=True")
    assert got.dims == want.dims
    want_na = Regridder(weights=w, skipna=True).regrid(dec["t"])
    del names[:]
    got_na = Regridder(weights=w, packed=True, skipna=True, packed_skipna=True).regrid(raw["t"])
    assert names.count("smm_grib_cpx_unpack_mv") == 1 and names.count("smm_apply_grib_na") == 1
    same_bits(got_na.values, want_na.values, "skipna")
    lazy = Regridder(weights=w, packed=True, lazy=True).regrid(raw["t"])
    assert isinstance(lazy.data, LazyArray)
    same_bits(np.asarray(lazy.values), want.values, "lazy")
    # the result complex-packed: bytewise GribEncode.encode of the float64 result at the widths the unpack reported
    del names[:]
    out = Regridder(weights=w, packed=True, grib_out=True, grib_out_cpx=True).regrid(raw["t"]).data
    assert isinstance(out, GribField) and out.cpx is not None and out.cpx_missing is None and out.bitmaps is not None
    assert names.count("smm_grib_cpx_unpack_mv") == 1 and names.count("smm_grib_cpx_pack") == 1
    widths = [xc.case("order1_noct2").width] + [mv.case(n).width for n in reversed(FILE_ROWS)]          # level ascending
    enc = GribEncode.from_field(src, cpx=True).resolved(widths).encode(want.values.reshape(4, -1))
    assert out.buf.tobytes() == enc.buf.tobytes() and out.rows.tobytes() == enc.rows.tobytes()
    assert out.cpx.tobytes() == enc.cpx.tobytes() and out.bitmaps.tobytes() == enc.bitmaps.tobytes()


# ------------------------------------------------------------------------------------------------ far offsets
from tests import far_cases as fc  # noqa: E402
from tests.test_gpu_far_offsets import far  # noqa: E402,F401
from tests.test_gpu_grib_far_offsets import P32, byte_view, decoy_bytes, guarded_tail, scratch, sentinel_bytes  # noqa: E402


def _one_more(case):
    """The stream of `case` (order 2, three octets per descriptor) with h_1 and h_2 one larger: the same record shape and
    bitmap, every integer one larger -- what a narrowed offset of the far row would decode instead."""
    s = case.stream.copy()
    assert case.order == 2 and case.params["n_oct"] == 3 and s[2] < 255 and s[5] < 255
    s[2] += 1
    s[5] += 1
    X, present = mv.numpy_decode(s, case.n_values, case.params, case.m)
    assert np.array_equal(X, case.X + 1) and np.array_equal(present, case.present)
    return s


def test_cpx_unpack_mv_far(far):  # noqa: F811
    """Modelled on test_cpx_unpack_input_far.  Row 2, order2_third_m1, has its stream at an odd offset past 2^32 bytes of
    x (ending in the buffer's last word), with a stream of the same shape and other integers where that offset lands mod
    2^32; its slot and its bitmap slot lie past 2^32 bytes of out, behind the spacer row 1: 2^30 + 1024 positions under
    mvm 1 in one group of width 32 with no tables -- its stream is the first 2^32 + 4096 bytes of x themselves, decoys
    and streams alike, as 32-bit samples (a few words of the streams are the code 0xFFFFFFFF: missing).  The spacer also puts row 2's entries in the
    second scratch array and in the values past 2^33 bytes.  Row 0, order1_edge_runs_m2, is near.  The spacer is checked
    in windows: its first and last 4096 values, the values where row 2's slot and bitmap slot land mod 2^32, its bitmap's
    ends, the sentinel behind its integers."""
    near, true = mv.case("order1_edge_runs_m2"), mv.case("order2_third_m1")
    n_sp = (1 << 30) + 1024
    at_near, at_alias = 4096 + 1, 65536 + 1
    at_true = P32 + at_alias
    x_bytes = at_true + true.stream.size
    assert 4 * n_sp <= x_bytes and at_alias + true.stream.size < 4 * n_sp
    xa = decoy_bytes(far, x_bytes, [(at_near, near.stream), (at_alias, _one_more(true)), (at_true, true.stream)], seed=13)
    x = byte_view(xa)
    rows = cc.rules(3, seed=2)
    recs = np.zeros(3, dtype=GRIB_CPX_DTYPE)
    recs[0], recs[2] = near.record(at_near), true.record(at_true)
    spacer = dict(n_groups=1, nbits=0, width_ref=32, width_bits=0, length_ref=n_sp, length_inc=1, length_last=n_sp, length_bits=0,
                  order=0, n_oct=0)
    recs[1] = xc.record(0, 4 * n_sp, n_sp, spacer)
    rows["nbits"] = (near.params["nbits"], 0, true.params["nbits"])
    missing = np.array([near.m, 1, true.m], dtype=np.uint8)
    off = [0, 8192 + 256, 8192 + 256 + 4 * n_sp + n_sp // 8]             # the slots; a bitmap slot lies behind its row's
    bm = [8192, off[1] + 4 * n_sp, off[2] + 8192]
    total = bm[2] + 256
    assert off[2] > P32 and n_sp % 32 == 0
    out = sentinel_bytes(far, total + fc.GUARD)
    scratch(far, 17 * n_sp)
    _, rows_out, bms = grib_unpack_cpx_mv(x, rows, recs, missing, x_bytes=x_bytes, out=out)
    assert rows_out["byte_off"].tolist() == off and bms["bitmap_off"].tolist() == bm
    assert [int(bms["n_values"][i]) for i in (0, 2)] == [near.P, true.P]
    for i, c in ((0, near), (2, true)):
        assert int(rows_out["nbits"][i]) == c.width
        assert np.array_equal(byte_view(out, off[i], c.packed.size).to_host(), c.packed), c
        assert (byte_view(out, off[i] + c.packed.size, 4 * c.n_values - c.packed.size).to_host() == fc.SENTINEL).all(), c
        assert np.array_equal(byte_view(out, bm[i], c.bitmap_slot.size).to_host(), c.bitmap_slot), c
    guarded_tail(byte_view(out, total - 256, 256 + fc.GUARD), 256, "smm_grib_cpx_unpack_mv")
    # the spacer: the streams that lie in its first bytes hold runs of one bits -- words that are its code, missing
    # positions -- so every later value's rank is its position less k
    w = int(rows_out["nbits"][1])
    assert 31 <= w <= 32
    head_words = (at_alias + true.stream.size) // 4 + 1
    head = byte_view(xa, 0, 4 * head_words).to_host().view(">u4").astype(np.int64)
    gone = head == 0xFFFFFFFF
    k = int(gone.sum())
    P = n_sp - k
    assert int(bms["n_values"][1]) == P and head_words - k >= 4096

    def samples(rank):
        """4096 of the spacer's present values from `rank` on"""
        if rank == 0:
            return head[~gone][:4096]
        assert rank >= head_words
        return byte_view(xa, 4 * (rank + k), 4 * 4096).to_host().view(">u4").astype(np.int64)
    landing = [(q % P32 - off[1]) * 8 // w // 8 * 8 for q in (off[2], bm[2])]
    for a in [0, (P - 4096) // 8 * 8] + landing:
        assert a + 4096 <= P
        want = cc.pack_bits(samples(a), w)
        assert np.array_equal(byte_view(out, off[1] + a * w // 8, want.size).to_host(), want), a
    used = (P * w + 7) // 8
    if used + 4096 <= 4 * n_sp:
        assert (byte_view(out, off[1] + (used + 3) // 4 * 4, 4096).to_host() == fc.SENTINEL).all()
    first = np.ones(8 * 4096, dtype=np.uint8)
    first[:head_words] = ~gone
    assert np.array_equal(byte_view(out, bm[1], 4096).to_host(), np.packbits(first))
    assert (byte_view(out, bm[1] + n_sp // 8 - 4096, 4096).to_host() == 0xFF).all()
