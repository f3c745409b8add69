"""The CCSDS encoder on the CPU (THE RULE OF THIS ENCODER in smm_grib_aec.hpp): smm_grib_aec_encode_host /
`griblite.aec_encode` round-tripped through the host decoder -- which is pinned against libaec and therefore the arbiter
-- on the fixtures of tests/golden/ccsds and on hand-built edge cases; the sizes against the bound and against libaec's
own streams; the refusals of the three entries; `GribEncode(..., ccsds=)`; and encode_row then decode_row in a stand-alone
program under AddressSanitizer + UBSan (tests/cpp/grib_aec_encode_harness.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from smmregrid_amd import GRIB_AEC_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribEncode, GribField, Regridder, _lib, aec_encode
from tests import ccsds_cases as cc
from tests import ccsds_encode_cases as ec

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = cc.fixtures()
EDGES = ec.edge_cases()
_STREAMS = {}


def encoded(case):
    """(stream, the encoder's histogram) of a fixture or an edge case; coded once."""
    if case.name not in _STREAMS:
        hist = cc.new_histogram()
        _STREAMS[case.name] = (aec_encode(case.values, cc.record(0, 0, 0, case.nbits, case.block, case.rsi, case.flags), hist), hist)
    return _STREAMS[case.name]


def bound_of(case):
    blocks = -(-case.n_values // case.block)
    id_len = 3 if case.nbits <= 8 else 4 if case.nbits <= 16 else 5
    return (-(-(blocks * (id_len + case.block * case.nbits)) // 8) + 3) // 4 * 4


def test_there_are_33_fixtures():
    assert len(FIXTURES) == 33


@pytest.mark.parametrize("case", FIXTURES + EDGES, ids=repr)
def test_round_trip_through_the_host_decoder(case):
    """What the encoder writes the decoder reads back exactly, status ok (a bad status raises), with the histogram the
    encoder counted; the stream is within the bound; libaec, where it is installed, reads the same integers."""
    stream, hist = encoded(case)
    back_hist = cc.new_histogram()
    back = cc.host_decode(stream, case.n_values, case.nbits, case.block, case.rsi, case.flags, back_hist)
    assert back.dtype == np.uint32 and np.array_equal(back, case.values)
    assert np.array_equal(hist, back_hist)
    assert stream.size <= bound_of(case)
    if cc.load_libaec() is not None:
        assert np.array_equal(cc.aec_decode_libaec(stream, case.n_values, case.nbits, case.block, case.rsi, case.preprocess),
                              case.values)


def test_the_streams_are_no_longer_than_libaecs():
    """An exhaustive search over k cannot lose to libaec's neighbour search on the same blocks."""
    ours = sum(encoded(fx)[0].size for fx in FIXTURES)
    theirs = sum(fx.stream.size for fx in FIXTURES)
    assert ours <= theirs, (ours, theirs)


@pytest.mark.parametrize("case", [c for c in EDGES if c.hist is not None], ids=repr)
def test_edge_cases_take_the_expected_options(case):
    back_hist = cc.new_histogram()
    cc.host_decode(encoded(case)[0], case.n_values, case.nbits, case.block, case.rsi, case.flags, back_hist)
    for name, got, want in zip(_lib.GRIB_AEC_OPTIONS, back_hist.tolist(), case.hist):
        assert want is None or got == want, (case, name, back_hist.tolist(), case.hist)


def test_the_edge_cases_take_every_option():
    hist = cc.new_histogram()
    for case in EDGES:
        cc.host_decode(encoded(case)[0], case.n_values, case.nbits, case.block, case.rsi, case.flags, hist)
    assert (hist > 0).all(), dict(zip(_lib.GRIB_AEC_OPTIONS, hist.tolist()))


def test_zero_runs_are_coded_as_the_rule_says():
    """fs = 3 for a run of 4 at a segment's end, ROS (fs = 4) for a run of 5 there: read from the bits.  8-bit samples,
    J = 8: the ID has 3 bits and a zero run is 000 0 then the FS code."""
    def last_run(pattern):
        noise = np.arange(1, 600, dtype=np.uint32) % 200 + 1
        q = ec._blocks(pattern, 8, noise)
        stream = aec_encode(q, cc.record(0, 0, 0, 8, 8, 128, 0))
        bits = np.unpackbits(stream)
        # the stream ends with the run: ID 000, selector 0, fs zeros, a one, then the pad to a byte
        end = int(np.flatnonzero(bits)[-1])
        fs = 0
        while bits[end - 1 - fs] == 0:
            fs += 1
        return fs - 4
    assert last_run("N" * 60 + "Z" * 4) == 3
    assert last_run("N" * 59 + "Z" * 5) == 4
    assert last_run("N" * 58 + "Z" * 6) == 4
    assert last_run("N" * 50 + "Z" * 6) == 6          # ends with the data, not with the segment


# ------------------------------------------------------------------------------------------------ refusals
def _rec(**kw):
    r = np.zeros(1, dtype=GRIB_AEC_DTYPE)
    r["n_values"], r["nbits"], r["block_size"], r["rsi"], r["flags"] = 100, 12, 32, 128, 8
    for k, v in kw.items():
        r[k] = v
    return r


_ap = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribAecStruct))               # noqa: E731
BAD_RECORDS = [dict(nbits=-1), dict(nbits=33), dict(block_size=0), dict(block_size=12), dict(block_size=128), dict(rsi=0),
               dict(rsi=4097), dict(flags=8 | 1), dict(flags=8 | 16), dict(flags=8 | 32), dict(flags=8 | 64), dict(reserved=1),
               dict(n_values=2 ** 31)]


@pytest.mark.parametrize("kw", BAD_RECORDS, ids=lambda kw: ",".join(kw))
def test_the_three_entries_refuse_a_bad_record(kw):
    lib, rec, total, used = _lib.load(), _rec(**kw), ctypes.c_uint64(0), ctypes.c_uint64(0)
    assert lib.smm_grib_aec_pack_bound(_ap(rec), 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    assert b"recs[0]" in lib.smm_last_error()
    assert _pack_status(rec) == _lib.SMM_ERR_INVALID
    values, out = np.zeros(100, np.uint32), np.zeros(4096, np.uint8)
    assert lib.smm_grib_aec_encode_host(values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), 100, _ap(rec),
                                        ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID


def test_bound_entry():
    lib = _lib.load()
    recs = np.concatenate([_rec(n_values=5, nbits=12, block_size=8), _rec(nbits=0, block_size=0, rsi=0), _rec(n_values=2048, nbits=17),
                           _rec(n_values=0)])
    offs, total = np.zeros(4, np.uint64), ctypes.c_uint64(0)
    assert lib.smm_grib_aec_pack_bound(_ap(recs), 4, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(total)) == 0
    first = (-(-(4 + 8 * 12) // 8) + 3) // 4 * 4                       # one block of 4 + 96 bits: 13 bytes, 16
    third = (-(-(64 * (5 + 32 * 17)) // 8) + 3) // 4 * 4
    assert offs.tolist() == [0, first, first, first + third] and total.value == first + third
    assert lib.smm_grib_aec_pack_bound(_ap(recs), 4, None, None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_pack_bound(None, 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_pack_bound(_ap(recs), -1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID


def test_encode_host_refusals():
    lib, rec, used = _lib.load(), _rec(), ctypes.c_uint64(0)
    values, out = np.arange(100, dtype=np.uint32), np.zeros(4096, np.uint8)
    vp, op = values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_void_p(out.ctypes.data)
    bound = (-(-(4 * (4 + 32 * 12)) // 8) + 3) // 4 * 4
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), op, bound, ctypes.byref(used), None) == 0 and 0 < used.value <= bound
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), op, bound - 1, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert b"bound" in lib.smm_last_error()
    assert lib.smm_grib_aec_encode_host(vp, 99, _ap(rec), op, bound, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_encode_host(None, 100, _ap(rec), op, bound, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_encode_host(vp, 100, None, op, bound, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), None, bound, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), op, bound, None, None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), op, -1, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    values[7] = 4096                                                    # does not fit into 12 bits
    assert lib.smm_grib_aec_encode_host(vp, 100, _ap(rec), op, bound, ctypes.byref(used), None) == _lib.SMM_ERR_INVALID
    assert b"values[7]" in lib.smm_last_error()
    # a constant field and an empty one have no stream
    assert lib.smm_grib_aec_encode_host(None, 100, _ap(_rec(nbits=0)), None, 0, ctypes.byref(used), None) == 0 and used.value == 0
    assert lib.smm_grib_aec_encode_host(None, 0, _ap(_rec(n_values=0)), None, 0, ctypes.byref(used), None) == 0 and used.value == 0


def _pack_status(rec, x=0x1000, x_bytes=1 << 20, out=0x2000, out_bytes=1 << 20, n_batch=None, rows_nbits=None, rows_off=0,
                 null=()):
    """smm_grib_aec_pack with pointers that are never followed: every refusal comes before the device is touched."""
    n_batch = rec.size if n_batch is None else n_batch
    rows = np.zeros(max(rec.size, 1), dtype=GRIB_ROW_DTYPE)
    rows["nbits"] = rec["nbits"] if rows_nbits is None else rows_nbits
    rows["byte_off"] = rows_off
    recs_out, used = np.zeros(max(rec.size, 1), dtype=GRIB_AEC_DTYPE), ctypes.c_uint64(0)
    return _lib.load().smm_grib_aec_pack(
        0, None if "x" in null else ctypes.c_void_p(x), x_bytes,
        None if "rows_in" in null else ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
        None if "recs" in null else _ap(rec), n_batch, None if "out" in null else ctypes.c_void_p(out), out_bytes,
        None if "recs_out" in null else _ap(recs_out), None if "used" in null else ctypes.byref(used), None)


PACK_REFUSALS = [dict(out_bytes=195), dict(x=0x1002), dict(out=0x2001), dict(n_batch=-1), dict(x_bytes=-1), dict(out_bytes=-1),
                 dict(rows_nbits=16), dict(x_bytes=149), dict(rows_off=(1 << 20) - 149), dict(null=("x",)), dict(null=("out",)),
                 dict(null=("recs",)), dict(null=("rows_in",)), dict(null=("recs_out",)), dict(null=("used",))]


@pytest.mark.parametrize("kw", PACK_REFUSALS, ids=lambda kw: ",".join(kw))
def test_pack_refuses_before_any_device(kw):
    """The record of `_rec`: 100 values of 12 bits = 150 bytes of input, a bound of 4 blocks of 4 + 384 bits = 194 bytes -> 196."""
    assert _pack_status(_rec(), **kw) == _lib.SMM_ERR_INVALID
    assert _lib.load().smm_last_error()


def test_what_pack_takes_without_a_device():
    assert _pack_status(_rec(), n_batch=0, null=("x", "out", "recs", "rows_in", "recs_out")) == _lib.SMM_OK


# ------------------------------------------------------------------------------------------------ GribEncode(ccsds=)
def _values(rng, n_fields, n):
    v = 250.0 + 20.0 * np.cumsum(rng.standard_normal((n_fields, n)), axis=1) / 10.0
    v[1, rng.permutation(n)[:n // 7]] = np.nan       # a bitmapped field
    v[2] = 3.25                                      # a constant one: width 0, no stream
    v[3] = np.nan                                    # an empty one
    return v


@pytest.mark.parametrize("ccsds", [True, (8, 4, False), [(16, 3, True), (64, 4096, True), (8, 1, False), (32, 128, True), (16, 16, False)]],
                         ids=["default", "one_set", "per_field"])
def test_grib_encode_with_ccsds_decodes_to_the_simple_packed_bits(ccsds):
    rng = np.random.default_rng(9)
    v = _values(rng, 5, 700)
    nbits = np.array([16, 12, 9, 24, 32], dtype=np.int32)
    simple = GribEncode(nbits, 1).encode(v)
    coded = GribEncode(nbits, 1, ccsds=ccsds).encode(v)
    assert isinstance(coded, GribField) and coded.ccsds is not None and coded.bitmaps is not None and simple.ccsds is None
    a, b = simple.decode(), coded.decode()
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(np.asarray(coded).view(np.uint32), a.view(np.uint32))
    assert np.array_equal(coded.rows["nbits"], simple.rows["nbits"]) and coded.rows["nbits"].tolist()[2:4] == [0, 0]
    assert np.array_equal(coded.bitmaps["n_values"], simple.bitmaps["n_values"])
    assert int(coded.bitmaps["bitmap_off"][1]) != GRIB_NO_BITMAP and int(coded.bitmaps["bitmap_off"][0]) == GRIB_NO_BITMAP
    # a field without a stream carries the mark; the others lie back to back, 4-byte aligned, behind the bitmap slots
    assert coded.ccsds["block_size"].tolist()[2:4] == [0, 0] and (coded.ccsds["byte_len"][2:4] == 0).all()
    at = 5 * (((700 + 7) // 8 + 3) // 4 * 4)
    for r in coded.ccsds:
        assert int(r["byte_off"]) == at
        at += (int(r["byte_len"]) + 3) // 4 * 4
    assert at == coded.buf.size
    want = GribEncode.CCSDS_DEFAULT if ccsds is True else ccsds if isinstance(ccsds, tuple) else None
    if want is not None:
        live = coded.ccsds[coded.ccsds["block_size"] != 0]
        assert set(live["block_size"].tolist()) == {want[0]} and set(live["rsi"].tolist()) == {want[1]}
        assert set(live["flags"].tolist()) == {0x06 | (8 if want[2] else 0)}
    if ccsds is True:
        assert set(coded.ccsds["flags"][[0, 1, 4]].tolist()) == {0x0e}
    # smooth fields: the coded streams are shorter than the simple-packed ones
    if ccsds is True:
        assert int(coded.ccsds["byte_len"][0]) < 700 * 16 // 8


def test_grib_encode_from_field_takes_each_source_fields_parameters():
    rng = np.random.default_rng(10)
    v = _values(rng, 5, 300)
    src = GribEncode(np.array([16, 12, 9, 24, 32], dtype=np.int32), 0, ccsds=[(16, 3, True), (64, 7, True), (8, 1, False),
                                                                              (32, 128, True), (16, 16, False)]).encode(v)
    enc = GribEncode.from_field(src, ccsds=True)
    rec = enc.ccsds_records(5)
    # the fields without a stream (block_size 0 in the source) get the defaults
    assert rec["block_size"].tolist() == [16, 64, 32, 32, 16] and rec["rsi"].tolist() == [3, 7, 128, 128, 16]
    assert rec["flags"].tolist() == [0x0e, 0x0e, 0x0e, 0x0e, 0x06]
    plain = GribEncode.from_field(GribEncode(12, 0).encode(v), ccsds=True).ccsds_records(5)
    assert set(plain["block_size"].tolist()) == {32} and set(plain["rsi"].tolist()) == {128} and set(plain["flags"].tolist()) == {0x0e}
    assert GribEncode.from_field(src).ccsds is None
    with pytest.raises(ValueError):
        GribEncode(12, 0, ccsds=(12, 128, True))
    with pytest.raises(ValueError):
        GribEncode(12, 0, ccsds=(8, 5000, True))
    with pytest.raises(ValueError):
        GribEncode(np.array([12, 12], dtype=np.int32), 0, ccsds=[(8, 1, True)] * 3)


def test_regridder_refuses_grib_out_ccsds_without_grib_out():
    with pytest.raises(ValueError, match="grib_out_ccsds=True needs grib_out=True"):
        Regridder(weights=object(), packed=True, grib_out_ccsds=True)


def grib_reason(dims, levels=False, out_dtype=np.float64, codec=None, mask_dim="isobaricInhPa", **switches):
    """why `road.decide` sends a `GribField` with these dims to the host decoder, or None: it stays raw"""
    from smmregrid_amd import road
    horizontal = [d for d in dims if d in ("lat", "lon", "latitude", "longitude")]
    way = road.decide(road.Switches.of(out_dtype=out_dtype, **switches),
                      road.Facts("t", road.GRIB, np.float32, dims, horizontal, mask_dim if levels else None, codec=codec))
    assert (way.source == road.RAW_GRIB) == (way.why is None) and way.source in (road.RAW_GRIB, road.DECODED)
    return way.why


def test_regridder_keeps_a_ccsds_field_raw_only_with_grib_out_ccsds():
    on = dict(packed=True, packed_levels=True, grib_out=True)
    dims = ("isobaricInhPa", "latitude", "longitude")
    assert "grib_out" in grib_reason(dims, codec="ccsds", **on)
    on["grib_out_ccsds"] = True
    assert grib_reason(dims, codec="ccsds", **on) is None
    assert "masked levels" in grib_reason(dims, levels=True, codec="ccsds", **on)


# ------------------------------------------------------------------------------------------------ the stand-alone program
def test_encode_row_then_decode_row_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "grib_aec_encode_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_aec_encode_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "cases, options" in out.stdout
