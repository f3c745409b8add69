"""The complex-packing encoder on the host (smm_grib_cpx_encode_host, smm_grib_cpx_pack_bound; no GPU):
`griblite.cpx_encode` byte for byte and parameter for parameter against `complex_cases.encode` -- an encoder written from
the template text, with equal-length groups and the minimal n_oct -- on every X of tests/complex_cases.py at every order
and group length; round trips through the host decoder and `numpy_decode`; the sizes against the bound; the edges of THE
RULE OF THIS ENCODER read from the returned record; the refusals of the three entries; `GribEncode(..., cpx=)`; and
encode_row then decode_row in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/grib_cpx_encode_harness.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

from smmregrid_amd import GRIB_CPX_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribEncode, GribField, Regridder, _lib, cpx_encode
from smmregrid_amd.griblite import GRIB_CPX_SIMPLE, cpx_decode, cpx_want
from tests import complex_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORDERS, LENGTHS = (0, 1, 2), (8, 16, 32, 64)


def named_rows():
    """(name, X) of every case of complex_cases, the hand-assembled row, and rows of 1, 2, 3 values, of n <= L, of n not a
    multiple of L."""
    rows = [(c.name, c.X) for c in cc.cases()] + [("hand", cc.HAND_X)]
    rng = np.random.default_rng(3)
    rows += [("n1", np.array([9])), ("n2", np.array([9, 4])), ("n3", np.array([9, 4, 11])),
             ("n8", rng.integers(0, 500, 8)), ("n63", rng.integers(0, 70000, 63)), ("n65", rng.integers(0, 70000, 65)),
             ("n1001", np.cumsum(rng.integers(0, 9, 1001)))]
    return rows


ROWS = named_rows()


def equal_lengths(n, L):
    ng = -(-n // L)
    return [L] * (ng - 1) + [n - (ng - 1) * L]


def effective_order(X, order):
    """Rule 1, from the integers, with none of the product's code: (effective order, minimal n_oct)."""
    X = np.asarray(X, dtype=np.int64)
    if X.size <= order or order == 0:
        return 0, 0
    d, g, heads = cc.differences(X, order)
    top = max(abs(int(v)) for v in heads + [g])
    if top > 2 ** 31 - 1 or int(d[order:].max()) - g >= 2 ** 32:
        return 0, 0
    return order, next(k for k in (1, 2, 3, 4) if top < 1 << (8 * k - 1))


def oracle(X, order, L):
    eff, n_oct = effective_order(X, order)
    return cc.encode(X, eff, equal_lengths(len(X), L), n_oct=n_oct or 2)


def bound_of(n, nbits, order, L):
    total = ctypes.c_uint64(0)
    rec = cpx_want(nbits, order, L, n).reshape(1)
    _lib.call("smm_grib_cpx_pack_bound", _cp(rec), 1, None, ctypes.byref(total))
    return int(total.value)


def _cp(rec):
    return ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct))


@pytest.mark.parametrize("name,X", ROWS, ids=[r[0] for r in ROWS])
def test_host_encoder_equals_the_template_encoder_and_round_trips(name, X):
    """Orders 0 / 1 / 2 and L = 8 / 16 / 32 / 64: the stream and every parameter are `complex_cases.encode`'s; the stream
    decodes back through smm_grib_cpx_decode_host and `numpy_decode`; it is no longer than the bound."""
    w = cc.width_of(X)
    for order in ORDERS:
        for L in LENGTHS:
            stream, rec = cpx_encode(X, cpx_want(w, order, L))
            if w == 0:
                assert int(rec["order"]) == GRIB_CPX_SIMPLE and stream.size == 0 and int(rec["byte_len"]) == 0
                assert int(rec["n_values"]) == X.size and bound_of(X.size, 0, order, L) == 0
                continue
            want, p = oracle(X, order, L)
            got_p = {k: int(rec[k]) for k in cc.PARAM_NAMES}
            assert got_p == p, (name, order, L, got_p, p)
            assert np.array_equal(stream, want), (name, order, L, stream.size, want.size)
            assert (int(rec["byte_off"]), int(rec["byte_len"]), int(rec["n_values"]), int(rec["reserved"])) == (0, want.size, X.size, 0)
            assert stream.size <= bound_of(X.size, w, order, L) and bound_of(X.size, w, order, L) % 4 == 0
            assert np.array_equal(cpx_decode(stream, rec).astype(np.int64), X)
            if X.size <= 5000:
                assert np.array_equal(cc.numpy_decode(stream, X.size, got_p), X)


def test_a_row_of_no_values_has_no_groups_and_no_bytes():
    for order in ORDERS:
        stream, rec = cpx_encode(np.zeros(0, np.uint32), cpx_want(12, order, 32))
        assert stream.size == 0 and [int(rec[k]) for k in ("n_groups", "byte_len", "n_values", "order", "n_oct")] == [0] * 5
        assert bound_of(0, 12, order, 32) == 0


def _rec_of(X, nbits, order, L):
    return cpx_encode(np.asarray(X, dtype=np.uint64).astype(np.uint32), cpx_want(nbits, order, L))


def test_edges_of_the_rule():
    rng = np.random.default_rng(4)
    # a group of equal z: its width is 0, and it is the width reference
    X = np.concatenate([np.full(8, 77), rng.integers(0, 256, 24)])
    st, r = _rec_of(X, 8, 0, 8)
    assert int(r["width_ref"]) == 0 and int(r["width_bits"]) >= 1 and int(r["n_groups"]) == 4
    assert np.array_equal(cpx_decode(st, r), X)
    # all groups of one width: no bits per stored width, an empty widths table
    X = np.tile(np.array([0, 255, 3, 9, 100, 1, 2, 200]), 6) + np.repeat(np.arange(6) * 256, 8)
    st, r = _rec_of(X, 11, 0, 8)
    assert (int(r["width_ref"]), int(r["width_bits"])) == (8, 0)
    assert int(r["byte_len"]) == (6 * int(r["nbits"]) + 7) // 8 + 48
    # every reference 0: no bits per reference
    X = rng.integers(1, 1000, 64)
    X[::8] = 0
    st, r = _rec_of(X, 10, 0, 8)
    assert int(r["nbits"]) == 0 and np.array_equal(cpx_decode(st, r), X)
    # a 32-bit row whose first integer does not fit a descriptor: order 0
    X = np.array([2 ** 31, 2 ** 31 + 5, 2 ** 31 + 9, 2 ** 31 + 11] * 4)
    for order in (1, 2):
        st, r = _rec_of(X, 32, order, 8)
        assert (int(r["order"]), int(r["n_oct"])) == (0, 0) and np.array_equal(cpx_decode(st, r), X)
    st, r = _rec_of(X - 1, 32, 1, 8)            # 2^31 - 1 fits: four octets
    assert (int(r["order"]), int(r["n_oct"])) == (1, 4) and np.array_equal(cpx_decode(st, r), X - 1)
    # 0 / 2^32 - 1 alternating: the differences span more than 32 bits: order 0
    X = np.array([0, 2 ** 32 - 1] * 20)
    for order in (1, 2):
        st, r = _rec_of(X, 32, order, 16)
        assert int(r["order"]) == 0 and np.array_equal(cpx_decode(st, r), X)
    # 29 bits at their extremes keep order 2: |g| = 2^30 - 2, z up to 2^31 - 4
    X = np.array([0, 2 ** 29 - 1] * 20)
    st, r = _rec_of(X, 29, 2, 16)
    assert (int(r["order"]), int(r["n_oct"])) == (2, 4) and int(r["width_ref"]) == 31      # z = 0 or 2^31 - 4 in every group
    assert np.array_equal(cpx_decode(st, r), X) and st.size <= bound_of(40, 29, 2, 16)
    # there is no cascade from 2 to 1: a row that would fit order 1 but not order 2 goes to 0
    X = np.array([0, 2 ** 31 - 1, 0, 2 ** 31 - 1] * 4)
    assert int(_rec_of(X, 31, 1, 8)[1]["order"]) == 1 and int(_rec_of(X, 31, 2, 8)[1]["order"]) == 0
    # integers of width 0 are not coded
    st, r = _rec_of(np.zeros(50), 0, 2, 32)
    assert st.size == 0 and int(r["order"]) == GRIB_CPX_SIMPLE and int(r["byte_len"]) == 0


# ------------------------------------------------------------------------------------------------ refusals
def _want(**kw):
    rec = cpx_want(12, 2, 32, 100).reshape(1)
    for k, v in kw.items():
        rec[k] = v
    return rec


BAD_RECORDS = [dict(order=3), dict(order=-1), dict(length_ref=0), dict(length_ref=12), dict(length_ref=128), dict(nbits=33),
               dict(nbits=-1), dict(n_values=2 ** 31), dict(reserved=1)]


@pytest.mark.parametrize("kw", BAD_RECORDS, ids=lambda kw: ",".join(f"{k}={v}" for k, v in kw.items()))
def test_every_entry_refuses_a_bad_wanted_record(kw):
    lib, total, used = _lib.load(), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rec, out_rec = _want(**kw), np.zeros(1, dtype=GRIB_CPX_DTYPE)
    assert lib.smm_grib_cpx_pack_bound(_cp(rec), 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    assert lib.smm_last_error()
    assert _pack_status(rec) == _lib.SMM_ERR_INVALID
    values, out = np.zeros(100, np.uint32), np.zeros(4096, np.uint8)
    assert lib.smm_grib_cpx_encode_host(values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), int(rec["n_values"][0]), _cp(rec),
                                        ctypes.c_void_p(out.ctypes.data), out.size, ctypes.byref(used), _cp(out_rec)) == _lib.SMM_ERR_INVALID


def test_bound_and_encode_host_refusals():
    lib, total, used = _lib.load(), ctypes.c_uint64(0), ctypes.c_uint64(0)
    rec, out_rec = _want(), np.zeros(1, dtype=GRIB_CPX_DTYPE)
    assert lib.smm_grib_cpx_pack_bound(_cp(rec), 1, None, None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_cpx_pack_bound(None, 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_cpx_pack_bound(_cp(rec), -1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    # 100 values of 12 bits at order 2 in groups of 32: 12 + ceil(4 * 14 / 8) + ceil(4 * 6 / 8) + ceil(100 * 14 / 8) = 197 -> 200
    offs = np.zeros(2, dtype=np.uint64)
    two = np.concatenate([rec, rec])
    assert lib.smm_grib_cpx_pack_bound(_cp(two), 2, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(total)) == 0
    assert offs.tolist() == [0, 200] and total.value == 400
    values, out = np.arange(100, dtype=np.uint32), np.zeros(200, np.uint8)
    vp, op = values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.c_void_p(out.ctypes.data)

    def call(v=vp, n=100, r=rec, o=op, cap=200, u=ctypes.byref(used), ro=out_rec):
        return lib.smm_grib_cpx_encode_host(v, n, None if r is None else _cp(r), o, cap, u, None if ro is None else _cp(ro))
    assert call() == _lib.SMM_OK and used.value > 0
    for bad in (dict(v=None), dict(n=99), dict(n=-1), dict(r=None), dict(o=None), dict(cap=199), dict(cap=-1), dict(u=None),
                dict(ro=None)):
        assert call(**bad) == _lib.SMM_ERR_INVALID, bad
        assert lib.smm_last_error()
    values[7] = 4096                                                    # does not fit into 12 bits
    assert call() == _lib.SMM_ERR_INVALID and b"values[7]" in lib.smm_last_error()
    # rows of width 0 and of no values need neither values nor room
    assert call(v=None, r=_want(nbits=0), o=None, cap=0) == _lib.SMM_ERR_INVALID      # 100 values, no pointer
    assert call(v=None, n=0, r=_want(n_values=0), o=None, cap=0) == _lib.SMM_OK and used.value == 0


def _pack_status(rec, x=0x1000, x_bytes=1 << 20, out=0x2000, out_bytes=1 << 20, n_batch=None, rows_nbits=None, rows_off=0,
                 null=()):
    """smm_grib_cpx_pack with pointers that are never followed: every refusal comes before the device is touched."""
    n_batch = rec.size if n_batch is None else n_batch
    rows = np.zeros(max(rec.size, 1), dtype=GRIB_ROW_DTYPE)
    rows["nbits"] = rec["nbits"] if rows_nbits is None else rows_nbits
    rows["byte_off"] = rows_off
    recs_out, used = np.zeros(max(rec.size, 1), dtype=GRIB_CPX_DTYPE), ctypes.c_uint64(0)
    return _lib.load().smm_grib_cpx_pack(
        0, None if "x" in null else ctypes.c_void_p(x), x_bytes,
        None if "rows_in" in null else ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
        None if "recs" in null else _cp(rec), n_batch, None if "out" in null else ctypes.c_void_p(out), out_bytes,
        None if "recs_out" in null else _cp(recs_out), None if "used" in null else ctypes.byref(used), None)


PACK_REFUSALS = [dict(out_bytes=199), dict(x=0x1002), dict(out=0x2001), dict(n_batch=-1), dict(x_bytes=-1), dict(out_bytes=-1),
                 dict(rows_nbits=16), dict(x_bytes=149), dict(rows_off=(1 << 20) - 149), dict(null=("x",)), dict(null=("out",)),
                 dict(null=("recs",)), dict(null=("rows_in",)), dict(null=("recs_out",)), dict(null=("used",))]


@pytest.mark.parametrize("kw", PACK_REFUSALS, ids=lambda kw: ",".join(kw))
def test_pack_refuses_before_any_device(kw):
    """The record of `_want`: 100 values of 12 bits = 150 bytes of input, a bound of 200 bytes."""
    assert _pack_status(_want(), **kw) == _lib.SMM_ERR_INVALID
    assert _lib.load().smm_last_error()


def test_what_pack_takes_without_a_device():
    assert _pack_status(_want(), n_batch=0, null=("x", "out", "recs", "rows_in", "recs_out")) == _lib.SMM_OK


# ------------------------------------------------------------------------------------------------ GribEncode(cpx=)
def _values(rng, n_fields, n):
    v = 250.0 + 20.0 * np.cumsum(rng.standard_normal((n_fields, n)), axis=1) / 10.0
    v[1, rng.permutation(n)[:n // 7]] = np.nan       # a bitmapped field
    v[2] = 3.25                                      # a constant one: width 0, no stream
    v[3] = np.nan                                    # an empty one
    return v


@pytest.mark.parametrize("cpx", [True, (1, 8), [(0, 16), (2, 64), (1, 8), (2, 32), (1, 16)]], ids=["default", "one_set", "per_field"])
def test_grib_encode_with_cpx_decodes_to_the_simple_packed_bits(cpx):
    rng = np.random.default_rng(9)
    v = _values(rng, 5, 700)
    nbits = np.array([16, 12, 9, 24, 32], dtype=np.int32)
    simple = GribEncode(nbits, 1).encode(v)
    coded = GribEncode(nbits, 1, cpx=cpx).encode(v)
    assert isinstance(coded, GribField) and coded.cpx is not None and coded.bitmaps is not None and coded.ccsds is None
    a, b = simple.decode(), coded.decode()
    assert a.dtype == b.dtype == np.float32 and np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert np.array_equal(np.asarray(coded).view(np.uint32), a.view(np.uint32))
    # the rows keep the widths of the integers
    assert np.array_equal(coded.rows["nbits"], simple.rows["nbits"]) and coded.rows["nbits"].tolist()[2:4] == [0, 0]
    assert np.array_equal(coded.bitmaps["n_values"], simple.bitmaps["n_values"])
    assert int(coded.bitmaps["bitmap_off"][1]) != GRIB_NO_BITMAP and int(coded.bitmaps["bitmap_off"][0]) == GRIB_NO_BITMAP
    # a field without a stream carries the mark; the others lie back to back, 4-byte aligned, behind the bitmap slots
    assert coded.cpx["order"].tolist()[2:4] == [GRIB_CPX_SIMPLE] * 2 and (coded.cpx["byte_len"][2:4] == 0).all()
    at = 5 * (((700 + 7) // 8 + 3) // 4 * 4)
    for r, row in zip(coded.cpx, coded.rows):
        assert int(r["byte_off"]) == at == int(row["byte_off"])
        at += (int(r["byte_len"]) + 3) // 4 * 4
    assert at == coded.buf.size
    want = GribEncode.CPX_DEFAULT if cpx is True else cpx if isinstance(cpx, tuple) else None
    live = coded.cpx[coded.cpx["order"] != GRIB_CPX_SIMPLE]
    if want is not None:
        assert set(live["order"].tolist()) == {want[0]} and set(live["length_ref"].tolist()) == {want[1]}
    if cpx is True:      # a smooth field: shorter than simple-packed
        assert GribEncode.CPX_DEFAULT == (2, 32) and int(coded.cpx["byte_len"][0]) < 700 * 16 // 8
    # bounds, per field and summed, hold the streams
    enc = GribEncode(nbits, 1, cpx=cpx)
    assert (coded.cpx["byte_len"] <= enc.cpx_bounds(700, 5)).all() and enc.cpx_bound(700, 5) == int(enc.cpx_bounds(700, 5).sum())
    part = enc.rows_of(1, 4, 5)
    assert part.nbits.tolist() == [12, 9, 24] and np.array_equal(part.cpx_records(3)["order"], enc.cpx_records(5)["order"][1:4])


def test_grib_encode_cpx_argument_checks():
    for bad in ((3, 32), (-1, 32), (1, 12), (2, 128)):
        with pytest.raises(ValueError, match="complex packing of order"):
            GribEncode(12, 0, cpx=bad)
    with pytest.raises(ValueError, match="cpx does not go with ccsds"):
        GribEncode(12, 0, cpx=True, ccsds=True)
    with pytest.raises(ValueError):
        GribEncode(np.array([12, 12], dtype=np.int32), 0, cpx=[(1, 8)] * 3)
    assert GribEncode(12, 0, cpx=[(1, 8)] * 3).n_fields == 3
    assert GribEncode(12, 0).cpx is None


def test_from_field_marks_complex_packed_source_rows_with_source_width():
    rng = np.random.default_rng(10)
    v = _values(rng, 5, 300)
    src = GribEncode(np.array([16, 12, 9, 24, 32], dtype=np.int32), 0, cpx=[(1, 8), (2, 64), (1, 16), (0, 32), (0, 8)]).encode(v)
    enc = GribEncode.from_field(src, cpx=True)
    # fields 2 and 3 have no stream in the source (marked simple-packed, width 0): the defaults and the largest live width
    assert enc.cpx_records(5, marks=True)["order"].tolist() == [1, 2, 2, 2, 0]
    assert set(enc.cpx_records(5, marks=True)["length_ref"].tolist()) == {32}
    assert enc.nbits.tolist() == [GribEncode.SOURCE_WIDTH] * 2 + [16, 16] + [GribEncode.SOURCE_WIDTH] and enc.has_source_width
    for refused in (lambda: enc.encode(v), lambda: enc.records(5), lambda: enc.layout(300, 5), lambda: enc.cpx_bounds(300, 5)):
        with pytest.raises(ValueError, match="SOURCE_WIDTH"):
            refused()
    done = enc.resolved([13, 0, 5, 5, 31])
    assert done.nbits.tolist() == [13, 31, 16, 16, 31] and not done.has_source_width
    assert np.array_equal(done.cpx_records(5)["order"], [1, 2, 2, 2, 0]) and np.array_equal(done.decimal_scale, enc.decimal_scale)
    assert enc.rows_of(0, 2, 5).nbits.tolist() == [GribEncode.SOURCE_WIDTH] * 2
    # a simple-packed source: its own widths, the defaults
    plain = GribEncode.from_field(GribEncode(12, 0).encode(v), cpx=True)
    assert not plain.has_source_width and set(plain.cpx_records(5)["order"].tolist()) == {2}
    assert GribEncode.from_field(src).cpx is None
    with pytest.raises(ValueError, match="1..32"):
        GribEncode(-2, 0)


def test_regridder_keyword_checks():
    with pytest.raises(ValueError, match="grib_out_cpx=True needs grib_out=True"):
        Regridder(weights=object(), packed=True, grib_out_cpx=True)
    with pytest.raises(ValueError, match="does not go with grib_out_ccsds"):
        Regridder(weights=object(), packed=True, grib_out=True, grib_out_cpx=True, grib_out_ccsds=True)


def grib_reason(dims, levels=False, out_dtype=np.float64, codec=None, mask_dim="isobaricInhPa", **switches):
    """why `road.decide` sends a `GribField` with these dims to the host decoder, or None: it stays raw"""
    from smmregrid_amd import road
    horizontal = [d for d in dims if d in ("lat", "lon", "latitude", "longitude")]
    way = road.decide(road.Switches.of(out_dtype=out_dtype, **switches),
                      road.Facts("t", road.GRIB, np.float32, dims, horizontal, mask_dim if levels else None, codec=codec))
    assert (way.source == road.RAW_GRIB) == (way.why is None) and way.source in (road.RAW_GRIB, road.DECODED)
    return way.why


def test_regridder_keeps_a_complex_packed_field_raw_only_with_grib_out_cpx():
    on = dict(packed=True, packed_levels=True, grib_out=True)
    dims = ("isobaricInhPa", "latitude", "longitude")
    assert grib_reason(dims, codec="cpx", **on) == "complex packing with grib_out"
    on["grib_out_cpx"] = True
    assert grib_reason(dims, codec="cpx", **on) is None
    assert grib_reason(dims, codec="ccsds", **on) == "CCSDS packing with grib_out"
    assert "masked levels" in grib_reason(dims, levels=True, codec="cpx", **on)


# ------------------------------------------------------------------------------------------------ the stand-alone program
def test_encode_row_then_decode_row_under_the_sanitizers(tmp_path):
    exe = str(tmp_path / "grib_cpx_encode_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_cpx_encode_harness.cpp")])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    assert "cases, fallbacks" in out.stdout
