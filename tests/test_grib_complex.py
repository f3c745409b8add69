"""Complex-packed GRIB-2 fields (data representation templates 5.2 / 5.3) without a GPU: the host decoder
(smm_grib_cpx_decode_host, the text of smmregrid_amd/csrc/smm_grib_cpx.hpp) against the numpy decoder of
tests/complex_cases.py on every case and on the hand-assembled message; `griblite` on synthesized messages; the refusals
of the reader and of the entries, which come before any device is touched; and the decoder on truncated, corrupted and
random input in a stand-alone program under AddressSanitizer + UBSan (tests/cpp/grib_cpx_harness.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import GRIB_CPX_DTYPE, GRIB_ROW_DTYPE, GribField, _lib, griblite
from smmregrid_amd.io import open_dataset
from tests import complex_cases as xc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = xc.cases()
NI, NJ = xc.NI, xc.NJ


# ------------------------------------------------------------------------------------------------ the decoders
def test_the_case_list_covers_what_it_should():
    p = {c.name: c.params for c in CASES}
    assert {c.order for c in CASES} == {0, 1, 2} and {c.params["n_oct"] for c in CASES if c.order} == {1, 2, 3, 4}
    assert p["order0_widths_0_1_31_32"]["width_bits"] == 6 and xc.case("order0_widths_0_1_31_32").width == 32
    assert p["order0_width_bits0"]["width_bits"] == 0 and p["order0_width_bits0"]["width_ref"] == 10
    assert p["order1_length_bits0_last48"]["length_bits"] == 0 and p["order1_length_bits0_last48"]["length_last"] == 48
    assert p["order2_inc7_last1"]["length_inc"] == 7 and p["order2_inc7_last1"]["length_last"] == 1
    assert p["order1_one_group"]["n_groups"] == 1 and p["order0_groups_of_one"]["n_groups"] == xc.S
    five = p["order0_five_groups_3bits"]
    assert (five["n_groups"] * five["nbits"]) % 8 and (five["n_groups"] * five["width_bits"]) % 8 and \
        (five["n_groups"] * five["length_bits"]) % 8
    assert p["order1_nbits0"]["nbits"] == 0 and xc.case("order0_all_zero").width == 0 and xc.case("order0_all_zero").stream.size == 0
    assert xc.case("order1_constant_777").width == 10 and xc.case("n3_order2").n_values == 3 and xc.case("n2_order1").n_values == 2
    big = xc.case("big300000_order2")
    assert big.n_values == 300000 and big.params["n_groups"] == 40000 and len(set(big.lengths)) > 10
    g = {c.name: xc.differences(c.X, c.order)[1] for c in CASES}
    assert g["order1_descending"] < 0
    d = xc.differences(xc.case("order2_curvature").X, 2)[0][2:]
    assert d.min() < 0 < d.max()                                    # z + g changes sign


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_numpy_decoder_host_entry_and_cpx_decode_agree(c):
    want = xc.numpy_decode(c.stream, c.n_values, c.params)
    assert np.array_equal(want, c.X)
    got = griblite.cpx_decode(c.stream, c.record(0))
    assert got.dtype == np.uint32 and np.array_equal(got, c.X)
    # the stream anywhere in a larger buffer, at an odd offset, garbage around it; the entry itself
    buf = np.full(c.stream.size + 11, 0xA5, dtype=np.uint8)
    buf[5:5 + c.stream.size] = c.stream
    rec = c.record(5).reshape(1)
    values, status = np.zeros(c.n_values, np.uint32), ctypes.c_int(-1)
    assert _lib.load().smm_grib_cpx_decode_host(buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                                ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct)),
                                                values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), ctypes.byref(status)) == 0
    assert status.value == _lib.GRIB_CPX_OK and np.array_equal(values, c.X)


def test_the_hand_assembled_message():
    """Encoder and decoders are not only checked against each other: the bytes were worked out by hand (the docstring of
    tests/complex_cases.py) and lie in tests/golden/complex/hand_order2.grib2."""
    with open(os.path.join(xc.GOLDEN, "hand_order2.grib2"), "rb") as fh:
        msg = fh.read()
    assert msg == xc.hand_message() and len(msg) < 512
    at = msg.index(xc.HAND_STREAM)
    assert msg[at - 5:at] == (5 + 16).to_bytes(4, "big") + bytes([7])          # section 7, 21 octets
    s5 = msg[msg.index(bytes([0, 0, 0, 49, 5])):][:49]
    assert s5[5:11] == (12).to_bytes(4, "big") + (3).to_bytes(2, "big")
    assert s5[19:49].hex() == "03000100" + "00" * 8 + "00000003" + "0301" + "00000004" + "01" + "00000003" + "01" + "0202"
    stream, params = xc.encode(xc.HAND_X, 2, xc.HAND_LENGTHS, n_oct=2)
    assert stream.tobytes() == xc.HAND_STREAM and params == xc.HAND_PARAMS
    hand = np.frombuffer(xc.HAND_STREAM, np.uint8)
    assert np.array_equal(xc.numpy_decode(hand, 12, xc.HAND_PARAMS), xc.HAND_X)
    assert np.array_equal(griblite.cpx_decode(hand, xc.record(0, 16, 12, xc.HAND_PARAMS)), xc.HAND_X)


def test_the_hand_assembled_message_opens(tmp_path):
    path = os.path.join(xc.GOLDEN, "hand_order2.grib2")
    want = xc.HAND_X.astype(np.float32).reshape(3, 4)
    assert np.array_equal(open_dataset(path)["t"].values, want)
    raw = open_dataset(path, decode=False)["t"].data
    assert isinstance(raw, GribField) and raw.cpx is not None and tuple(raw.cpx[0])[3:13] == tuple(xc.HAND_PARAMS[k] for k in xc.PARAM_NAMES)
    assert int(raw.cpx["byte_len"][0]) == 16 and np.array_equal(np.asarray(raw), want)


# ------------------------------------------------------------------------------------------------ griblite
@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("complex_grib")
    paths = {}
    for kind in ("complex", "simple"):
        paths[kind] = str(d / f"{kind}.grib2")
        with open(paths[kind], "wb") as fh:
            fh.write(xc.grib2_message(xc.message_fields(kind == "complex")))
    return paths


def rule_of_specs():
    """The float32 fields of MESSAGE_SPECS by the rule applied to X, in (time, level ascending) order."""
    out = np.full((2, 3, NJ * NI), np.nan, dtype=np.float32)
    present = xc.present_1500()
    for name, level, step, bitmap, R, E, D in xc.MESSAGE_SPECS:
        v = ((float(np.float32(R)) + xc.case(name).X.astype(np.float64) * 2.0 ** E) / 10.0 ** D).astype(np.float32)
        slot = (step // 6, {25000: 0, 50000: 1, 85000: 2}[level])
        if bitmap is None:
            out[slot] = v
        else:
            out[slot][present] = v
    return out.reshape(2, 3, NJ, NI)


def test_decoded_opening_is_the_rule_applied_to_the_integers(twins):
    got, twin = open_dataset(twins["complex"]), open_dataset(twins["simple"])
    assert got["t"].shape == (2, 3, NJ, NI) and got["t"].values.dtype == np.float32
    assert got["t"].values.tobytes() == rule_of_specs().tobytes()
    assert got["t"].values.tobytes() == twin["t"].values.tobytes()
    assert np.isnan(got["t"].values[1, 2]).sum() == NI * NJ - 1500       # the bitmapped fields are there


@pytest.mark.parametrize("bitmaps", [False, True])
def test_raw_opening_keeps_the_records(twins, bitmaps):
    decoded = rule_of_specs()
    ds = open_dataset(twins["complex"], decode=False, bitmaps=bitmaps)
    data = ds["t"].data
    if not bitmaps:      # a variable with bitmapped messages is decoded unless bitmaps=True
        assert isinstance(data, np.ndarray) and data.tobytes() == decoded.tobytes()
        return
    assert isinstance(data, GribField) and data.cpx is not None and data.cpx.dtype == GRIB_CPX_DTYPE and data.ccsds is None
    assert data.cpx.size == data.rows.size == 6 and "5 complex-packed" in repr(data)
    names = [name for name, *_ in sorted(xc.MESSAGE_SPECS, key=lambda sp: (sp[2], sp[1]))]     # (time, level ascending)
    for k, (rec, row, name) in enumerate(zip(data.cpx, data.rows, names)):
        c = xc.case(name)
        if name == xc.MESSAGE_SPECS[-1][0]:           # the simple-packed message among them
            assert int(rec["order"]) == _lib.GRIB_CPX_SIMPLE and int(row["nbits"]) == c.width
            continue
        assert tuple(int(rec[f]) for f in xc.PARAM_NAMES) == tuple(c.params[f] for f in xc.PARAM_NAMES)
        assert int(rec["n_values"]) == c.n_values and int(rec["byte_len"]) == c.stream.size
        off = int(rec["byte_off"])
        assert off == int(row["byte_off"]) and np.array_equal(data.buf[off:off + c.stream.size], c.stream)
    assert int((data.bitmaps["bitmap_off"] != smmregrid_amd.GRIB_NO_BITMAP).sum()) == 2
    assert data.bitmaps["bitmap_off"][2] == data.bitmaps["bitmap_off"][5]          # the reused bitmap
    assert data.decode().tobytes() == decoded.tobytes()
    assert np.asarray(data).tobytes() == decoded.tobytes()


def test_a_variable_that_mixes_ccsds_and_complex_packing_is_decoded_at_open(tmp_path):
    from tests import ccsds_cases as cc
    fx, c = cc.fixture("grid_w12_smooth"), xc.case("order2_noct3")
    one = cc.grib2_message([dict(q=fx.values, nbits=fx.nbits, R=1.0, level=50000, ccsds=(fx.stream, fx.flags, fx.block, fx.rsi))],
                           NI, NJ)
    two = xc.grib2_message([dict(cpx=(c.stream, c.params, c.n_values), R=1.0, level=85000)])
    p = tmp_path / "mixed.grib2"
    p.write_bytes(one + two)
    data = open_dataset(str(p), decode=False)["t"].data
    assert isinstance(data, np.ndarray) and data.shape == (2, NJ, NI)
    assert np.array_equal(data[1].ravel(), (1.0 + c.X).astype(np.float32))


def _message_with(tmp_path, name, **s5_changes):
    """A one-field file whose section 5 has octets replaced: {octet number (1-based): byte}."""
    c = xc.case(name)
    body = bytearray(xc.section5(c.n_values, c.params))
    for octet, byte in s5_changes.items():
        body[int(octet[1:]) - 6] = byte
    p = tmp_path / "refused.grib2"
    p.write_bytes(xc.grib2_message([dict(cpx=(c.stream, c.params, c.n_values), s5=bytes(body))]))
    return str(p)


REFUSED = [("order2_noct3", dict(o23=1), "missing value management 1"), ("order0_noise12", dict(o23=2), "missing value management 2"),
           ("order2_noct3", dict(o48=3), "order 3"), ("order2_noct3", dict(o49=0), "0 octets per extra descriptor"),
           ("order2_noct3", dict(o49=5), "5 octets per extra descriptor"), ("order0_noise12", dict(o37=33), "group widths stored in 33 bits"),
           ("order0_noise12", dict(o47=40), "group lengths in 40"), ("order1_noct2", dict(o20=33), "group references of 33 bits"),
           ("order1_noct2", dict(o32=0, o33=0, o34=0, o35=0), "in no group"), ("n2_order1", dict(o48=2), "order 2 on 2 values")]


@pytest.mark.parametrize("name, changes, what", REFUSED, ids=[r[2].replace(" ", "_") for r in REFUSED])
def test_refusals_are_named(tmp_path, name, changes, what):
    path = _message_with(tmp_path, name, **changes)
    for decode in (True, False):
        with pytest.raises(griblite.GribUnsupported, match=re.escape(what)) as err:
            open_dataset(path, decode=decode)
        assert "complex packing" in str(err.value)


def test_short_section5_and_other_templates_are_refused(tmp_path):
    c = xc.case("order2_noct3")
    body = xc.section5(c.n_values, c.params)[:-1]
    p = tmp_path / "short5.grib2"
    p.write_bytes(xc.grib2_message([dict(cpx=(c.stream, c.params, c.n_values), s5=body)]))
    with pytest.raises(griblite.GribUnsupported, match="the template takes 49"):
        open_dataset(str(p))
    jpeg = bytearray(xc.section5(c.n_values, c.params))
    jpeg[4:6] = (40).to_bytes(2, "big")
    p.write_bytes(xc.grib2_message([dict(cpx=(c.stream, c.params, c.n_values), s5=bytes(jpeg))]))
    with pytest.raises(griblite.GribUnsupported, match="JPEG"):
        open_dataset(str(p))


def test_a_stream_that_ends_early_is_an_error_not_numbers(tmp_path):
    c = xc.case("order2_noct3")
    p = tmp_path / "short.grib2"
    p.write_bytes(xc.grib2_message([dict(cpx=(c.stream[:c.stream.size // 2], c.params, c.n_values))]))
    with pytest.raises(ValueError, match="ends before"):
        open_dataset(str(p))


# ------------------------------------------------------------------------------------------------ the ABI and its refusals
def test_record_dtype_header_exports_and_ctypes_table_agree():
    assert GRIB_CPX_DTYPE.itemsize == ctypes.sizeof(_lib.GribCpxStruct) == 72
    for name, ctype in _lib.GribCpxStruct._fields_:
        assert GRIB_CPX_DTYPE.fields[name][1] == getattr(_lib.GribCpxStruct, name).offset
        assert GRIB_CPX_DTYPE.fields[name][0].itemsize == ctypes.sizeof(ctype)
    header = open(os.path.join(ROOT, "include", "smmregrid_amd.h")).read()
    struct = header[header.index("typedef struct smm_grib_cpx_t"):header.index("} smm_grib_cpx_t;")]
    assert re.findall(r"^\s+u?int\d+_t (\w+);", struct, re.M) == [n for n, _ in _lib.GribCpxStruct._fields_]
    assert "#define SMM_GRIB_CPX_SIMPLE (-1)" in header and _lib.GRIB_CPX_SIMPLE == griblite.GRIB_CPX_SIMPLE == -1
    assert "SMM_GRIB_CPX_OK = 0, SMM_GRIB_CPX_EXHAUSTED = 1, SMM_GRIB_CPX_INVALID = 2" in header
    lib = _lib.load()
    for entry in ("smm_grib_cpx_layout", "smm_grib_cpx_unpack", "smm_grib_cpx_decode_host"):
        assert entry in _lib.SIGNATURES and re.search(r"^int " + entry + r"\(", header, re.M) and getattr(lib, entry)
    assert lib.smm_abi_version() == 6 and "#define SMM_ABI_VERSION 6" in header
    assert {"GRIB_CPX_DTYPE", "grib_unpack_cpx"} <= set(smmregrid_amd.__all__)
    assert smmregrid_amd.grib_unpack_cpx is smmregrid_amd.device.grib_unpack_cpx


def _rec(**kw):
    r = np.zeros(1, dtype=GRIB_CPX_DTYPE)
    r["byte_len"], r["n_values"], r["n_groups"], r["nbits"], r["width_ref"], r["width_bits"] = 64, 100, 4, 8, 3, 3
    r["length_ref"], r["length_inc"], r["length_last"], r["length_bits"], r["order"], r["n_oct"] = 20, 1, 40, 4, 2, 2
    for k, v in kw.items():
        r[k] = v
    return r


def _unpack_status(rec, x=0x1000, x_bytes=64, out=0x2000, out_bytes=1 << 20, n_batch=None, null=()):
    """smm_grib_cpx_unpack with pointers that are never followed: every refusal comes before the device is touched."""
    n_batch = rec.size if n_batch is None else n_batch
    rows = np.zeros(max(rec.size, 1), dtype=GRIB_ROW_DTYPE)
    rows_out = np.zeros_like(rows)
    rp = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))               # noqa: E731
    return _lib.load().smm_grib_cpx_unpack(
        0, None if "x" in null else ctypes.c_void_p(x), x_bytes,
        None if "recs" in null else ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct)),
        None if "rows_in" in null else rp(rows), n_batch, None if "out" in null else ctypes.c_void_p(out), out_bytes,
        None if "rows_out" in null else rp(rows_out), None)


REFUSALS = [dict(rec=_rec(order=3)), dict(rec=_rec(order=-2)), dict(rec=_rec(n_oct=0)), dict(rec=_rec(n_oct=5)), dict(rec=_rec(nbits=33)),
            dict(rec=_rec(nbits=-1)), dict(rec=_rec(width_bits=33)), dict(rec=_rec(length_bits=33)), dict(rec=_rec(width_ref=256)),
            dict(rec=_rec(length_inc=256)), dict(rec=_rec(n_groups=0)), dict(rec=_rec(n_values=2)), dict(rec=_rec(n_values=1, order=1)),
            dict(rec=_rec(n_values=2 ** 31)), dict(rec=_rec(reserved=1)), dict(rec=_rec(byte_off=1)), dict(rec=_rec(byte_len=65)),
            dict(rec=_rec(byte_off=2 ** 63, byte_len=2 ** 63)), dict(rec=_rec(), out_bytes=399), dict(rec=_rec(), x=0x1002),
            dict(rec=_rec(), out=0x2001), dict(rec=_rec(), n_batch=-1), dict(rec=_rec(), x_bytes=-1), dict(rec=_rec(), out_bytes=-1),
            dict(rec=_rec(), null=("x",)), dict(rec=_rec(), null=("out",)), dict(rec=_rec(), null=("recs",)),
            dict(rec=_rec(), null=("rows_in",)), dict(rec=_rec(), null=("rows_out",))]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: ",".join(f"{k}" for k in kw if k != "rec") or "rec")
def test_unpack_refuses_before_any_device(kw):
    assert _unpack_status(**kw) == _lib.SMM_ERR_INVALID
    assert _lib.load().smm_last_error()


def test_refusals_name_the_field_and_the_row():
    lib = _lib.load()
    two = np.concatenate([_rec(), _rec(order=3)])
    assert _unpack_status(two) == _lib.SMM_ERR_INVALID
    assert b"recs[1]" in lib.smm_last_error() and b"order" in lib.smm_last_error()
    assert _unpack_status(_rec(n_oct=7)) == _lib.SMM_ERR_INVALID and b"n_oct" in lib.smm_last_error()
    assert _unpack_status(_rec(n_groups=0)) == _lib.SMM_ERR_INVALID and b"n_groups" in lib.smm_last_error()


def test_what_unpack_takes_without_a_device():
    """An empty call, a call of rows marked simple-packed and a call of rows without values have nothing to do: SMM_OK
    with no device looked for; a marked row passes through whatever its other fields hold."""
    assert _unpack_status(_rec(), n_batch=0, null=("x", "out", "recs", "rows_in", "rows_out")) == _lib.SMM_OK
    assert _unpack_status(_rec(order=-1, nbits=99, n_values=2 ** 40, reserved=5, byte_off=2 ** 50), out_bytes=0, null=("x", "out")) == _lib.SMM_OK
    assert _unpack_status(_rec(n_values=0, n_groups=0), out_bytes=0, null=("x", "out")) == _lib.SMM_OK


def test_layout_entry():
    lib = _lib.load()
    recs = np.concatenate([_rec(n_values=5), _rec(order=-1, n_values=777), _rec(n_values=2048), _rec(n_values=3, order=0)])
    offs, total = np.zeros(4, np.uint64), ctypes.c_uint64(0)
    ap = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct))               # noqa: E731
    assert lib.smm_grib_cpx_layout(ap(recs), 4, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(total)) == 0
    assert offs.tolist() == [0, 20, 20, 20 + 8192] and total.value == 20 + 8192 + 12          # 4 bytes per value; none for a marked row
    assert lib.smm_grib_cpx_layout(ap(recs), 4, None, ctypes.byref(total)) == 0 and total.value == 8224
    assert lib.smm_grib_cpx_layout(ap(recs), 4, None, None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_cpx_layout(ap(_rec(order=5)), 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID


def test_host_decode_entry_refusals_and_statuses():
    lib = _lib.load()
    c = xc.case("order2_noct3")
    values, status = np.zeros(c.n_values, np.uint32), ctypes.c_int(-1)
    vp = values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    ap = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct))               # noqa: E731
    sp, n = c.stream.ctypes.data_as(ctypes.c_void_p), c.stream.size
    rec = c.record(0).reshape(1)
    assert lib.smm_grib_cpx_decode_host(sp, n - 1, ap(rec), vp, ctypes.byref(status)) == _lib.SMM_ERR_INVALID      # leaves x_bytes
    assert lib.smm_grib_cpx_decode_host(sp, n, ap(rec), None, ctypes.byref(status)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_cpx_decode_host(sp, n, ap(rec), vp, None) == _lib.SMM_ERR_INVALID
    marked = rec.copy()
    marked["order"] = -1
    assert lib.smm_grib_cpx_decode_host(sp, n, ap(marked), vp, ctypes.byref(status)) == _lib.SMM_ERR_INVALID

    def status_of(stream=c.stream, **changes):
        r = xc.record(0, stream.size, c.n_values, dict(c.params, **changes)).reshape(1)
        values[:] = 7
        assert lib.smm_grib_cpx_decode_host(stream.ctypes.data_as(ctypes.c_void_p), stream.size, ap(r), vp, ctypes.byref(status)) == 0
        assert status.value == _lib.GRIB_CPX_OK or not values.any()        # a failed row leaves zeros, not numbers
        return status.value
    assert status_of() == _lib.GRIB_CPX_OK and np.array_equal(values, c.X)
    assert status_of(stream=c.stream[:20].copy()) == _lib.GRIB_CPX_EXHAUSTED            # the tables are cut
    assert status_of(stream=c.stream[:-9].copy()) == _lib.GRIB_CPX_EXHAUSTED            # the last groups' bits are cut
    assert status_of(length_last=c.params["length_last"] + 1) == _lib.GRIB_CPX_INVALID  # the lengths sum to n_values + 1
    assert status_of(length_last=c.params["length_last"] - 1) == _lib.GRIB_CPX_INVALID
    assert status_of(width_ref=33) == _lib.GRIB_CPX_INVALID                             # a group of 33 bits
    assert status_of(width_ref=c.params["width_ref"] + 1) == _lib.GRIB_CPX_EXHAUSTED    # the groups' bits pass the end
    assert status_of(n_groups=c.n_values + 1) == _lib.GRIB_CPX_INVALID                  # more groups than values
    signed = c.stream.copy()
    signed[0] |= 0x80                                                                   # h_1 < 0: X_0 leaves [0, 2^32)
    assert status_of(stream=signed) == _lib.GRIB_CPX_INVALID
    with pytest.raises(ValueError, match="is invalid"):
        griblite.cpx_decode(signed, c.record(0))


def grib_reason(dims, levels=False, out_dtype=np.float64, codec=None, mask_dim="isobaricInhPa", **switches):
    """why `road.decide` sends a `GribField` with these dims to the host decoder, or None: it stays raw"""
    from smmregrid_amd import road
    horizontal = [d for d in dims if d in ("lat", "lon", "latitude", "longitude")]
    way = road.decide(road.Switches.of(out_dtype=out_dtype, **switches),
                      road.Facts("t", road.GRIB, np.float32, dims, horizontal, mask_dim if levels else None, codec=codec))
    assert (way.source == road.RAW_GRIB) == (way.why is None) and way.source in (road.RAW_GRIB, road.DECODED)
    return way.why


def test_regridder_knows_why_a_complex_packed_field_is_decoded():
    """road.decide: masked levels, grib_out and a non-float64 result send a complex-packed field to the host."""
    on = dict(packed=True, packed_levels=True)
    dims = ("isobaricInhPa", "latitude", "longitude")
    assert grib_reason(dims, codec="cpx", **on) is None
    assert "complex packing" in grib_reason(dims, levels=True, codec="cpx", **on)
    assert "float32" in grib_reason(dims, out_dtype=np.float32, codec="cpx", **on)
    on["grib_out"] = True
    assert "grib_out" in grib_reason(dims, codec="cpx", **on)
    on["grib_out_ccsds"] = True
    assert "grib_out" in grib_reason(dims, codec="cpx", **on)
    assert grib_reason(dims, **on) is None
    on.update(grib_out=False, skipna=True)
    assert grib_reason(dims, codec="cpx", **on) == "skipna"
    on["packed_skipna"] = True
    assert grib_reason(dims, codec="cpx", **on) is None


def test_operator_refuses_cpx_with_ccsds_or_grib_out_before_any_device():
    from smmregrid_amd import GRIB_AEC_DTYPE, GribEncode, SparseOperator
    op = SparseOperator.__new__(SparseOperator)
    rows, cpx = np.zeros(2, dtype=GRIB_ROW_DTYPE), np.concatenate([_rec(), _rec()])
    buf = np.zeros(64, np.uint8)
    with pytest.raises(ValueError, match="ccsds"):
        op.apply_host_grib(buf, rows, cpx=cpx, ccsds=np.zeros(2, dtype=GRIB_AEC_DTYPE))
    with pytest.raises(ValueError, match="grib_out"):
        op.apply_host_grib(buf, rows, cpx=cpx, grib_out=GribEncode(16))
    with pytest.raises(ValueError, match="ccsds"):
        op.apply_grib(None, rows, cpx=cpx, ccsds=np.zeros(2, dtype=GRIB_AEC_DTYPE))


# ------------------------------------------------------------------------------------------------ malformed input
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib_cpx") / "grib_cpx_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_cpx_harness.cpp")])
    return exe


def test_malformed_input_ends_with_a_status_and_no_sanitizer_report(harness, tmp_path):
    """Truncated, corrupted and random input is tested here only, on the scalar decoder.  The GPU kernels take the tables
    apart with the same functions, but raise their statuses in kernels of their own: malformed rows with the status each
    must end with go through both in tests/test_grib_complex_seams.py and tests/test_gpu_grib_complex_seams.py."""
    cs = [c for c in CASES if c.n_values <= 4096]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.int64(len(cs)).tobytes())
        for c in cs:
            fh.write(np.array([c.n_values] + [c.params[k] for k in xc.PARAM_NAMES] + [c.stream.size], np.int64).tobytes())
            fh.write(c.stream.tobytes())
            fh.write(c.X.astype(np.uint32).tobytes())
    out = subprocess.run([harness, path], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cs)
    INVALID, EXHAUSTED = _lib.GRIB_CPX_INVALID, _lib.GRIB_CPX_EXHAUSTED
    for c, ln in zip(cs, lines):
        runs, ok, exhausted, invalid = int(ln[3]), int(ln[5]), int(ln[7]), int(ln[9])
        plus, minus, w33, wider, sign = (int(v) for v in ln[11:16])
        assert runs == ok + exhausted + invalid and runs >= 6 + c.stream.size + c.stream.size // 7
        assert exhausted >= c.stream.size - 8, (c, ln)         # a cut stream runs out (but for the pad bits)
        assert plus == minus == w33 == INVALID, (c, ln)
        if c.n_values >= 8:                                    # (fewer extra bits than a last octet may have to spare)
            assert wider == (INVALID if c.name == "order0_widths_0_1_31_32" else EXHAUSTED), (c, ln)
        heads = c.X[0] != 0 if c.order else False
        assert sign == (INVALID if heads else 9), (c, ln)
    rand = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("random ")]
    assert len(rand) == 1 and int(rand[0][2]) == 6000
    ok, exhausted, invalid = int(rand[0][4]), int(rand[0][6]), int(rand[0][8])
    assert ok + exhausted + invalid == 6000 and ok > 0 and exhausted > 0 and invalid > 0, rand
