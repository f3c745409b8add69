"""`GribEncode`: the numpy statement of the GRIB encode rule (smm_grib_codec.hpp) -- the layout arithmetic, the
refusals of the class and of the C entries (which answer before any device is touched), `from_field`, and the
properties of the rule itself: what decodes back, where the missing cells are, the error bound and the range of q."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_ENCODE_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribEncode, GribField,
                           _lib)
from smmregrid_amd.griblite import _decode_rule, _unpack_bits
from tests import grib_pack_cases as pc

FLT_MAX = float(np.finfo(np.float32).max)


def align4(n):
    return (n + 3) // 4 * 4


# ------------------------------------------------------------------ layout

@pytest.mark.parametrize("n", [0, 1, 7, 8, 9, 31, 32, 33, 1000, 32769])
def test_layout_arithmetic(n):
    widths = [1, 7, 12, 16, 17, 24, 25, 31, 32]
    enc = GribEncode(widths)
    offs, total = enc.layout(n, len(widths))
    at = 0
    for b, w in enumerate(widths):
        assert int(offs[b]) == at and at % 4 == 0
        at += align4((n + 7) // 8) + align4((n * w + 7) // 8)
    assert total == at
    # the C entry agrees
    rec = enc.records(len(widths))
    c_offs = np.zeros(len(widths), dtype=np.uint64)
    c_total = ctypes.c_uint64(0)
    _lib.call("smm_grib_out_layout", n, ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)), len(widths),
              c_offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(c_total))
    assert c_total.value == total and np.array_equal(c_offs, offs)
    _lib.call("smm_grib_out_layout", n, ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)), len(widths),
              None, ctypes.byref(c_total))                           # the offsets may be left out
    assert c_total.value == total


def test_scalar_rule_serves_any_number_of_fields_and_a_list_only_its_own():
    assert GribEncode(16).layout(10, 3)[1] == 3 * (4 + 20)
    assert GribEncode(12, 2).records(4)["ddiv"].tolist() == [100.0] * 4
    assert GribEncode([16, 12], [0, 1]).records(2)["nbits"].tolist() == [16, 12]
    with pytest.raises(ValueError):
        GribEncode([16, 12]).layout(10, 3)
    assert GRIB_ENCODE_DTYPE.itemsize == ctypes.sizeof(_lib.GribEncodeStruct) == 16


# ------------------------------------------------------------------ refusals

@pytest.mark.parametrize("args", [(0,), (33,), (-1,), ([16, 0],), (16.0,), (16, 0.5), (16, 400), (16, -400),
                                  ([16, 12], [0, 1, 2]), ([[16]],)])
def test_class_refusals(args):
    with pytest.raises(ValueError):
        GribEncode(*args)


def test_layout_refuses_2_31_points():
    GribEncode(1).layout(2 ** 31 - 1, 1)
    with pytest.raises(ValueError):
        GribEncode(1).layout(2 ** 31, 1)


def _enc(nbits=16, ddiv=1.0, reserved=0, n=1):
    rec = np.zeros(n, dtype=GRIB_ENCODE_DTYPE)
    rec["ddiv"], rec["nbits"], rec["reserved"] = ddiv, nbits, reserved
    return rec


def _pack_status(rec, y=0x1000, ldy=8, n_dst=8, out=0x2000, out_bytes=1 << 20, n_batch=None):
    """smm_grib_pack with pointers that are never followed: every refusal comes before the device is touched."""
    n_batch = rec.size if n_batch is None else n_batch
    rows = np.zeros(max(n_batch, 1), dtype=GRIB_ROW_DTYPE)
    bms = np.zeros(max(n_batch, 1), dtype=GRIB_BITMAP_DTYPE)
    return _lib.load().smm_grib_pack(0, ctypes.c_void_p(y), ldy, n_dst, n_batch,
                                     ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)),
                                     ctypes.c_void_p(out), out_bytes,
                                     ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
                                     ctypes.cast(bms.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), None)


@pytest.mark.parametrize("kw", [dict(rec=_enc(nbits=0)), dict(rec=_enc(nbits=33)), dict(rec=_enc(ddiv=0.0)),
                                dict(rec=_enc(ddiv=-10.0)), dict(rec=_enc(ddiv=np.inf)), dict(rec=_enc(ddiv=np.nan)),
                                dict(rec=_enc(reserved=1)), dict(rec=_enc(), out_bytes=4 + 16 - 1),
                                dict(rec=_enc(), out=0x2002), dict(rec=_enc(), y=0x1004), dict(rec=_enc(), ldy=7),
                                dict(rec=_enc(), n_dst=2 ** 31, ldy=2 ** 31, out_bytes=2 ** 40),
                                dict(rec=_enc(), n_batch=-1)])
def test_pack_entry_refuses_before_any_device(kw):
    assert _pack_status(**kw) == _lib.SMM_ERR_INVALID


def test_host_entry_refuses_before_any_device():
    """smm_apply_host_grib_pk: the encode records, then the handle -- a NULL operator is SMM_ERR_INVALID, a bad rule
    too, and SMM_APPLY_KERNEL_TILE is what the GRIB entries make of it today (SMM_ERR_UNSUPPORTED)."""
    lib = _lib.load()
    rows = np.zeros(1, dtype=GRIB_ROW_DTYPE)
    rows["bscale"], rows["ddiv"], rows["nbits"] = 1.0, 1.0, 16
    out_rows, out_bms = np.zeros(1, dtype=GRIB_ROW_DTYPE), np.zeros(1, dtype=GRIB_BITMAP_DTYPE)
    buf, out = np.zeros(64, np.uint8), np.zeros(64, np.uint8)

    def status(rec, flags=0):
        return lib.smm_apply_host_grib_pk(None, buf.ctypes.data_as(ctypes.c_void_p), buf.size,
                                          ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)), None,
                                          ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)),
                                          out.ctypes.data_as(ctypes.c_void_p), out.size,
                                          ctypes.cast(out_rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
                                          ctypes.cast(out_bms.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), 1, 0.0,
                                          flags, 0)
    assert status(_enc()) == _lib.SMM_ERR_INVALID                    # the NULL handle
    assert b"null operator" in lib.smm_last_error()
    assert status(_enc(), _lib.APPLY_KERNEL_TILE) == _lib.SMM_ERR_UNSUPPORTED
    assert status(_enc(), 1 << 20) == _lib.SMM_ERR_INVALID


# ------------------------------------------------------------------ from_field

def _field(nbits, ddiv):
    rows = np.zeros(len(nbits), dtype=GRIB_ROW_DTYPE)
    rows["nbits"], rows["ddiv"], rows["bscale"] = nbits, ddiv, 1.0
    return GribField(np.zeros(8, np.uint8), rows, (len(nbits), 1), 1)


def test_from_field_takes_each_rows_width_and_d():
    enc = GribEncode.from_field(_field([16, 12, 0, 24], [1.0, 100.0, 0.01, 1e3]))
    assert enc.nbits.tolist() == [16, 12, 24, 24]                    # the constant row: the variable's largest width
    assert enc.decimal_scale.tolist() == [0, 2, -2, 3]
    assert enc.ddiv.tolist() == [1.0, 10.0 ** 2, 10.0 ** -2, 10.0 ** 3]
    assert GribEncode.from_field(_field([0, 0], [1.0, 1.0])).nbits.tolist() == [16, 16]
    for bad in (3.0, 99.99999999999999, np.nextafter(100.0, 200.0)):
        with pytest.raises(ValueError):
            GribEncode.from_field(_field([16], [bad]))


# ------------------------------------------------------------------ the rule

def check_rule(values, nbits, dec):
    """Every property of the rule on one batch; returns the worst ratio error / bound."""
    enc = GribEncode(nbits, dec)
    f = enc.encode(values)
    back32 = f.decode()
    worst = 0.0
    for b in range(values.shape[0]):
        v, w, ddiv = values[b], int(nbits[b]), float(enc.ddiv[b])
        with np.errstate(over="ignore", invalid="ignore"):
            t = v * ddiv
            present = np.isfinite(v) & (np.abs(t) <= FLT_MAX)
        assert np.array_equal(np.isnan(back32[b]), ~present)         # missing exactly where non-finite or overflowing
        r, bm = f.rows[b], f.bitmaps[b]
        assert int(bm["n_values"]) == int(present.sum())
        assert (int(bm["bitmap_off"]) == GRIB_NO_BITMAP) == bool(present.all())
        assert int(r["nbits"]) in (0, w) and int(r["reserved"]) == 0 and float(r["ddiv"]) == ddiv
        if not present.any():
            assert float(r["ref"]) == 0.0 and int(r["nbits"]) == 0 and float(r["bscale"]) == 1.0
            continue
        tp = t[present]
        ref, bscale = float(r["ref"]), float(r["bscale"])
        E = int(np.log2(bscale))
        assert np.ldexp(1.0, E) == bscale and E >= -1022
        assert ref == float(np.float32(ref)) and ref <= tp.min()
        assert ref != 0.0 or not np.signbit(ref)
        assert float(np.nextafter(np.float32(ref), np.float32(np.inf))) > tp.min()     # the LARGEST float32 <= tmin
        if int(r["nbits"]) == 0:
            assert tp.max() - ref == 0.0
            q = np.zeros(tp.size)
        else:
            q = np.rint(np.ldexp(tp - ref, -E))
            assert q.min() >= 0 and q.max() <= 2 ** w - 1
            n = tp.size
            raw = bytes(f.buf[int(r["byte_off"]):int(r["byte_off"]) + (n * w + 7) // 8])
            assert np.array_equal(_unpack_bits(raw, w, n), q)         # the stream holds exactly these q
            # E is the smallest that fits
            rng_ = tp.max() - ref
            assert np.ldexp(rng_, -E) <= 2 ** w - 1
            assert E == -1022 or np.ldexp(rng_, -(E - 1)) > 2 ** w - 1
        # the float64 decode (the float32 of GribField.decode would add its own rounding) against v
        bmrec = None if int(bm["bitmap_off"]) == GRIB_NO_BITMAP else (int(bm["bitmap_off"]), int(bm["n_values"]))
        back = _decode_rule(f.buf, (int(r["byte_off"]), ref, bscale, ddiv, int(r["nbits"])), v.size, bmrec)
        err = np.abs(back[present] - v[present])
        half = 0.0 if int(r["nbits"]) == 0 else np.ldexp(1.0, E - 1)
        bound = (half + 4 * np.spacing(max(abs(tp.min()), abs(tp.max()), abs(ref)))) / ddiv * (1 + 2.0 ** -50)
        assert (err <= bound).all(), (b, w, float(err.max()), bound)
        if bound > 0:
            worst = max(worst, float(err.max()) / bound)
    return worst


@pytest.mark.parametrize("n_dst", [1, 33, 257])
def test_rule_on_the_adversarial_rows(n_dst):
    values, nbits, dec, _ = pc.batch(n_dst, seed=3 + n_dst)
    assert check_rule(values, nbits, dec) <= 1.0


def test_rule_on_random_rows():
    """Widths 1..32, D in {-2, 0, 3}, magnitudes 1e-30..1e30, ranges down to adjacent doubles."""
    rng = np.random.default_rng(20261019)
    worst = 0.0
    for _ in range(40):
        n_rows, n = 50, int(rng.integers(1, 40))
        mag = 10.0 ** rng.uniform(-30, 30, (n_rows, 1))
        spread = np.where(rng.random((n_rows, 1)) < 0.2, 2.0 ** -rng.integers(40, 53, (n_rows, 1)),
                          10.0 ** rng.uniform(-6, 0, (n_rows, 1)))
        values = mag * (rng.choice([-1.0, 1.0], (n_rows, 1)) + spread * rng.normal(0, 1, (n_rows, n)))
        values[rng.random(values.shape) < 0.1] = np.nan
        worst = max(worst, check_rule(values, rng.integers(1, 33, n_rows).astype(np.int32), rng.choice([-2, 0, 3], n_rows)))
    assert 0.0 < worst <= 1.0


def test_ties_go_to_even_and_a_negative_zero_reference_is_stored_positive():
    v = np.array([[0.0, 0.5, 1.5, 2.5, 3.5, 255.0]])
    f = GribEncode(8).encode(v)
    assert float(f.rows[0]["bscale"]) == 1.0
    assert f.buf[int(f.rows[0]["byte_off"]):][:6].tolist() == [0, 0, 2, 2, 4, 255]
    for zeros in ([-0.0, 0.0, 1.0], [0.0, -0.0, 1.0], [-0.0, -0.0, 1.0]):
        r = GribEncode(8).encode(np.array([zeros])).rows[0]
        assert float(r["ref"]) == 0.0 and not np.signbit(float(r["ref"]))
    r = GribEncode(8).encode(np.array([[-0.0, 0.0]])).rows[0]
    assert int(r["nbits"]) == 0 and not np.signbit(float(r["ref"]))


def test_encode_output_feeds_decode_and_keeps_the_shape():
    v = np.random.default_rng(1).normal(0, 1, (2, 3, 50))
    v[1, 2, ::5] = np.nan
    f = GribEncode(16, 2).encode(v)
    assert f.shape == (2, 3, 50) and f.rows.size == 6 and f.n_points == 50 and f.bitmaps is not None
    back = np.asarray(f)
    assert back.dtype == np.float32 and np.array_equal(np.isnan(back), np.isnan(v))
    assert np.nanmax(np.abs(back - v)) < 1e-2
