"""Regrid results returned GRIB simple-packed (smm_apply_host_grib_pk, `grib_pack`, `Regridder(grib_out=True)`): every
comparison is bytes for bytes against `GribEncode.encode` of the float64 result the existing entry gives for the same
call -- the row records, the bitmap records and the whole buffer."""
import numpy as np
import pytest

from smmregrid_amd import (CdoGenerate, DataArray, GribEncode, GribField, Regridder, _lib, grib_pack, pinned_empty,
                           to_device)
from smmregrid_amd.io import open_dataset
from tests import grib_cases
from tests.test_gpu_grib import device_bytes, grib2_12bit, operator, same_bits
from tests.test_gpu_grib_bitmap import build_bm, grib2_sst, random_bitmaps

pytestmark = pytest.mark.gpu

WIDTHS_OUT = (16, 12, 7, 24, 17, 32, 1)
DECIMALS_OUT = (0, 2, -1, 0, 3, 0, 1)


def same_field(got, want, what=""):
    assert isinstance(got, GribField) and got.shape == want.shape and got.n_points == want.n_points, what
    for b in range(want.rows.size):
        assert got.rows[b].tobytes() == want.rows[b].tobytes(), (what, b, got.rows[b], want.rows[b])
        assert got.bitmaps[b].tobytes() == want.bitmaps[b].tobytes(), (what, b, got.bitmaps[b], want.bitmaps[b])
    buf = np.asarray(got.buf)[:want.buf.size]
    diff = np.flatnonzero(buf != want.buf)
    assert diff.size == 0, f"{what}: {diff.size} bytes differ, first at {diff[:5].tolist()}"


def case(name, bitmapped, seed=21):
    """Seven rows of mixed widths over the operator's source grid, with or without bitmaps."""
    rng = np.random.default_rng(seed)
    S = operator(name)[0].n_src
    specs = grib_cases.row_specs(rng, S, 7, (16, 12, 0, 24, 17, 7, 32), D=(0, 1))
    if bitmapped:
        specs = random_bitmaps(rng, specs, S)
        specs[2]["bitmap"] = None                                   # one row without a bitmap among them
        buf, rows, bitmaps, _ = build_bm(specs, rng, tail_residue=1)
        return buf, rows, bitmaps
    buf, rows, _ = grib_cases.build(specs, rng, tail_residue=1)
    return buf, rows, None


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("bitmapped", [False, True])
@pytest.mark.parametrize("name", ["bil_r180x90_r90x45", "ragged_random", "tiny"])
def test_apply_host_grib_out_is_the_encode_of_the_float64_result(hip, name, bitmapped, skipna):
    op = operator(name)[0]
    buf, rows, bitmaps = case(name, bitmapped)
    enc = GribEncode(WIDTHS_OUT, DECIMALS_OUT)
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        kw = dict(masked=masked, remap_area_min=area_min, bitmaps=bitmaps, skipna=skipna)
        y = op.apply_host_grib(buf, rows, **kw)
        want = enc.encode(y)
        got = op.apply_host_grib(buf, rows, grib_out=enc, **kw)
        same_field(got, want, f"{name} bitmapped={bitmapped} skipna={skipna} masked={masked}")
        assert np.array_equal(np.asarray(got), want.decode(), equal_nan=True)


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("chunk_rows", [1, 2, 3, 0])
def test_chunks_result_buffers_and_the_bytes_that_crossed(hip, pinned, chunk_rows):
    name = "bil_r180x90_r90x45"
    op = operator(name)[0]
    D = op.n_dst
    buf, rows, bitmaps = case(name, True, seed=22)
    enc = GribEncode(WIDTHS_OUT, DECIMALS_OUT)
    want = enc.encode(op.apply_host_grib(buf, rows, bitmaps=bitmaps, masked=True, remap_area_min=0.5))
    _, total = enc.layout(D, 7)
    assert total == want.buf.size
    tail = 64
    out = pinned_empty(total + tail, np.uint8) if pinned else np.empty(total + tail, np.uint8)
    out[:] = 0xEE
    _lib.host_stats(reset=True)
    got = op.apply_host_grib(buf, rows, bitmaps=bitmaps, masked=True, remap_area_min=0.5, chunk_rows=chunk_rows,
                             grib_out=enc, out=out)
    st = _lib.host_stats(reset=True)
    same_field(got, want, f"pinned={pinned} chunk_rows={chunk_rows}")
    assert got.buf is out and (out[total:] == 0xEE).all()            # nothing behind the layout was touched
    assert st["calls"] == 1 and st["chunks"] == {1: 7, 2: 4, 3: 3, 0: 1}[chunk_rows]
    assert st["d2h_bytes"] == total + 7 * (40 + 16)                   # the slots and the records, not 7 * D * 8
    assert st["d2h_bytes"] < 7 * D * 8


def test_a_failed_chunk_drains_and_the_next_packed_call_succeeds(hip):
    name = "ragged_random"
    op = operator(name)[0]
    buf, rows, bitmaps = case(name, True, seed=23)
    enc = GribEncode(16, 1)
    want = enc.encode(op.apply_host_grib(buf, rows, bitmaps=bitmaps))
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        with pytest.raises(_lib.SmmError, match="injected failure"):
            op.apply_host_grib(buf, rows, bitmaps=bitmaps, chunk_rows=3, grib_out=enc)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    same_field(op.apply_host_grib(buf, rows, bitmaps=bitmaps, chunk_rows=3, grib_out=enc), want, "after the failure")


def test_grib_pack_feeds_apply_grib_on_the_device(hip):
    """grib_pack -> apply_grib(bitmaps=) chained in HBM: the bits of regridding the decoded packed field."""
    name = "tiny"
    op = operator(name)[0]
    rng = np.random.default_rng(31)
    v = rng.normal(280.0, 10.0, (5, op.n_src))
    v[1, rng.random(op.n_src) < 0.3] = np.nan
    v[3, :] = np.nan
    v[4, :] = 7.5
    enc = GribEncode([16, 12, 24, 16, 9], [0, 1, 0, 0, 2])
    packed, rows, bitmaps = grib_pack(to_device(v), enc)
    want_field = enc.encode(v)
    assert rows.tobytes() == want_field.rows.tobytes() and bitmaps.tobytes() == want_field.bitmaps.tobytes()
    got = op.apply_grib(packed, rows, x_bytes=want_field.buf.size, bitmaps=bitmaps).to_host()
    field = want_field.decode()
    want = op.apply(to_device(field), flags=_lib.APPLY_KERNEL_SELL).to_host()
    same_bits(got, want, "grib_pack -> apply_grib")
    again = op.apply_grib(device_bytes(want_field.buf), want_field.rows, x_bytes=want_field.buf.size,
                          bitmaps=want_field.bitmaps).to_host()
    same_bits(again, want, "the host encode through the same entry")


# ---------------------------------------------------------------------------------------------- Regridder

def grib_out_lines(caplog):
    return [r.getMessage() for r in caplog.records if r.getMessage().startswith("grib_out:")]


@pytest.mark.parametrize("kw", [dict(), dict(skipna=True, packed_skipna=True)])
def test_regridder_returns_a_grib_field_that_ships_raw_again(hip, tmp_path, caplog, kw):
    path, var, plain = grib2_sst(tmp_path, np.random.default_rng(70))
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    w = CdoGenerate(dec[var], "r12x6").weights(method="con")
    caplog.clear()
    y = Regridder(weights=w, packed=True, **kw).regrid(raw)
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, grib_out=True, loglevel="INFO", **kw).regrid(raw)
    assert not grib_out_lines(caplog)
    for name in (var, plain):                                        # bitmapped and not
        src = raw[name].data
        f = got[name].data
        assert got[name].dims == y[name].dims and f.shape == y[name].values.shape       # (step, lat, lon)
        want = GribEncode.from_field(src).encode(np.asarray(y[name].values).reshape(src.rows.size, -1))
        same_field(GribField(f.buf, f.rows, want.shape, f.n_points, bitmaps=f.bitmaps), want, name)
        assert f.rows["nbits"].max() == src.rows["nbits"].max() and (f.rows["ddiv"] == src.rows["ddiv"]).all()
        decoded = np.asarray(got[name].values)
        assert decoded.dtype == np.float32 and np.array_equal(decoded, want.decode().reshape(f.shape), equal_nan=True)
    assert np.isnan(np.asarray(got[var].values)).any() == np.isnan(y[var].values).any()
    # the packed result regridded once more, raw: the bits of regridding its float32 decode
    w2 = CdoGenerate(got[plain], "r6x3").weights(method="con")
    names = []
    real = _lib.call
    try:
        _lib.call = lambda name, *a: names.append(name) or real(name, *a)
        second = Regridder(weights=w2, packed=True).regrid(got[plain])
    finally:
        _lib.call = real
    assert any(n.startswith("smm_apply_host_grib") for n in names)
    g = got[plain]
    ref = Regridder(weights=w2).regrid(DataArray(np.asarray(g.values), dims=g.dims, coords=g.coords, attrs=g.attrs,
                                                 name=g.name))
    same_bits(np.asarray(second.values), np.asarray(ref.values), "second regrid, raw")


def test_regridder_fallbacks_log_one_line_and_the_refusals_fire(hip, tmp_path, caplog):
    path, var = grib2_12bit(tmp_path, np.random.default_rng(12))
    dec, raw = open_dataset(path), open_dataset(path, decode=False)
    w = CdoGenerate(dec[var], "r12x6").weights(method="con")
    want = Regridder(weights=w).regrid(dec[var])
    # a float variable
    caplog.clear()
    with caplog.at_level("INFO"):
        out = Regridder(weights=w, packed=True, grib_out=True, loglevel="INFO").regrid(dec[var])
    lines = grib_out_lines(caplog)
    assert len(lines) == 1 and "not a raw GRIB variable" in lines[0]
    same_bits(np.asarray(out.values), np.asarray(want.values), "float variable")
    # decoded on the host: skipna without packed_skipna
    caplog.clear()
    with caplog.at_level("INFO"):
        out = Regridder(weights=w, packed=True, grib_out=True, skipna=True, loglevel="INFO").regrid(raw[var])
    lines = grib_out_lines(caplog)
    assert len(lines) == 1 and "decoded on the host" in lines[0] and out.values.dtype == np.float64
    # masked-level weights, decoded or raw
    w3 = CdoGenerate(dec[var], "r12x6").weights(method="con", mask_dim="isobaricInhPa")
    want3 = Regridder(weights=w3).regrid(dec[var])
    for more in (dict(), dict(packed_levels=True)):
        caplog.clear()
        with caplog.at_level("INFO"):
            out = Regridder(weights=w3, packed=True, grib_out=True, loglevel="INFO", **more).regrid(raw[var])
        lines = grib_out_lines(caplog)
        assert len(lines) == 1 and ("masked levels" in lines[0] or "decoded on the host" in lines[0]), lines
        same_bits(np.asarray(out.values), np.asarray(want3.values), f"masked levels {more}")
    # the refusals
    for bad in (dict(grib_out=True), dict(grib_out=True, packed=True, lazy=True),
                dict(grib_out=True, packed=True, out_dtype=np.float32)):
        with pytest.raises(ValueError):
            Regridder(weights=w, **bad)
    # packed_out alone keeps its meaning: a GRIB variable stays float64
    out = Regridder(weights=w, packed=True, packed_out=True).regrid(raw[var])
    assert not isinstance(out.data, GribField)
    same_bits(np.asarray(out.values), np.asarray(want.values), "packed_out alone")
