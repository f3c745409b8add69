"""Regrid results on masked-level (3-D) weights returned GRIB simple-packed (smm_group_apply_host_grib_pk,
`OperatorGroup.apply_host_grib(grib_out=)`, `Regridder(grib_out_levels=True)`): every comparison is bytes for bytes
against `GribEncode.encode` of the float64 result the existing entry gives for the same call, taken in record order
(n_outer, n_lev, n_inner, D) -- the row records, the bitmap records and the whole buffer; once per case the float64
result is taken per level from the CPU oracle (plain) or from the restated SKIPNA rule of tests/helpers.py instead.
Geometry: the "std" one of tests/test_gpu_packed_levels.py (S = 2592, D = 288, 8 levels, masked_levels switching the
masks of members 1 and 5 off); fields from `level_case` of tests/test_gpu_grib_levels.py.

The kinds of result row, asserted on the expectation before anything is compared: a row without a bitmap (every cell
present), a row with a bitmap and 0 < n_values < D, and a row with n_values == 0 and stored width 0.  Every case has
all three in its masked call at remap_area_min 0 -- the epilogue (True, 0.0), which is also the one compared with the
CPU result -- and a partial row under every epilogue.  The other two epilogues cannot hold all three whatever the field:
without the mask a destination cell that has no link at a level is 0.0, a present cell, so no row of that level is
empty; and remap_area_min 0.5 drops the cells of dst_frac < 0.5 on the unmasked levels too, so no row need be full.
`level_case(edges=True)` gives the empty rows -- its last-but-one level has all-zero bitmaps -- and the partial ones; its
only row without a bitmap lies on a masked level, so a bitmapped case takes the rows of one unmasked level from a second
`level_case` without bitmaps, appended to the same buffer.  A call without bitmap records has no empty level: there
the rows of the last-but-one level become the constant 1e30, which the epilogue turns into missing cells (y > 1e19)."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CdoGenerate, GribEncode, GribField, Regridder,
                           SparseOperator, _lib, gridgen, pinned_empty)
from smmregrid_amd.io import open_dataset
from tests import grib_cases
from tests.helpers import skipna_ref
from tests.test_gpu_grib import same_bits
from tests.test_gpu_grib_levels import D_STD, level_case, oracle_levels, staged_bytes
from tests.test_gpu_grib_out import DECIMALS_OUT, WIDTHS_OUT, grib_out_lines, same_field
from tests.test_gpu_packed_levels import EPILOGUES, L, LEVEL_SETS, NX, NY, S, geometry
from tests.test_griblite import encode2

pytestmark = pytest.mark.gpu


def cycled_encode(n_rows):
    k = np.arange(n_rows) % len(WIDTHS_OUT)
    return GribEncode(np.asarray(WIDTHS_OUT)[k], np.asarray(DECIMALS_OUT)[k])


def mixed_case(rng, g, n_outer, lev, n_inner, bitmapped, edges=True, **kw):
    """`level_case` with all three kinds of result row in reach (the module's docstring)."""
    lev = np.asarray(lev, dtype=np.int32)
    buf, rows, bitmaps, field = level_case(rng, g["masks"], n_outer, lev, n_inner, bitmapped=bitmapped, edges=edges, **kw)
    open_levels = [k for k, w in enumerate(lev) if not g["masked_levels"][w] and (not edges or k != len(lev) - 2)]
    if bitmapped and open_levels:
        k = open_levels[-1]
        buf2, rows2, _, field2 = level_case(rng, g["masks"], n_outer, lev, n_inner, bitmapped=False)
        rows[:, k] = rows2[:, k]
        rows["byte_off"][:, k] += buf.size
        bitmaps["bitmap_off"][:, k], bitmaps["n_values"][:, k] = GRIB_NO_BITMAP, S
        field[:, k] = field2[:, k]
        buf = np.concatenate([buf, buf2])
    if not bitmapped and edges:
        k = len(lev) - 2
        for name, v in (("ref", 1e30), ("bscale", 1.0), ("ddiv", 1.0), ("nbits", 0)):
            rows[name][:, k] = v
        field[:, k] = grib_cases.decode_rows(buf, np.ascontiguousarray(rows[:, k]).ravel(), S).reshape(field[:, k].shape)
        assert (field[:, k] == np.float32(1e30)).all()
    return buf, rows, bitmaps, field


def assert_kinds(want, what, all_three=True):
    """A partial row always; with all_three a row without a bitmap and an empty row of stored width 0 as well."""
    bm, rows = want.bitmaps, want.rows
    D = want.n_points
    assert (bm["n_values"][bm["bitmap_off"] == GRIB_NO_BITMAP] == D).all(), what
    assert ((bm["bitmap_off"] != GRIB_NO_BITMAP) & (bm["n_values"] > 0) & (bm["n_values"] < D)).any(), what
    if all_three:
        assert (bm["bitmap_off"] == GRIB_NO_BITMAP).any(), what
        assert ((bm["n_values"] == 0) & (rows["nbits"] == 0)).any(), what


def record_order(y):
    """(n_outer, n_inner, n_lev, D) of a transpose=True call -> (n_outer, n_lev, n_inner, D)"""
    return np.ascontiguousarray(np.moveaxis(y, 2, 1))


def outside_result(g, field, lev, ml, masked, area_min, skipna):
    """The float64 result per level without the GPU: oracle.apply_c, or under skipna the restated rule."""
    if not skipna:
        return np.ascontiguousarray(np.moveaxis(oracle_levels(g, field, lev, masked, area_min, False, ml), 0, 1))
    out = np.empty(field.shape[:3] + (D_STD,))
    for k, w in enumerate(lev):
        x = np.ascontiguousarray(field[:, k]).reshape(-1, S)
        y = skipna_ref(g["csrs"][w], x, masked and bool(ml[w]), g["imask"][w], g["frac"][w], area_min)
        out[:, k] = y.reshape(field.shape[0], field.shape[2], D_STD)
    return out


# ---------------------------------------------------------------- 1: bytes and records

@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("bitmapped", [True, False])
@pytest.mark.parametrize("n_inner", [1, 2])
@pytest.mark.parametrize("n_outer", [1, 2, 3, 5])
def test_group_grib_out_is_the_encode_of_the_float64_result(hip, n_outer, n_inner, bitmapped, skipna):
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    assert (grp.n_src, grp.n_dst) == (S, D_STD) and ml.tolist() == [1, 0, 1, 1, 1, 0, 1, 1]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(6000 + 100 * n_outer + 10 * n_inner + 2 * bitmapped + skipna)
    buf, rows, bitmaps, field = mixed_case(rng, g, n_outer, lev, n_inner, bitmapped)
    enc = cycled_encode(rows.size)
    for masked, area_min in EPILOGUES:
        kw = dict(masked=masked, remap_area_min=area_min, bitmaps=bitmaps, skipna=skipna)
        what = f"{n_outer}x{L}x{n_inner} bitmapped={bitmapped} skipna={skipna} masked={masked} area_min={area_min}"
        y = record_order(grp.apply_host_grib(buf, rows, lev, ml, **kw))
        assert y.shape == (n_outer, L, n_inner, D_STD)
        want = enc.encode(y)
        assert_kinds(want, what, all_three=(masked, area_min) == (True, 0.0))
        got = grp.apply_host_grib(buf, rows, lev, ml, grib_out=enc, **kw)
        assert got.shape == (n_outer, L, n_inner, D_STD)
        same_field(got, want, what)
        assert np.array_equal(np.asarray(got), want.decode(), equal_nan=True)
        if (masked, area_min) == (True, 0.0):      # once per case the expectation from outside the GPU float path
            outside = enc.encode(outside_result(g, field, lev, ml, masked, area_min, skipna))
            assert_kinds(outside, what + " (CPU result)")
            same_field(got, outside, what + " against the CPU result")


# ---------------------------------------------------------------- 2: chunks, buffers, bytes

_CASE = {}


def chunk_case():
    """5 x 8 x 2 bitmapped rows, masked, all three kinds of result row; the expectation tied to the oracle once."""
    if not _CASE:
        g = geometry("std")
        lev = np.arange(L, dtype=np.int32)
        buf, rows, bitmaps, field = mixed_case(np.random.default_rng(6500), g, 5, lev, 2, True, tail_residue=3)
        enc = cycled_encode(rows.size)
        kw = dict(bitmaps=bitmaps, masked=True, remap_area_min=0.0)
        y = record_order(g["grp"].apply_host_grib(buf, rows, lev, g["masked_levels"], **kw))
        want = enc.encode(y)
        assert_kinds(want, "chunk case")
        same_field(enc.encode(outside_result(g, field, lev, g["masked_levels"], True, 0.0, False)), want, "chunk case vs oracle")
        _CASE.update(g=g, lev=lev, buf=buf, rows=rows, bitmaps=bitmaps, enc=enc, kw=kw, want=want, y=y)
    return _CASE


@pytest.mark.parametrize("out_kind", ["pageable", "pinned", "none"])
@pytest.mark.parametrize("chunk_outer", [1, 2, 3, 0])
def test_chunks_result_buffers_and_the_bytes_that_crossed(hip, chunk_outer, out_kind):
    c = chunk_case()
    grp, ml, buf, rows, bitmaps, enc, want = c["g"]["grp"], c["g"]["masked_levels"], c["buf"], c["rows"], c["bitmaps"], c["enc"], c["want"]
    n_rows = rows.size
    _, total = enc.layout(D_STD, n_rows)
    assert total == want.buf.size
    tail = 64
    out = {"pageable": lambda: np.empty(total + tail, np.uint8), "pinned": lambda: pinned_empty(total + tail, np.uint8),
           "none": lambda: None}[out_kind]()
    if out is not None:
        out[:] = 0xEE
    _lib.host_stats(reset=True)
    grp.apply_host_grib(buf, rows, c["lev"], ml, chunk_outer=chunk_outer, **c["kw"])
    st_float = _lib.host_stats(reset=True)
    got = grp.apply_host_grib(buf, rows, c["lev"], ml, chunk_outer=chunk_outer, grib_out=enc, out=out, **c["kw"])
    st = _lib.host_stats(reset=True)
    same_field(got, want, f"chunk_outer={chunk_outer} out={out_kind}")
    if out is not None:
        assert got.buf is out and (out[total:] == 0xEE).all()           # nothing behind the layout was touched
    per = {1: 1, 2: 2, 3: 3, 0: 5}[chunk_outer]
    chunks = [(o, min(o + per, 5)) for o in range(0, 5, per)]
    assert st["calls"] == 1 and st["chunks"] == st_float["chunks"] == len(chunks)
    assert st["d2h_bytes"] == total + 56 * n_rows                        # the slots and the records, not rows * D * 8
    assert st["d2h_bytes"] < st_float["d2h_bytes"] == n_rows * D_STD * 8
    staged = [staged_bytes(rows[a:b], bitmaps[a:b]) for a, b in chunks]
    assert st_float["h2d_bytes"] == sum(staged)
    pad = sum(-s % 8 for s in staged)                                    # the pack tables start 8-byte aligned
    assert st["h2d_bytes"] == st_float["h2d_bytes"] + 48 * n_rows + pad


# ---------------------------------------------------------------- 3: level subsets and order

@pytest.mark.parametrize("name,lev", [("subset", LEVEL_SETS["subset"]), ("single", [3]), ("reversed", LEVEL_SETS["reversed"])])
def test_level_subsets_and_order(hip, name, lev):
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.asarray(lev, dtype=np.int32)
    rng = np.random.default_rng(6600 + len(lev))
    buf, rows, bitmaps, field = mixed_case(rng, g, 3, lev, 2, True, edges=False)
    enc = cycled_encode(rows.size)
    for skipna in (False, True):
        kw = dict(bitmaps=bitmaps, masked=True, remap_area_min=0.5, skipna=skipna)
        y = record_order(grp.apply_host_grib(buf, rows, lev, ml, **kw))
        want = enc.encode(y)
        assert np.isnan(y).any() and np.isfinite(y).any()
        same_field(grp.apply_host_grib(buf, rows, lev, ml, grib_out=enc, chunk_outer=2, **kw), want, f"{name} skipna={skipna}")
        same_field(enc.encode(outside_result(g, field, lev, ml, True, 0.5, skipna)), want, f"{name} skipna={skipna} outside")


# ---------------------------------------------------------------- 4: a failed chunk drains

def test_a_failed_chunk_drains_and_the_next_calls_succeed(hip):
    c = chunk_case()
    grp, ml = c["g"]["grp"], c["g"]["masked_levels"]
    args = (c["buf"], c["rows"], c["lev"], ml)
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        with pytest.raises(_lib.SmmError, match="injected failure"):
            grp.apply_host_grib(*args, chunk_outer=2, grib_out=c["enc"], **c["kw"])
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    same_field(grp.apply_host_grib(*args, chunk_outer=2, grib_out=c["enc"], **c["kw"]), c["want"], "packed, after the failure")
    same_bits(record_order(grp.apply_host_grib(*args, chunk_outer=2, **c["kw"])), c["y"], "float, after the failure")


# ---------------------------------------------------------------- 5: the result ships raw again

def test_the_packed_result_ships_raw_again(hip):
    c = chunk_case()
    grp, ml = c["g"]["grp"], c["g"]["masked_levels"]
    got = grp.apply_host_grib(c["buf"], c["rows"], c["lev"], ml, grib_out=c["enc"], **c["kw"])
    rng = np.random.default_rng(6700)
    n_dst, nnz = 61, 500
    op = SparseOperator(D_STD, n_dst, rng.integers(1, D_STD + 1, nnz), rng.integers(1, n_dst + 1, nnz), rng.random(nnz))
    assert op.n_src == 288
    decoded = np.asarray(got).reshape(-1, D_STD)
    assert decoded.dtype == np.float32 and np.isnan(decoded).any() and np.isfinite(decoded).any()
    want = op.apply_host(decoded)
    again = op.apply_host_grib(np.asarray(got.buf), got.rows.ravel(), bitmaps=got.bitmaps.ravel())
    same_bits(again, want, "the packed level result, regridded raw")


# ---------------------------------------------------------------- the refusals that need the group's sizes

def test_refusals_that_need_the_group(hip):
    """out_bytes below the layout and a null out_host (the result side, first), then a level_index outside the group --
    SMM_ERR_INVALID each, and no byte of the result buffer is written."""
    c = chunk_case()
    grp, buf, enc = c["g"]["grp"], c["buf"], c["enc"]
    ml = np.ascontiguousarray(c["g"]["masked_levels"], dtype=np.uint8)
    rows, bitmaps = np.ascontiguousarray(c["rows"]).ravel(), np.ascontiguousarray(c["bitmaps"]).ravel()
    n = rows.size
    rec = enc.records(n)
    _, total = enc.layout(D_STD, n)
    out = np.full(total, 0xEE, np.uint8)
    rows_out, bms_out = np.zeros(n, GRIB_ROW_DTYPE), np.zeros(n, GRIB_BITMAP_DTYPE)
    lib = _lib.load()
    cast = lambda a, t: ctypes.cast(a.ctypes.data, ctypes.POINTER(t))      # noqa: E731

    def status(out_ptr=out.ctypes.data, out_bytes=total, lev=c["lev"], flags=_lib.APPLY_MASKED):
        lev = np.asarray(lev, np.int32)
        rc = lib.smm_group_apply_host_grib_pk(grp.handle, buf.ctypes.data, buf.size, cast(rows, _lib.GribRowStruct),
                                              cast(bitmaps, _lib.GribBitmapStruct), cast(rec, _lib.GribEncodeStruct), out_ptr,
                                              out_bytes, cast(rows_out, _lib.GribRowStruct), cast(bms_out, _lib.GribBitmapStruct),
                                              5, L, 2, lev.ctypes.data, ml.ctypes.data, 0.0, flags, 0)
        return rc, (lib.smm_last_error() or b"").decode()

    bad = c["lev"].copy()
    bad[2] = L
    rc, msg = status(out_bytes=total - 1, lev=bad, flags=1 << 20)          # the result side comes first
    assert rc == _lib.SMM_ERR_INVALID and "out_bytes" in msg and "below the layout" in msg, (rc, msg)
    rc, msg = status(out_ptr=None, lev=bad)
    assert rc == _lib.SMM_ERR_INVALID and "null result pointer" in msg, (rc, msg)
    rc, msg = status(lev=bad)
    assert rc == _lib.SMM_ERR_INVALID and "outside the group" in msg, (rc, msg)
    bad[2] = -1
    rc, msg = status(lev=bad, flags=_lib.APPLY_MASKED | _lib.APPLY_SKIPNA)
    assert rc == _lib.SMM_ERR_INVALID and "outside the group" in msg, (rc, msg)
    assert (out == 0xEE).all() and not rows_out.tobytes().strip(b"\0")
    rc, msg = status()
    assert rc == _lib.SMM_OK, (rc, msg)
    same_field(GribField(out, rows_out, c["want"].shape, D_STD, bitmaps=bms_out), c["want"], "the entry called directly")
    with pytest.raises(ValueError, match="transpose=False"):
        grp.apply_host_grib(buf, c["rows"], c["lev"], ml, transpose=False, grib_out=enc, **c["kw"])


# ---------------------------------------------------------------- 6: Regridder

LEVELS_PA = (100000, 70000, 40000)


def grib2_ocean(tmp_path, rng, n_steps=2):
    """(time, level, lat, lon) = (2, 3, 36, 72) on the std source grid: the top level without a bitmap, the others with
    the synthetic ocean masks of their depth and a few further cells cleared per step; widths 16 / 12 / 9 and decimal
    scales 0 / 1 / 2 by level."""
    grid = dict(template=0, ni=NX, nj=NY, la1=87.5, lo1=0.0, la2=-87.5, lo2=355.0, n_or_dj=5000000)
    masks = gridgen.synthetic_ocean_masks(NX, NY, len(LEVELS_PA), top=1.0, bottom=0.6)
    msgs = []
    for step in range(n_steps):
        fields = []
        for k, lev in enumerate(LEVELS_PA):
            f = dict(values=10.0 + 15 * rng.random((NY, NX)) - 3 * k, category=0, number=0, surface=(100, lev),
                     nbits=(16, 12, 9)[k], decimal=(0, 1, 2)[k], step=6 * step)
            if k > 0:
                f["bitmap"] = (np.asarray(masks[k]).reshape(NY, NX) != 0) & (rng.random((NY, NX)) > 0.02 * step)
            fields.append(f)
        msgs.append(encode2(fields, **grid))
    path = tmp_path / "ocean.grib2"
    path.write_bytes(b"".join(msgs))
    return str(path), "t"


@pytest.mark.parametrize("kw", [dict(), dict(skipna=True, packed_skipna=True)], ids=["plain", "skipna"])
def test_regridder_returns_a_masked_level_variable_grib_packed(hip, tmp_path, caplog, monkeypatch, kw):
    path, var = grib2_ocean(tmp_path, np.random.default_rng(80))
    mask_dim = "isobaricInhPa"
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    src = raw[var].data
    assert isinstance(src, GribField) and src.bitmaps is not None and src.shape == (2, 3, NY, NX)
    assert tuple(raw[var].dims[:2]) == ("time", mask_dim)
    w3 = CdoGenerate(dec[var], "r24x12").weights(method="con", mask_dim=mask_dim)
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))

    def group_host_calls():
        return [n for n in names if n.startswith("smm_group_apply_host")]

    base = dict(weights=w3, packed=True, packed_levels=True, loglevel="INFO", **kw)
    y = Regridder(**base).regrid(raw[var])
    assert y.values.dtype == np.float64 and y.values.shape == (2, 3, 12, 24)
    assert np.isnan(y.values).any() and np.isfinite(y.values).any()
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(grib_out=True, grib_out_levels=True, **base).regrid(raw[var])
    assert not grib_out_lines(caplog) and not any("decoded on the host" in r.getMessage() for r in caplog.records)
    assert group_host_calls() == ["smm_group_apply_host_grib_pk"]          # one call for the variable
    f = got.data
    assert isinstance(f, GribField) and f.shape == y.values.shape and got.dims == y.dims        # (time, level, lat, lon)
    want = GribEncode.from_field(src).encode(np.asarray(y.values).reshape(src.rows.size, -1))
    same_field(GribField(f.buf, f.rows, want.shape, f.n_points, bitmaps=f.bitmaps), want, f"regridder {kw}")
    assert (f.rows["ddiv"] == src.rows["ddiv"]).all() and f.rows["nbits"].max() == src.rows["nbits"].max()
    assert list(got.coords) == list(y.coords) and got.attrs == y.attrs
    decoded = np.asarray(got.values)
    assert decoded.dtype == np.float32 and np.array_equal(decoded, want.decode().reshape(f.shape), equal_nan=True)
    # grib_out alone keeps today's behaviour on masked-level weights: float64 and the one INFO line
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        plain = Regridder(grib_out=True, **base).regrid(raw[var])
    lines = grib_out_lines(caplog)
    assert len(lines) == 1 and "masked levels" in lines[0] and "comes back as without it" in lines[0], lines
    assert group_host_calls() == ["smm_group_apply_host_grib" + ("_na" if kw else "")]
    assert not isinstance(plain.data, GribField) and plain.values.dtype == np.float64
    same_bits(np.asarray(plain.values), np.asarray(y.values), "grib_out without grib_out_levels")
    if kw:
        # under skipna without packed_skipna the variable is decoded on the host: float64 and one INFO line, as before
        caplog.clear()
        with caplog.at_level("INFO"):
            out = Regridder(weights=w3, packed=True, packed_levels=True, grib_out=True, grib_out_levels=True, skipna=True,
                            loglevel="INFO").regrid(raw[var])
        lines = grib_out_lines(caplog)
        assert len(lines) == 1 and "decoded on the host" in lines[0] and out.values.dtype == np.float64
    else:
        # a float variable: one INFO line, the float64 result
        caplog.clear()
        with caplog.at_level("INFO"):
            out = Regridder(grib_out=True, grib_out_levels=True, **base).regrid(dec[var])
        lines = grib_out_lines(caplog)
        assert len(lines) == 1 and "not a raw GRIB variable" in lines[0] and out.values.dtype == np.float64
