"""Raw GRIB fields under skipna (smm_apply_grib_na, smm_apply_host_grib_na, smm_group_apply_grib_na,
smm_group_apply_host_grib_na, `skipna=True` of the four Python methods, `Regridder(packed=True, skipna=True,
packed_skipna=True)`): every result is compared bit for bit -- uint64 views -- with this library's SKIPNA float path on
the float32 field a host decode gives (SMM_APPLY_SKIPNA | SMM_APPLY_KERNEL_SELL, NaN where the bitmap is 0, +inf where
a rule overflows float32), which the 2-D cases tie to the rule restated in tests/helpers.py first.  Before a case
touches the GPU it shows on the CPU that its field meets every branch of the rule (`coverage`)."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, CdoGenerate, DeviceArray, GribField, Regridder, _lib,
                           pinned_empty, to_device)
from smmregrid_amd.io import open_dataset
from tests import far_cases as fc
from tests import grib_cases
from tests.helpers import bits_equal, skipna_ref
from tests.test_gpu_far_offsets import AREA_MIN, F32, F64, U8, far, grib_case, reference, sell_operator  # noqa: F401
from tests.test_gpu_grib import device_bytes, operator, same_arrays, same_bits
from tests.test_gpu_grib_bitmap import build_bm, grib1_sst, grib2_sst, random_bitmaps
from tests.test_gpu_grib_levels import D_STD, grib1_levels, grib2_levels, level_case
from tests.test_gpu_packed_levels import S as S_STD, geometry

pytestmark = pytest.mark.gpu
SELL, MASKED = _lib.APPLY_KERNEL_SELL, _lib.APPLY_MASKED
OPERATORS = ["bil_r180x90_r90x45", "ragged_random", "tiny"]
EPILOGUES = ((False, 0.0), (True, 0.5), (False, 1.0))
SITUATIONS = ("no invalid link", "some invalid links, den > 0", "every link invalid", "dead at area_min 0.5 by r alone")
# The threshold of the fourth situation.  0.5 everywhere but on the bilinear golden: between its aligned grids every
# destination row has two links of weight 0.5 and two of weight 0 and dst_frac is 1.0 throughout, so r is 0, 0.5 or 1 and
# frac_d * r never falls below 0.5 while r > 0, whatever the field.  There the area test can drop a row through r only at
# a threshold above 0.5: the 1.0 that EPILOGUES runs.
BY_R_AT = {"bil_r180x90_r90x45": 1.0}


# ---------------------------------------------------------------- what a field exercises (no device needed)

def coverage(csr, field, imask, frac, by_r_at=0.5):
    """Which branches of the SMM_APPLY_SKIPNA rule the (batch row, destination row) pairs with at least one link take,
    from the links, the decoded field and the restated rule alone: a pair without an invalid link, one with some and
    den > 0, one whose every link is invalid, and one that the rule keeps at remap_area_min = 0 and drops at 0.5
    (by_r_at) although dst_frac[d] alone passes it -- it is r that brings it down."""
    rowptr, col, val = (np.asarray(a) for a in csr)
    x = np.asarray(field).astype(np.float64)
    bad = ~np.isfinite(x[:, col]) & (val != 0.0)[None, :]

    def per_row(a):
        c = np.concatenate([np.zeros((a.shape[0], 1)), np.cumsum(a, axis=1)], axis=1)
        return c[:, rowptr[1:]] - c[:, rowptr[:-1]]

    n_bad = per_row(bad.astype(np.float64))
    den = per_row(np.where(bad, 0.0, np.broadcast_to(val, bad.shape)))
    linked = (np.diff(rowptr) > 0)[None, :]
    y0 = skipna_ref(csr, field, False, imask, frac, 0.0)
    y5 = skipna_ref(csr, field, False, imask, frac, by_r_at)
    by_r = ~np.isnan(y0) & np.isnan(y5) & (np.asarray(frac) >= by_r_at)[None, :] & (n_bad > 0)
    return np.array([(linked & (n_bad == 0)).any(), (linked & (n_bad > 0) & (den > 0.0)).any(),
                     (linked & (n_bad > 0) & ~(den > 0.0)).any(), by_r.any()])


def assert_covered(seen, what):
    assert seen.all(), f"{what}: the field never meets {[s for s, ok in zip(SITUATIONS, seen) if not ok]}"


def bitmapped_call(rng, S, n_batch, widths, D):
    """n_batch rows, every row with its own bitmap at a density of 0.05 .. 0.95 and byte residues 0 .. 3 for data and
    bitmaps; from five rows on also a row with an all-zero bitmap, a row without one and a row on its neighbour's."""
    specs = grib_cases.row_specs(rng, S, n_batch, widths, D=D)
    random_bitmaps(rng, specs, S, residues=(n_batch % 4, 1, 2, 3, 0))
    if n_batch >= 5:
        specs[1]["bitmap"] = np.zeros(S, bool)
        specs[2]["bitmap"] = None
        specs[4]["bitmap"] = ("row", 3)
    return build_bm(specs, rng, tail_residue=1 + n_batch % 3)


def overflow_call(rng, S, n_batch, D):
    """No bitmap anywhere: finite rows, and rows whose rule leaves float32 -- E = 127 on ref = 250, so q = 0 decodes to
    250 and q >= 2 to +inf -- with q drawn from {0, 2, 3}: their destination rows mix valid and invalid links."""
    specs = grib_cases.row_specs(rng, S, n_batch, (16, 12, 7, 25), D=D)
    for b in range(0, n_batch, 3):
        q = rng.choice(np.array([0, 2, 3], np.uint64), size=S, p=(0.5, 0.25, 0.25))
        specs[b].update(q=q, nbits=2, E=127, ref=250.0, D=0)
    buf, rows, field = grib_cases.build(specs, rng, tail_residue=1 + n_batch % 3)
    assert np.isposinf(field[0]).any() and (field[0][np.isfinite(field[0])] == 250.0).all() and not np.isnan(field).any()
    return buf, rows, field


# ---------------------------------------------------------------- the expectation and the calls

def expected_na(name, field, masked, area_min):
    """smm_apply with SMM_F32 X, SMM_APPLY_SKIPNA and the SELL kernel on the host-decoded field, tied to the restated
    rule first"""
    op, csr, imask, frac = operator(name)
    want = op.apply(to_device(field), masked=masked, remap_area_min=area_min, flags=SELL, skipna=True).to_host()
    bits_equal(want, skipna_ref(csr, field, masked, imask, frac, area_min))
    return want


def run_na(name, buf, rows, bitmaps, masked=False, area_min=0.0, **kw):
    op = operator(name)[0]
    return op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, masked=masked, remap_area_min=area_min, bitmaps=bitmaps,
                         skipna=True, **kw).to_host()


def check_epilogues(name, buf, rows, bitmaps, field, what):
    for masked, area_min in EPILOGUES:
        same_bits(run_na(name, buf, rows, bitmaps, masked, area_min), expected_na(name, field, masked, area_min),
                  f"{what} masked={masked} area_min={area_min}")


# ---------------------------------------------------------------- 1: bitmapped rows

WIDTH_SETS = [(0,), (12,), (16,), (32,), (16, 0, 12, 32, 1, 25, 7)]


def bitmapped_calls(name, widths, csr, imask, frac, S):
    """The three calls of one case -- B = 1, 5, 9: the tails of the 4 rows a thread holds -- with what they must contain
    shown before anything runs."""
    rng = np.random.default_rng(4000 + 7 * len(widths) + widths[0])
    calls, bm_residues, data_residues = [], set(), set()
    seen = np.zeros(4, bool)
    for n_batch in (1, 5, 9):
        D = (0,) if n_batch == 1 else (0, 2, -1)               # all ddiv == 1: DIV = false; else DIV = true
        buf, rows, bitmaps, field = bitmapped_call(rng, S, n_batch, widths, D)
        assert np.isnan(field).any() and np.isfinite(field).any() and buf.size % 4 != 0
        assert set(rows["ddiv"].tolist()) == ({1.0} if n_batch == 1 else {1.0, 100.0, 0.1})
        bm_residues |= set((bitmaps["bitmap_off"][bitmaps["bitmap_off"] != GRIB_NO_BITMAP] % 4).tolist())
        data_residues |= set((rows["byte_off"][(rows["nbits"] > 0) & (bitmaps["n_values"] > 0)] % 4).tolist())
        each = coverage(csr, field, imask, frac, BY_R_AT.get(name, 0.5))
        if n_batch >= 5:
            assert bitmaps["n_values"][1] == 0 and np.isnan(field[1]).all() and bitmaps["bitmap_off"][2] == GRIB_NO_BITMAP
            assert bitmaps["bitmap_off"][4] == bitmaps["bitmap_off"][3]
            assert_covered(each, f"{name} widths={widths} B={n_batch}")
        seen |= each
        calls.append((n_batch, buf, rows, bitmaps, field))
    assert_covered(seen, f"{name} widths={widths}")
    assert bm_residues == {0, 1, 2, 3} and (data_residues == {0, 1, 2, 3} or widths == (0,))
    return calls


@pytest.mark.parametrize("widths", WIDTH_SETS, ids=["0", "12", "16", "32", "mixed"])
@pytest.mark.parametrize("name", OPERATORS)
def test_bitmapped_rows_renormalise_as_apply_on_the_decoded_field(hip, name, widths):
    op, csr, imask, frac = operator(name)
    for n_batch, buf, rows, bitmaps, field in bitmapped_calls(name, widths, csr, imask, frac, op.n_src):
        check_epilogues(name, buf, rows, bitmaps, field, f"{name} widths={widths} B={n_batch}")


def test_four_rows_per_thread_without_the_division(hip):
    """all ddiv == 1 on five rows: the DIV = false instantiation at 4 rows per thread and its tail, which the B = 1 call
    of the test above runs at one row per thread only; and SMM_APPLY_SKIPNA passed in flags= beside the implied one."""
    name = "bil_r180x90_r90x45"
    csr, imask, frac = operator(name)[1:]
    rng = np.random.default_rng(4100)
    buf, rows, bitmaps, field = bitmapped_call(rng, operator(name)[0].n_src, 5, (16, 12, 25), (0,))
    assert (rows["ddiv"] == 1.0).all()
    assert_covered(coverage(csr, field, imask, frac, BY_R_AT[name]), "DIV = false")
    check_epilogues(name, buf, rows, bitmaps, field, "DIV = false")
    same_bits(run_na(name, buf, rows, bitmaps, True, 0.5, flags=_lib.APPLY_SKIPNA | SELL),
              expected_na(name, field, True, 0.5), "the bit passed as well")


# ---------------------------------------------------------------- 2: no bitmaps at all

@pytest.mark.parametrize("name", OPERATORS)
def test_rows_that_overflow_float32_without_any_bitmap(hip, name):
    """bitmaps=None: the BM = false, NA = true instantiations.  The invalid values are the +inf of a rule that leaves
    float32."""
    csr, imask, frac = operator(name)[1:]
    S = operator(name)[0].n_src
    rng = np.random.default_rng(4200)
    calls = [(n_batch,) + overflow_call(rng, S, n_batch, (0,) if n_batch == 1 else (0, 2, -1)) for n_batch in (1, 5, 9)]
    for n_batch, buf, rows, field in calls:
        assert_covered(coverage(csr, field, imask, frac, BY_R_AT.get(name, 0.5)), f"{name} overflow B={n_batch}")
    for n_batch, buf, rows, field in calls:
        check_epilogues(name, buf, rows, None, field, f"{name} overflow B={n_batch}")
    # records without one bitmap run the same gather
    n_batch, buf, rows, field = calls[1]
    none = np.zeros(n_batch, GRIB_BITMAP_DTYPE)
    none["bitmap_off"], none["n_values"] = GRIB_NO_BITMAP, S
    same_bits(run_na(name, buf, rows, none, True, 0.5), run_na(name, buf, rows, None, True, 0.5), "records without a bitmap")


# ---------------------------------------------------------------- 3: plain where nothing is invalid

@pytest.mark.parametrize("name", OPERATORS)
def test_a_field_without_an_invalid_value_has_the_plain_bits(hip, name):
    op = operator(name)[0]
    S = op.n_src
    rng = np.random.default_rng(4300)
    specs = grib_cases.row_specs(rng, S, 6, (16, 12, 0, 25, 7), D=(0, 1))
    for b, s in enumerate(specs):
        s["bitmap"], s["bm_residue"] = np.ones(S, bool), b % 4
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=2)
    assert np.isfinite(field).all() and (bitmaps["bitmap_off"] != GRIB_NO_BITMAP).all()
    plain = op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, masked=True, remap_area_min=0.5, bitmaps=bitmaps).to_host()
    assert np.isfinite(plain).any()
    same_bits(run_na(name, buf, rows, bitmaps, True, 0.5), plain, f"{name}: nothing invalid")
    same_bits(plain, expected_na(name, field, True, 0.5), f"{name}: and both are the float path's")


# ---------------------------------------------------------------- 4: the host entry

_HOST = {}


def host_case():
    if not _HOST:
        name = "bil_r180x90_r90x45"
        op, csr, imask, frac = operator(name)
        rng = np.random.default_rng(4400)
        buf, rows, bitmaps, field = bitmapped_call(rng, op.n_src, 7, (16, 12, 0, 24, 17, 7, 32), (0, 1))
        assert_covered(coverage(csr, field, imask, frac, BY_R_AT[name]), "host case")
        want = run_na(name, buf, rows, bitmaps, True, 0.5)
        same_bits(want, expected_na(name, field, True, 0.5), "device entry")
        _HOST.update(op=op, buf=buf, rows=rows, bitmaps=bitmaps, want=want)
    return _HOST


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("chunk_rows", [0, 1, 2])
def test_apply_host_grib_na_has_the_bits_of_the_device_entry(hip, pinned, chunk_rows):
    c = host_case()
    op, buf, rows, bitmaps, want = c["op"], c["buf"], c["rows"], c["bitmaps"], c["want"]
    D = op.n_dst
    out = pinned_empty((7, D), np.float64) if pinned else np.empty((7, D))
    out[:] = -1.0
    _lib.host_stats(reset=True)
    got = op.apply_host_grib(buf, rows, out=out, masked=True, remap_area_min=0.5, chunk_rows=chunk_rows, bitmaps=bitmaps,
                             skipna=True)
    st = _lib.host_stats(reset=True)
    assert got is out and st["calls"] == 1 and st["chunks"] == {0: 1, 1: 7, 2: 4}[chunk_rows]
    same_bits(got, want, f"host entry pinned={pinned} chunk_rows={chunk_rows}")
    # the Python method takes a contiguous out= only, as for the twin: ldy > n_dst goes to the entry itself
    y = pinned_empty((7, D + 3), np.float64) if pinned else np.empty((7, D + 3))
    y[:] = -1.0
    _lib.call("smm_apply_host_grib_na", op.handle, buf.ctypes.data, buf.size,
              ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
              ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), y.ctypes.data, _lib.SMM_F64, D + 3, 7,
              0.5, MASKED, chunk_rows)
    same_bits(np.ascontiguousarray(y[:, :D]), want, "ldy > D")
    assert (y[:, D:] == -1.0).all()


def test_apply_host_grib_na_without_bitmaps(hip):
    name = "ragged_random"
    op = operator(name)[0]
    buf, rows, field = overflow_call(np.random.default_rng(4450), op.n_src, 5, (0, 1))
    want = expected_na(name, field, True, 0.5)
    for chunk_rows in (0, 2):
        got = op.apply_host_grib(buf, rows, masked=True, remap_area_min=0.5, chunk_rows=chunk_rows, skipna=True)
        same_bits(got, want, f"host entry, bitmaps=None, chunk_rows={chunk_rows}")


# ---------------------------------------------------------------- 5: groups

LEVELS = np.array([5, 2, 7, 0, 6], dtype=np.int32)              # a subset of the group in non-monotone order
SPARSE = 2                                                       # data level 2 (member 7): its bitmaps leave almost nothing


def group_case(n_outer, n_inner):
    """Rows of five data levels: a level's bitmaps are its source mask with a further 30 % of the cells cleared; data
    level 2 keeps 2 % of its mask, data level 3 (the last but one) has all-zero bitmaps, row (0, 0, 0) has no bitmap and
    two rows share one (level_case)."""
    g = geometry("std")
    rng = np.random.default_rng(4500 + 10 * n_outer + n_inner)
    masks = np.array(g["masks"]).copy()
    masks[LEVELS[SPARSE]] = (masks[LEVELS[SPARSE]] != 0) & (rng.random(S_STD) < 0.02)
    buf, rows, bitmaps, field = level_case(rng, masks, n_outer, LEVELS, n_inner, rate=0.3, tail_residue=1 + n_outer % 3)
    assert 0 < bitmaps["n_values"][:, SPARSE].max() < 0.03 * S_STD and (bitmaps["n_values"][:, len(LEVELS) - 2] == 0).all()
    seen = np.zeros(4, bool)
    for k, w in enumerate(LEVELS):
        x = np.ascontiguousarray(field[:, k]).reshape(-1, S_STD)
        seen |= coverage(g["csrs"][w], x, g["imask"][w], g["frac"][w])
    assert_covered(seen, f"group case {n_outer} x {n_inner}")
    return g, buf, rows, bitmaps, field


@pytest.mark.parametrize("n_inner", [1, 2])
def test_group_entries_renormalise_every_level(hip, n_inner):
    """5 and 10 rows per level (4 rows per thread with a tail; 8 with a tail), masked_levels switching members 1 and 5
    off -- data level 0 runs unmasked in a masked call -- both Y layouts, the device and the host entry, chunk_outer 1
    and default."""
    n_outer = 5
    g, buf, rows, bitmaps, field = group_case(n_outer, n_inner)
    grp, ml = g["grp"], g["masked_levels"]
    assert (grp.n_src, grp.n_dst) == (S_STD, D_STD) and ml[LEVELS].tolist() == [0, 1, 1, 1, 1]
    dx, x = to_device(field), device_bytes(buf)
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        for transpose in (True, False):
            kw = dict(masked=masked, remap_area_min=area_min, transpose=transpose)
            what = f"n_inner={n_inner} {kw}"
            want = grp.apply(dx, LEVELS, ml, flags=SELL, skipna=True, **kw).to_host()
            assert np.isnan(want).any() and np.isfinite(want).any()
            got = grp.apply_grib(x, rows, LEVELS, ml, bitmaps=bitmaps, x_bytes=buf.size, skipna=True, **kw).to_host()
            same_bits(got, want, what + " device entry")
            for chunk_outer in (1, 0):
                got = grp.apply_host_grib(buf, rows, LEVELS, ml, bitmaps=bitmaps, chunk_outer=chunk_outer, skipna=True, **kw)
                same_bits(got, want, what + f" host entry chunk_outer={chunk_outer}")
    # the float path per level against the restated rule, once
    for k, w in enumerate(LEVELS):
        ref = skipna_ref(g["csrs"][w], np.ascontiguousarray(field[:, k]).reshape(-1, S_STD), bool(ml[w]), g["imask"][w],
                         g["frac"][w], 0.5)
        bits_equal(np.ascontiguousarray(want[k]).reshape(-1, D_STD), ref)
    # without bitmaps (BM = false, GRP = true, NA = true): the rows' own +inf are the invalid values
    rng = np.random.default_rng(4600 + n_inner)
    pbuf, prows, none, pfield = level_case(rng, g["masks"], 2, LEVELS, n_inner, bitmapped=False)
    flat = prows.ravel()
    flat["ref"][::3], flat["bscale"][::3], flat["ddiv"][::3] = 250.0, 2.0 ** 127, 1.0
    pfield = grib_cases.decode_rows(pbuf, flat, S_STD).reshape(pfield.shape)
    assert none is None and np.isposinf(pfield).any() and np.isfinite(pfield).any()
    want = grp.apply(to_device(pfield), LEVELS, ml, flags=SELL, skipna=True, masked=True, remap_area_min=0.5).to_host()
    assert np.isfinite(want).any()
    got = grp.apply_grib(device_bytes(pbuf), prows, LEVELS, ml, x_bytes=pbuf.size, skipna=True, masked=True, remap_area_min=0.5)
    same_bits(got.to_host(), want, "group, no bitmaps, device entry")
    same_bits(grp.apply_host_grib(pbuf, prows, LEVELS, ml, skipna=True, masked=True, remap_area_min=0.5), want,
              "group, no bitmaps, host entry")


# ---------------------------------------------------------------- 6: the facade

def spy(monkeypatch):
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    return names


@pytest.mark.parametrize("make", [grib1_sst, grib2_sst])
def test_regridder_keeps_a_bitmapped_variable_raw_under_skipna(hip, tmp_path, caplog, monkeypatch, make):
    path, var, plain = make(tmp_path, np.random.default_rng(70))
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    assert isinstance(raw[var].data, GribField) and raw[var].data.bitmaps is not None and np.isnan(dec[var].values).any()
    # bilinear weights of the variable without a bitmap: no source mask, so the missing cells are invalid links.  r16x8
    # does not divide the 36 x 18 source grid, so a target cell has four links of weight > 0 (onto r12x6 it has one)
    w = CdoGenerate(dec[plain], "r16x8").weights(method="bil")
    poisoned = Regridder(weights=w).regrid(dec[var])
    names = spy(monkeypatch)
    for area_min in (0.0, 0.5):
        want = Regridder(weights=w, skipna=True, remap_area_min=area_min).regrid(dec[var])
        assert np.isfinite(want.values).any() and not np.array_equal(np.isnan(want.values), np.isnan(poisoned.values))
        for lazy in (False, True):
            del names[:]
            caplog.clear()
            with caplog.at_level("INFO"):
                got = Regridder(weights=w, packed=True, skipna=True, packed_skipna=True, remap_area_min=area_min, lazy=lazy,
                                loglevel="INFO").regrid(raw[var])
                assert names.count("smm_apply_host_grib_na") == (0 if lazy else 1)
                vals = np.asarray(got.values)
            assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
            assert names.count("smm_apply_host_grib_na") == 1 and "smm_apply_host" not in names
            assert not any(n in ("smm_apply_host_grib", "smm_apply_host_grib_bm") for n in names)
            same_bits(vals, want.values, f"packed_skipna area_min={area_min} lazy={lazy}")
            if not lazy:
                same_arrays(got, want, f"packed_skipna area_min={area_min}")
    # the variable without a bitmap beside it takes the same entry, with bitmaps = NULL
    del names[:]
    got = Regridder(weights=w, packed=True, skipna=True, packed_skipna=True).regrid(raw[plain])
    assert names.count("smm_apply_host_grib_na") == 1
    same_arrays(got, Regridder(weights=w, skipna=True).regrid(dec[plain]), "the plain variable")
    # without the switch nothing changes: the host decode and its one INFO line
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        fb = Regridder(weights=w, packed=True, skipna=True, loglevel="INFO").regrid(raw[var])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "skipna" in lines[0] and "smm_apply_host_grib_na" not in names
    same_arrays(fb, Regridder(weights=w, skipna=True).regrid(dec[var]), "packed_skipna off")
    # a float32 result keeps its fallback with the switch on
    caplog.clear()
    with caplog.at_level("INFO"):
        Regridder(weights=w, packed=True, skipna=True, packed_skipna=True, out_dtype=np.float32, loglevel="INFO").regrid(raw[var])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "out_dtype float32" in lines[0]


@pytest.mark.parametrize("make", [grib2_levels, grib1_levels])
def test_regridder_keeps_a_masked_level_variable_raw_under_skipna(hip, tmp_path, caplog, monkeypatch, make):
    path, var, plain = make(tmp_path, np.random.default_rng(72), True)
    mask_dim = "isobaricInhPa"
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    assert isinstance(raw[var].data, GribField) and raw[var].data.bitmaps is not None
    # the weights' masks follow the first time step; the second step's bitmaps differ: invalid links
    w3 = CdoGenerate(dec[var], "r12x6").weights(method="con", mask_dim=mask_dim)
    v = dec[var].values
    assert (np.isnan(v[0]) != np.isnan(v[1])).any()
    names = spy(monkeypatch)

    def group_host_calls():
        return [n for n in names if n.startswith("smm_group_apply_host")]

    for transpose, area_min in ((True, 0.0), (False, 0.5)):
        kw = dict(weights=w3, skipna=True, transpose=transpose, remap_area_min=area_min)
        want = Regridder(**kw).regrid(dec[var])
        plain_sum = Regridder(weights=w3, transpose=transpose, remap_area_min=area_min).regrid(dec[var])
        assert np.isfinite(want.values).any() and not np.array_equal(np.isnan(want.values), np.isnan(plain_sum.values))
        for lazy in (False, True):
            del names[:]
            caplog.clear()
            with caplog.at_level("INFO"):
                got = Regridder(packed=True, packed_levels=True, packed_skipna=True, lazy=lazy, loglevel="INFO", **kw).regrid(raw[var])
                assert group_host_calls() == ([] if lazy else ["smm_group_apply_host_grib_na"])
                vals = np.asarray(got.values)
            assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
            assert group_host_calls() == ["smm_group_apply_host_grib_na"]
            same_bits(vals, want.values, f"packed_skipna levels transpose={transpose} lazy={lazy}")
    # masked levels without packed_levels keep their fallback
    caplog.clear()
    del names[:]
    with caplog.at_level("INFO"):
        Regridder(weights=w3, packed=True, skipna=True, packed_skipna=True, loglevel="INFO").regrid(raw[var])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "masked levels" in lines[0] and group_host_calls() == ["smm_group_apply_host"]


# ---------------------------------------------------------------- 7: far offsets

def test_apply_grib_na_past_2_32_bytes(far):       # noqa: F811
    """The GRIB case of tests/test_gpu_far_offsets.py at its size: streams and bitmaps at byte offsets past 2^32 and 2^34
    in one buffer, through smm_apply_grib_na."""
    op, csr, imask, frac = sell_operator()
    x_bytes, pieces, rows, bitmaps, fld = grib_case()
    assert int(rows["byte_off"].max()) > 1 << 32 and np.isnan(fld).any()
    xa = far.alloc((x_bytes + 3) // 4, F32).fill_random(seed=9, mean=1000.0, sigma=50.0)          # decoy bytes everywhere
    for off, data in pieces:
        DeviceArray((len(data),), U8, ptr=xa.ptr + off, base=xa).copy_from_host(np.frombuffer(data, U8))
    n = len(rows)
    ref = reference(csr, fld, imask, frac, skipna=True)
    lx, ly = fc.near_layout(n, op.n_src), fc.near_layout(n, op.n_dst)
    Xd, Yd = far.x(lx, F32, fld), far.y(ly, F64)
    _lib.call("smm_apply", op.handle, Xd.ptr, _lib.SMM_F32, op.n_src, Yd.ptr, _lib.SMM_F64, op.n_dst, n, AREA_MIN,
              SELL | MASKED | _lib.APPLY_SKIPNA, None)
    want = Yd.rows()
    fc.check_rows(want, ref, "smm_apply SKIPNA on the decoded field")
    Y = far.y(ly, F64)
    _lib.call("smm_apply_grib_na", op.handle, ctypes.c_void_p(xa.ptr), x_bytes,
              ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
              ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), Y.ptr, _lib.SMM_F64, op.n_dst, n,
              AREA_MIN, MASKED, None)
    got = Y.rows()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:3]
