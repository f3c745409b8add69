"""Raw GRIB fields, bitmapped or not, on masked-level (3-D) weights: `smm_group_apply_grib`, `smm_group_apply_host_grib`,
`OperatorGroup.apply_grib` / `apply_host_grib` and `Regridder(packed=True, packed_levels=True)`.  The expectation
everywhere is this library's float path -- `OperatorGroup.apply` / `apply_host` on the float32 field the reference
decoder of tests/grib_cases.py gives, NaN where the bitmap bit is 0 -- compared as raw bits; at least one case per test
is also taken per level from the CPU oracle.  Geometry: the "std" one of tests/test_gpu_packed_levels.py (r72x36 ->
r24x12 conservative on 8 synthetic ocean levels, S = 2592, D = 288: two destination blocks, the second with one slice of
32 live lanes).  A level's bitmaps are its source mask with a further 3 % of the cells cleared."""
import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, CdoGenerate, DataArray, Dataset, GribField, OperatorGroup, Regridder,
                           SparseOperator, _lib, pinned_empty, to_device)
from smmregrid_amd import road
from smmregrid_amd.gridtype import GridType
from smmregrid_amd.io import open_dataset
from tests import grib_cases
from tests.test_gpu_grib import device_bytes, same_arrays
from tests.test_gpu_grib_bitmap import build_bm
from tests.test_gpu_packed_levels import EPILOGUES, L, LEVEL_SETS, S, bits_equal, geometry, nan_share_ok
from tests.test_griblite import encode, encode2

pytestmark = pytest.mark.gpu
WIDTHS = (0, 1, 12, 16, 25, 32)
D_STD = 288


# ---------------------------------------------------------------- fields (no device needed)

def level_case(rng, masks, n_outer, lev, n_inner, D=(0, 2, -1), edges=True, bitmapped=True, rate=0.03, tail_residue=1):
    """One call's buffer: n_outer x len(lev) x n_inner rows in record order (o, l, i), the six widths cycled over them,
    per-row ref / E / byte residue, D cycled from `D`, pieces shuffled in the buffer.  A row's bitmap is the source mask
    of its level with a further `rate` of the cells cleared (bitmapped=False: no row has one).  edges: row (0, 0, 0) has
    no bitmap; the last row of level 0 names the bitmap of level 0's second row -- or, when level 0 has one row, level
    1's row names level 0's -- and every row of the last-but-one level has an all-zero bitmap, no value, and its data "at"
    the very end of the buffer.  Returns buf, rows and bitmaps shaped (n_outer, n_lev, n_inner), and the float32 field
    (n_outer, n_lev, n_inner, S) decoded from the buffer by the reference decoder, NaN where the bitmap bit is 0."""
    dims = (n_outer, len(lev), n_inner)
    n_rows = int(np.prod(dims))
    specs = grib_cases.row_specs(rng, S, n_rows, WIDTHS, D=D)
    at = lambda o, l, i: int(np.ravel_multi_index((o, l, i), dims))      # noqa: E731
    empty = []
    for b, s in enumerate(specs):
        l = np.unravel_index(b, dims)[1]
        s["bitmap"] = ((masks[lev[l]] != 0) & (rng.random(S) >= rate)) if bitmapped else None
        s["bm_residue"] = (b + 1) % 4
    if edges and bitmapped:
        specs[at(0, 0, 0)]["bitmap"] = None
        level0 = [at(o, 0, i) for o in range(n_outer) for i in range(n_inner)]
        if len(level0) >= 3:
            specs[level0[-1]]["bitmap"] = ("row", level0[1])
        else:
            specs[at(0, 1, 0)]["bitmap"] = ("row", level0[-1] if len(level0) > 1 else at(0, 2, 0))
        empty = [at(o, dims[1] - 2, i) for o in range(n_outer) for i in range(n_inner)]
        for b in empty:
            specs[b]["bitmap"] = np.zeros(S, bool)
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=tail_residue)
    rows["byte_off"][empty] = buf.size
    assert (bitmaps["n_values"][empty] == 0).all()
    # the reference decoder on the buffer: each row's stream holds its present cells only
    decoded = np.full((n_rows, S), np.float32(np.nan))
    for b in range(n_rows):
        m = np.ones(S, bool)
        if bitmaps["bitmap_off"][b] != GRIB_NO_BITMAP:
            off = int(bitmaps["bitmap_off"][b])
            m = np.unpackbits(buf[off:off + (S + 7) // 8])[:S].astype(bool)
        assert int(m.sum()) == int(bitmaps["n_values"][b])
        decoded[b, m] = grib_cases.decode_rows(buf, rows[b:b + 1], int(m.sum()))[0]
    assert np.array_equal(decoded.view(np.uint32), field.view(np.uint32))
    return buf, rows.reshape(dims), (bitmaps.reshape(dims) if bitmapped else None), decoded.reshape(dims + (S,))


def oracle_levels(g, field, lev, masked, area_min, transpose, masked_levels=None, fill=True):
    """Per level oracle.apply_c on (n_outer, n_lev, n_inner, S); the level's mask applies when the call is masked and
    masked_levels leaves it on."""
    outs = []
    for k, w in enumerate(lev):
        use = masked and (masked_levels is None or bool(masked_levels[w]))
        x = np.ascontiguousarray(field[:, k]).reshape(-1, S)
        y = oracle.apply_c(g["csrs"][w], x, masked=use, dst_imask=g["imask"][w], dst_frac=g["frac"][w], area_min=area_min,
                           fill=fill)
        outs.append(y.reshape(field.shape[0], field.shape[2], -1))
    out = np.stack(outs, axis=0)                                          # (n_lev, n_outer, n_inner, D)
    return np.ascontiguousarray(np.moveaxis(out, 0, -2)) if transpose else out


def same_as_oracle(got, ref, what):
    assert np.array_equal(np.isnan(got), np.isnan(ref)), what
    assert np.array_equal(got[~np.isnan(ref)], ref[~np.isnan(ref)]), what


def without_level(y, k, transpose):
    """the expectation without data level k (the deliberately empty one)"""
    return np.delete(y, k, axis=-2 if transpose else 0)


def run_device(grp, buf, rows, bitmaps, lev, ml, **kw):
    return grp.apply_grib(device_bytes(buf), rows, lev, ml, bitmaps=bitmaps, x_bytes=buf.size, **kw).to_host()


# ---------------------------------------------------------------- 1: the device entry

@pytest.mark.parametrize("n_inner", [1, 2])
@pytest.mark.parametrize("n_outer", [1, 2, 3, 5, 9])
def test_group_apply_grib_has_the_bits_of_the_decoded_field(hip, n_outer, n_inner):
    """Every batch tile size and its tail (1 .. 18 rows per level), the six widths mixed in one call, rows shuffled at all
    byte residues, one row without a bitmap, two rows on one bitmap_off, one whole level without a value, every epilogue
    with masked_levels switching levels 1 and 5 off, both Y layouts; mixed ddiv and all ddiv == 1."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    assert (grp.n_src, grp.n_dst) == (S, D_STD) and ml.tolist() == [1, 0, 1, 1, 1, 0, 1, 1]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(3000 + 10 * n_outer + n_inner)
    buf, rows, bitmaps, field = level_case(rng, g["masks"], n_outer, lev, n_inner, tail_residue=1 + n_outer % 3)
    flat_r, flat_b = rows.ravel(), bitmaps.ravel()
    assert set(flat_r["nbits"].tolist()) == set(WIDTHS) and len(set((flat_r["byte_off"] % 4).tolist())) == 4
    assert set(flat_r["ddiv"].tolist()) == {1.0, 100.0, 0.1} and (np.diff(flat_r["byte_off"].astype(np.int64)) < 0).any()
    assert (flat_b["bitmap_off"] == GRIB_NO_BITMAP).sum() == 1 and buf.size % 4 != 0
    shared = flat_b["bitmap_off"][flat_b["bitmap_off"] != GRIB_NO_BITMAP]
    assert len(set(shared.tolist())) == shared.size - 1
    assert (bitmaps["n_values"][:, L - 2] == 0).all() and (rows["byte_off"][:, L - 2] == buf.size).all()
    dx = to_device(field)
    for masked, area_min in EPILOGUES:
        for transpose in (True, False):
            kw = dict(masked=masked, remap_area_min=area_min, transpose=transpose)
            what = f"n_outer={n_outer} n_inner={n_inner} {kw}"
            want = grp.apply(dx, lev, ml, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host()
            nan_share_ok(without_level(want, L - 2, transpose), what)
            assert np.isnan(want[..., L - 2, :] if transpose else want[L - 2]).any()
            bits_equal(run_device(grp, buf, rows, bitmaps, lev, ml, **kw), want, what)
    same_as_oracle(want, oracle_levels(g, field, lev, True, 0.5, False, ml), "float path vs oracle")
    # masked_levels = NULL: every level masks; rows given flat
    want = grp.apply(dx, lev, None, masked=True).to_host()
    bits_equal(run_device(grp, buf, rows.ravel(), bitmaps.ravel(), lev, None, masked=True, n_inner=n_inner), want,
               "masked_levels=None, flat records")
    same_as_oracle(want, oracle_levels(g, field, lev, True, 0.0, True), "masked_levels=None vs oracle")
    # all ddiv == 1.0: the instantiation without the division, on a call without edge rows
    buf1, rows1, bitmaps1, field1 = level_case(rng, g["masks"], n_outer, lev, n_inner, D=(0,), edges=False)
    assert (rows1["ddiv"] == 1.0).all() and (bitmaps1["bitmap_off"] != GRIB_NO_BITMAP).all()
    want = grp.apply(to_device(field1), lev, ml, masked=True, remap_area_min=0.5).to_host()
    nan_share_ok(want, f"n_outer={n_outer} n_inner={n_inner} ddiv == 1")
    bits_equal(run_device(grp, buf1, rows1, bitmaps1, lev, ml, masked=True, remap_area_min=0.5), want, "ddiv == 1")


@pytest.mark.parametrize("n_outer,n_inner", [(9, 1), (5, 2), (2, 9)])
def test_eight_rows_per_thread_and_their_tail(hip, n_outer, n_inner):
    """SMM_TUNE_SELL_BATCH_ROWS = 8: the BT = 8 instantiations, with and without bitmaps, 9 / 10 / 18 rows per level."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(3100 + n_outer)
    for bitmapped in (True, False):
        buf, rows, bitmaps, field = level_case(rng, g["masks"], n_outer, lev, n_inner, bitmapped=bitmapped)
        kw = dict(masked=True, remap_area_min=0.5, transpose=n_inner == 1)
        want = grp.apply(to_device(field), lev, ml, **kw).to_host()
        if bitmapped:
            nan_share_ok(without_level(want, L - 2, kw["transpose"]), f"BT=8 {n_outer}x{n_inner}")
            same_as_oracle(want, oracle_levels(g, field, lev, True, 0.5, kw["transpose"], ml), "BT=8 vs oracle")
        with _lib.tuning(sell_batch_rows=8):
            got = run_device(grp, buf, rows, bitmaps, lev, ml, **kw)
        bits_equal(got, want, f"BT=8 {n_outer}x{n_inner} bitmapped={bitmapped}")


def test_no_fill_on_a_call_without_missing_cells(hip):
    """SMM_APPLY_NO_FILL: no bitmap records at all (the instantiations without the rank lookup), and records that are
    all SMM_GRIB_NO_BITMAP or all-present bitmaps."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(3200)
    buf, rows, none, field = level_case(rng, g["masks"], 5, lev, 2, bitmapped=False)
    assert none is None and np.isfinite(field).all()
    for masked, area_min in EPILOGUES:
        kw = dict(masked=masked, remap_area_min=area_min, flags=_lib.APPLY_NO_FILL)
        want = grp.apply(to_device(field), lev, ml, **kw).to_host()
        bits_equal(run_device(grp, buf, rows, None, lev, ml, **kw), want, f"NO_FILL {kw}")
        kw["flags"] = 0
        bits_equal(run_device(grp, buf, rows, None, lev, ml, **kw), want, f"fill on, nothing to fill {kw}")
    same_as_oracle(want, oracle_levels(g, field, lev, True, 0.5, True, ml, fill=False), "NO_FILL vs oracle")
    # the same through the instantiations with the rank lookup: records without a bitmap, and all-present bitmaps
    none = np.zeros(rows.shape, GRIB_BITMAP_DTYPE)
    none["bitmap_off"], none["n_values"] = GRIB_NO_BITMAP, S
    bits_equal(run_device(grp, buf, rows, none, lev, ml, masked=True, remap_area_min=0.5, flags=_lib.APPLY_NO_FILL), want,
               "NO_FILL, records without a bitmap")
    buf, rows, ones, field = level_case(rng, np.ones((L, S), np.int32), 3, lev, 1, edges=False, rate=-1.0)
    assert (ones["n_values"] == S).all() and (ones["bitmap_off"] != GRIB_NO_BITMAP).all() and np.isfinite(field).all()
    kw = dict(masked=True, remap_area_min=0.5, flags=_lib.APPLY_NO_FILL)
    bits_equal(run_device(grp, buf, rows, ones, lev, ml, **kw), grp.apply(to_device(field), lev, ml, **kw).to_host(),
               "NO_FILL, all-present bitmaps")


# ---------------------------------------------------------------- 2: level subsets, the grid limit

@pytest.mark.parametrize("name", ["subset", "reversed", "repeated"])
def test_level_subsets_and_repeats(hip, name):
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.asarray(LEVEL_SETS[name], dtype=np.int32)
    rng = np.random.default_rng(3300 + len(lev))
    buf, rows, bitmaps, field = level_case(rng, g["masks"], 9, lev, 2, edges=False)
    for transpose in (True, False):
        kw = dict(masked=True, remap_area_min=0.5, transpose=transpose)
        want = grp.apply(to_device(field), lev, ml, **kw).to_host()
        nan_share_ok(want, name)
        same_as_oracle(want, oracle_levels(g, field, lev, True, 0.5, transpose, ml), f"{name} vs oracle")
        bits_equal(run_device(grp, buf, rows, bitmaps, lev, ml, **kw), want, f"{name} device")
        bits_equal(grp.apply_host_grib(buf, rows, lev, ml, bitmaps=bitmaps, **kw), want, f"{name} host")


def test_a_small_grid_limit_cuts_the_outer_range_and_the_levels(hip):
    """5 x 8 x 2 rows need 2 destination blocks x 3 batch tiles x 8 levels = 48 workgroups.  A limit of 20 cuts the outer
    range, 5 and 2 leave single rows whose levels are cut as well (2: one level per launch); 1 is below the 2 destination
    blocks of one row of one level."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(3400)
    buf, rows, bitmaps, field = level_case(rng, g["masks"], 5, lev, 2)
    kw = dict(masked=True, remap_area_min=0.5, transpose=False)
    want = grp.apply(to_device(field), lev, ml, **kw).to_host()
    same_as_oracle(want, oracle_levels(g, field, lev, True, 0.5, False, ml), "grid limit vs oracle")
    bits_equal(run_device(grp, buf, rows, bitmaps, lev, ml, **kw), want, "no limit")
    try:
        for limit in (20, 5, 2):
            _lib.call("smm_debug_set_grid_limit", limit)
            bits_equal(run_device(grp, buf, rows, bitmaps, lev, ml, **kw), want, f"grid limit {limit}")
            bits_equal(grp.apply_host_grib(buf, rows, lev, ml, bitmaps=bitmaps, **kw), want, f"grid limit {limit}, host")
        _lib.call("smm_debug_set_grid_limit", 1)
        with pytest.raises(_lib.SmmError, match="launch grid beyond 1 workgroups") as err:
            run_device(grp, buf, rows, bitmaps, lev, ml, **kw)
        assert err.value.code == _lib.SMM_ERR_INVALID
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    bits_equal(run_device(grp, buf, rows, bitmaps, lev, ml, **kw), want, "limit restored")


# ---------------------------------------------------------------- 3: the host entry

def staged_bytes(rows, bitmaps):
    """40 + (bitmaps ? 16 : 0) + align4(data) + (bitmapped ? align4(ceil(n_src / 8)) : 0), summed over the rows"""
    total = 0
    for b, r in enumerate(rows.ravel()):
        has = bitmaps is not None and int(bitmaps.ravel()[b]["bitmap_off"]) != GRIB_NO_BITMAP
        n = int(bitmaps.ravel()[b]["n_values"]) if has else S
        total += 40 + (16 if bitmaps is not None else 0) + ((n * int(r["nbits"]) + 7) // 8 + 3) // 4 * 4
        total += ((S + 7) // 8 + 3) // 4 * 4 if has else 0
    return total


_HOST = {}


def host_case():
    """5 x 8 x 2 rows with every edge row; the device entry's bits for both layouts, tied to the float path and to the
    oracle once."""
    if not _HOST:
        g = geometry("std")
        grp, ml = g["grp"], g["masked_levels"]
        lev = np.arange(L, dtype=np.int32)
        buf, rows, bitmaps, field = level_case(np.random.default_rng(3500), g["masks"], 5, lev, 2, tail_residue=3)
        want = {}
        for transpose in (True, False):
            kw = dict(masked=True, remap_area_min=0.5, transpose=transpose)
            want[transpose] = run_device(grp, buf, rows, bitmaps, lev, ml, **kw)
            bits_equal(want[transpose], grp.apply_host(field, lev, ml, **kw), "device entry vs apply_host")
            same_as_oracle(want[transpose], oracle_levels(g, field, lev, True, 0.5, transpose, ml), "host case vs oracle")
            nan_share_ok(without_level(want[transpose], L - 2, transpose), "host case")
        _HOST.update(g=g, lev=lev, buf=buf, rows=rows, bitmaps=bitmaps, field=field, want=want)
    return _HOST


@pytest.mark.parametrize("chunk_outer", [0, 1, 2])
@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("pinned", [False, True])
def test_apply_host_grib_has_the_bits_of_the_device_entry(hip, pinned, transpose, chunk_outer):
    c = host_case()
    grp, ml, buf, rows, bitmaps = c["g"]["grp"], c["g"]["masked_levels"], c["buf"], c["rows"], c["bitmaps"]
    shape = (5, 2, L, D_STD) if transpose else (L, 5, 2, D_STD)
    x_host, out = buf, np.full(shape, -1.0)
    if pinned:
        x_host, out = pinned_empty(buf.size, np.uint8), pinned_empty(shape, np.float64)
        x_host[:], out[:] = buf, -1.0
    _lib.host_stats(reset=True)
    got = grp.apply_host_grib(x_host, rows, c["lev"], ml, bitmaps=bitmaps, out=out, masked=True, remap_area_min=0.5,
                              transpose=transpose, chunk_outer=chunk_outer)
    st = _lib.host_stats(reset=True)
    assert got is out
    bits_equal(got, c["want"][transpose], f"host entry pinned={pinned} transpose={transpose} chunk_outer={chunk_outer}")
    assert st["calls"] == 1 and st["chunks"] == {0: 1, 1: 5, 2: 3}[chunk_outer]
    assert st["h2d_bytes"] == staged_bytes(rows, bitmaps) and st["d2h_bytes"] == rows.size * D_STD * 8
    if chunk_outer == 2:                                       # without bitmap records: 16 B less per row
        pbuf, prows, none, pfield = level_case(np.random.default_rng(3501), c["g"]["masks"], 5, c["lev"], 2, bitmapped=False)
        _lib.host_stats(reset=True)
        got = grp.apply_host_grib(pbuf, prows, c["lev"], ml, masked=True, transpose=transpose, chunk_outer=2)
        assert none is None and _lib.host_stats(reset=True)["h2d_bytes"] == staged_bytes(prows, None)
        bits_equal(got, grp.apply_host(pfield, c["lev"], ml, masked=True, transpose=transpose), "no bitmap records")


def test_a_failed_chunk_drains_and_the_next_call_succeeds(hip):
    c = host_case()
    grp, ml = c["g"]["grp"], c["g"]["masked_levels"]
    kw = dict(bitmaps=c["bitmaps"], masked=True, remap_area_min=0.5, chunk_outer=2)
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        with pytest.raises(_lib.SmmError, match="injected failure"):
            grp.apply_host_grib(c["buf"], c["rows"], c["lev"], ml, **kw)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    bits_equal(grp.apply_host_grib(c["buf"], c["rows"], c["lev"], ml, **kw), c["want"][True], "after the injected failure")


def test_a_member_operator_keeps_its_bits_between_group_calls(hip):
    """smm_apply_host_grib_bm on member 3 -- the rows of data level 3 -- between two group calls: the group's tables and
    the operator's are buffers of their own."""
    c = host_case()
    g = c["g"]
    grp, ml, op = g["grp"], g["masked_levels"], g["ops"][3]
    rows3, bm3 = np.ascontiguousarray(c["rows"][:, 3]).ravel(), np.ascontiguousarray(c["bitmaps"][:, 3]).ravel()
    field3 = np.ascontiguousarray(c["field"][:, 3]).reshape(-1, S)
    want3 = op.apply_host(field3, masked=True, remap_area_min=0.5, flags=_lib.APPLY_KERNEL_SELL)
    kw = dict(bitmaps=c["bitmaps"], masked=True, remap_area_min=0.5)
    for _ in range(2):
        bits_equal(grp.apply_host_grib(c["buf"], c["rows"], c["lev"], ml, **kw), c["want"][True], "group call")
        bits_equal(op.apply_host_grib(c["buf"], rows3, masked=True, remap_area_min=0.5, bitmaps=bm3), want3, "member call")
        bits_equal(run_device(grp, c["buf"], c["rows"], c["bitmaps"], c["lev"], ml, masked=True, remap_area_min=0.5),
                   c["want"][True], "group device call")
    bits_equal(want3.reshape(5, 2, D_STD), np.ascontiguousarray(c["want"][True][:, :, 3]), "member 3 is data level 3")


def test_refusals_that_need_the_group(hip):
    c = host_case()
    g = c["g"]
    grp, buf, rows, bitmaps, lev = g["grp"], c["buf"], c["rows"], c["bitmaps"], c["lev"]
    x = device_bytes(buf)

    def refused(word, rows=rows, bitmaps=bitmaps, lev=lev, x_bytes=buf.size, group=grp, **kw):
        for call in (lambda: group.apply_grib(x, rows, lev, bitmaps=bitmaps, x_bytes=x_bytes, **kw),
                     lambda: group.apply_host_grib(buf[:x_bytes], rows, lev, bitmaps=bitmaps, **kw)):
            with pytest.raises(_lib.SmmError, match=word) as err:
                call()
            assert err.value.code == _lib.SMM_ERR_INVALID, word

    bad = lev.copy()
    bad[2] = L
    refused("outside the group", lev=bad)
    bad[2] = -1
    refused("outside the group", lev=bad)
    refused("leave the buffer", x_bytes=buf.size - 1)            # the piece laid last ends exactly at x_bytes
    many = bitmaps.copy()
    many["n_values"][1, 1, 0] = S + 1
    refused("n_values", bitmaps=many)
    # a used member without the epilogue vectors the call asks for; an unused one does not matter
    rowptr, col, val = g["csrs"][0]
    bare = SparseOperator.from_csr(S, D_STD, rowptr, col, val, device=0)
    mixed = OperatorGroup([g["ops"][0], bare])
    r2, b2 = np.ascontiguousarray(rows[:, :2]), np.ascontiguousarray(bitmaps[:, :2])
    ok = mixed.apply_host_grib(buf, r2, np.array([0, 0], np.int32), bitmaps=b2, masked=True, remap_area_min=0.5)
    bits_equal(np.ascontiguousarray(ok[:, :, 0]), np.ascontiguousarray(c["want"][True][:, :, 0]), "the unused member is bare")
    for kw, word in ((dict(masked=True), "dst_imask"), (dict(remap_area_min=0.5), "dst_frac")):
        refused(word, rows=r2, bitmaps=b2, lev=np.array([0, 1], np.int32), group=mixed, **kw)


# ---------------------------------------------------------------- 4: Regridder

NI, NJ = 36, 18


def grib2_levels(tmp_path, rng, bitmapped):
    """The file of test_regridder_masked_levels_decode_a_bitmapped_variable_on_the_host -- 2 levels x 2 steps, 36 x 18,
    bitmaps differing per level -- with a 2-D variable beside the 3-D one."""
    grid = dict(template=0, ni=NI, nj=NJ, la1=85.0, lo1=0.0, la2=-85.0, lo2=350.0, n_or_dj=10000000)
    msgs = []
    for step in (0, 6):
        fields = []
        for lev in (85000, 50000):
            f = dict(values=220.0 + 30 * rng.random((NJ, NI)) + lev / 1e4, category=0, number=0, surface=(100, lev), nbits=12,
                     decimal=1, step=step)
            if bitmapped:
                f["bitmap"] = rng.random((NJ, NI)) > (0.2 if lev == 85000 else 0.4)
            fields.append(f)
        msgs.append(encode2(fields, **grid))
        msgs.append(encode2([dict(values=280.0 + rng.standard_normal((NJ, NI)), category=0, number=0, surface=(103, 2),
                                  nbits=17, step=step)], **grid))
    path = tmp_path / "t.grib2"
    path.write_bytes(b"".join(msgs))
    return str(path), "t", "t2m"


def grib1_levels(tmp_path, rng, bitmapped):
    """The GRIB-1 twin built with `encode`: temperature on two pressure levels x 2 days with per-level bitmaps, 2 m
    temperature beside it."""
    grid = (0, NI, NJ, 85, 0, -85, 350, 10000)
    msgs = []
    for day in (1, 2):
        for lev in (850, 500):
            kw = dict(bitmap=rng.random((NJ, NI)) > (0.2 if lev == 850 else 0.4)) if bitmapped else {}
            msgs.append(encode(220.0 + 30 * rng.random((NJ, NI)) + lev / 100.0, *grid, param=130, level_type=100, level=lev,
                               date=(2021, 3, day, 12), nbits=12, **kw))
        msgs.append(encode(280.0 + rng.standard_normal((NJ, NI)), *grid, param=167, date=(2021, 3, day, 12), nbits=16))
    path = tmp_path / "t.grib"
    path.write_bytes(b"".join(msgs))
    return str(path), "t", "t2m"


@pytest.mark.parametrize("bitmapped", [True, False])
@pytest.mark.parametrize("make", [grib2_levels, grib1_levels])
def test_regridder_ships_a_masked_level_variable_raw(hip, tmp_path, caplog, monkeypatch, make, bitmapped):
    path, var, plain = make(tmp_path, np.random.default_rng(72), bitmapped)
    mask_dim = "isobaricInhPa"
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    f = raw[var].data
    assert isinstance(f, GribField) and (f.bitmaps is not None) == bitmapped and f.shape == (2, 2, NJ, NI)
    assert tuple(raw[var].dims[:2]) == ("time", mask_dim) and bool(np.isnan(dec[var].values).any()) == bitmapped
    assert isinstance(raw[plain].data, GribField) and raw[plain].data.shape == (2, NJ, NI)
    w3 = CdoGenerate(dec[var], "r12x6").weights(method="con", mask_dim=mask_dim)
    w2 = CdoGenerate(dec[plain], "r12x6").weights(method="con")
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))

    def group_host_calls():
        return [n for n in names if n.startswith("smm_group_apply_host")]

    for transpose in (True, False):
        want = Regridder(weights=w3, transpose=transpose).regrid(dec[var])
        assert want.dtype == np.float64 and np.isfinite(want.values).any()
        del names[:]
        caplog.clear()
        with caplog.at_level("INFO"):
            got = Regridder(weights=w3, packed=True, packed_levels=True, transpose=transpose, loglevel="INFO").regrid(raw[var])
        assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
        assert group_host_calls() == ["smm_group_apply_host_grib"]              # exactly one call for the variable
        same_arrays(got, want, f"raw levels transpose={transpose}")
    want = Regridder(weights=w3).regrid(dec[var])
    # packed=True alone keeps the host decode and its INFO line
    caplog.clear()
    del names[:]
    with caplog.at_level("INFO"):
        host = Regridder(weights=w3, packed=True, loglevel="INFO").regrid(raw[var])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "masked levels" in lines[0] and group_host_calls() == ["smm_group_apply_host"]
    same_arrays(host, want, "packed=True alone")
    # lazy=True defers the call
    del names[:]
    lazy = Regridder(weights=w3, packed=True, packed_levels=True, lazy=True).regrid(raw[var])
    assert group_host_calls() == []
    vals = np.asarray(lazy.values)
    assert group_host_calls() == ["smm_group_apply_host_grib"]
    assert vals.dtype == np.float64 and np.array_equal(vals.view(np.uint64), want.values.view(np.uint64))
    # the fallbacks decode on the host with one INFO line each and give the bits of the decoded road
    for kw, word in ((dict(skipna=True), "skipna"), (dict(out_dtype=np.float32), "out_dtype float32")):
        caplog.clear()
        del names[:]
        with caplog.at_level("INFO"):
            fb = Regridder(weights=w3, packed=True, packed_levels=True, loglevel="INFO", **kw).regrid(raw[var])
        lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
        assert len(lines) == 1 and word in lines[0] and "smm_group_apply_host_grib" not in names, lines
        ref = Regridder(weights=w3, **kw).regrid(dec[var])
        assert fb.dtype == ref.dtype and np.array_equal(fb.values.view(np.uint8), ref.values.view(np.uint8)), word
    # a Dataset mixing a 2-D raw variable and the 3-D one: weights per gridtype, one raw call per variable
    ds_dec = Dataset({var: dec[var], plain: dec[plain]}, attrs=dec.attrs)
    ds_raw = Dataset({var: raw[var], plain: raw[plain]}, attrs=raw.attrs)
    grids = dict(source_grid=ds_dec, target_grid="r12x6", method="con", mask_dim=mask_dim)
    want_ds = Regridder(**grids).regrid(ds_dec)
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        got_ds = Regridder(packed=True, packed_levels=True, loglevel="INFO", **grids).regrid(ds_raw)
    assert not any("decoded on the host" in r.getMessage() for r in caplog.records)
    assert group_host_calls() == ["smm_group_apply_host_grib"] and names.count("smm_apply_host_grib") == 1
    assert not any(n in ("smm_apply_host", "smm_apply_host_grib_bm") for n in names)
    assert list(got_ds.data_vars) == list(want_ds.data_vars)
    for name in (var, plain):
        same_arrays(got_ds[name], want_ds[name], f"{name} of the mixed Dataset")


def test_a_gribfield_whose_fields_are_not_ordered_by_level_is_decoded(hip, tmp_path, caplog):
    """dims (lat, lon, level)-style declarations cannot be batch rows of the group entry: one INFO line with its own
    reason, the bits of the decoded road."""
    path, var, _ = grib2_levels(tmp_path, np.random.default_rng(73), True)
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    mask_dim = "isobaricInhPa"
    dims = tuple(raw[var].dims)
    gt = GridType(dims=dims, extra_dims={"mask": [mask_dim]})
    on = road.Switches.of(packed=True, packed_levels=True)

    def way(d):
        return road.decide(on, road.Facts(var, road.GRIB, np.float32, d, gt.horizontal_dims, mask_dim))
    assert way(dims).source == road.RAW_GRIB and not way(dims).lines
    assert way(dims[2:] + dims[:2]).source == road.DECODED and way((dims[0],) + dims[2:]).source == road.DECODED
    odd_dims = (dims[0], dims[2], dims[1], dims[3])
    odd = way(odd_dims)
    assert odd.source == road.DECODED
    lines = [text for level, text in odd.lines if "is decoded on the host" in text]
    assert len(lines) == 1 and odd.lines[0][0] == road.INFO and "not ordered (outer..., level, inner...)" in lines[0], lines
    # the decode that road asks for: the bits of the decoded file
    out = raw[var].data.decode()
    assert isinstance(out, np.ndarray) and np.array_equal(out.view(np.uint32), dec[var].values.view(np.uint32))
