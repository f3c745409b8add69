"""CF-packed int16 / uint16 RESULTS on masked-level (3-D) weights: `smm_group_apply_pk`, `smm_group_apply_sb_pk`,
`smm_group_apply_host_pk`, `OperatorGroup.*(cf_out=)` and `Regridder(packed=True, packed_out=True,
packed_out_levels=True)`.  The expectation everywhere is `CFEncode.encode` of the float64 result of the existing group
entry (`OperatorGroup.apply / apply_sb / apply_host(cf=...)`) on the same inputs, compared bit for bit.

Geometry: that of tests/test_gpu_packed_levels.py -- conservative masked-level weights r72x36 -> r24x12 on 8 synthetic
ocean levels.  D = 288 is 4.5 tiles of 64 destination rows (the default tile height of a packed Y: a ragged last
tile) and exactly 18 tiles of 16 (SMM_TUNE_SB_PACKED_Y_ROWS).

Fields: built as `raw_field` of tests/test_gpu_packed_out.py, restated here per level -- dyadic rules (decode scale
1/8, encode scale 1/4), eight latitude plateaus per row drawn from the whole raw range, two plateaus in a hundred in
the top 300 counts (their results round beyond the raw range), one batch row of the first level decoding to exactly
0.0 (t = n + 0.5 on conservative weights too), the fill value where the level's mask is 0 plus scattered cells.  The
float64 expectation of every case is asserted to hold at least one tie, an overflow share within [0.001, 0.05] and a
NaN share within [0.01, 0.6]."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (CdoGenerate, CFDecode, CFEncode, DataArray, Dataset, OperatorGroup, Regridder, SparseOperator,
                           _lib, gridgen, to_device)
from smmregrid_amd.lazy import LazyArray, is_dask
from smmregrid_amd.weights import compute_weights_matrix3d

pytestmark = pytest.mark.gpu
PACKING = ("scale_factor", "add_offset", "_FillValue", "missing_value")
NX, NY, L = 72, 36, 8
S = NX * NY
K_MAX = 9            # links of a conservative row r72x36 -> r24x12

# raw type -> (encode offset, decode offset of the source, raw value that decodes to 0.0, fill values); the encode scale
# is 0.25 and the decode scale 0.125: t = q / 2 + shift, shift placing the top 1 % of the range beyond iinfo.max, and
# t(y = 0) = -4 * encode offset = 4096.5 / 40000.5
RULES = {np.dtype(np.int16): (-1024.125, 3112.5, -24900, (-32768, 7)),
         np.dtype(np.uint16): (-10000.125, -1726.5, 13812, (65535, 300))}
ENC_SCALE, DEC_SCALE = 0.25, 0.125


def enc_rule(raw):
    return CFEncode(ENC_SCALE, RULES[np.dtype(raw)][0], RULES[np.dtype(raw)][3][0], raw)


def dec_rule(raw, dtype):
    return CFDecode(DEC_SCALE, RULES[np.dtype(raw)][1], RULES[np.dtype(raw)][3], dtype)


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} elements differ, first at {bad[:3].tolist()}"


def check_expectation(y64, enc, what):
    """The float64 expectation (existing code) must exercise the rule: conditions, not measurements."""
    info = np.iinfo(enc.raw_dtype)
    fin = np.isfinite(y64)
    t = (y64[fin] - enc.add_offset) / enc.scale_factor
    r = np.rint(t)
    ties = int((np.abs(t - np.floor(t)) == 0.5).sum())
    over = float(((r < info.min) | (r > info.max)).mean())
    nan = float((~fin).mean())
    print(f"{what}: ties {ties}, overflow share {over:.4f}, NaN share {nan:.4f}")
    assert ties > 0, what
    assert 0.001 <= over <= 0.05, (what, over)
    assert 0.01 <= nan <= 0.6, (what, nan)


# ---------------------------------------------------------------- geometry and fields

def ocean_masks(name):
    """"std": the ocean covers 95 % (top) .. 60 % (bottom) of the cells; "deep": 95 % .. 30 % (the SKIPNA cases, which
    renormalise the rows that scattered fills would kill and so need more masked rows to keep their NaN share)."""
    return gridgen.synthetic_ocean_masks(NX, NY, L, top=0.95, bottom=0.6 if name == "std" else 0.3)


def level_weights(masks):
    return gridgen.ConservativeLevels(gridgen.regular_grid(NX, NY), "r24x12").stack(masks, np.arange(L, dtype=np.float64))


_GEO = {}


def geometry(name):
    """The masked-level group, built once per session; masked_levels switches the mask of levels 1 and 5 off."""
    if name not in _GEO:
        masks = ocean_masks(name)
        w3 = level_weights(masks)
        ops = compute_weights_matrix3d(w3, "lev", device=0)
        imask = np.stack([op.mask_apply(masks[i]) for i, op in enumerate(ops)])
        frac = w3["dst_grid_frac"].values
        for i, op in enumerate(ops):
            op.set_epilogue(imask[i], frac[i])
        masked_levels = (~(imask == 1).all(axis=1)).astype(np.uint8)
        assert masked_levels.all()
        masked_levels[[1, 5]] = 0
        _GEO[name] = {"masks": masks, "ops": ops, "grp": OperatorGroup(ops), "masked_levels": masked_levels,
                      "D": ops[0].n_dst, "used": np.array([op.n_used_src for op in ops], dtype=np.int64)}
        assert _GEO[name]["D"] == 288
    return _GEO[name]


def raw_levels(rng, raw, n_outer, level_index, n_inner, masks, shape=(NY, NX)):
    """Raw source values (n_outer, n_lev, n_inner, ny * nx), `raw_field` of tests/test_gpu_packed_out.py per level:
    eight latitude bands per row, each a plateau drawn from the whole raw range plus a few counts of noise; two bands
    in a hundred sit in the top 300 counts, whose results round beyond the raw range.  Row (0, 0, 0) -- the first
    entry of the first level -- decodes to 0.0 everywhere.  The first fill value where the level's mask is 0 (land /
    below the sea floor), either fill value on scattered cells at a rate of 0.03 / K_MAX."""
    info = np.iinfo(raw)
    _, _, q_zero, fills = RULES[np.dtype(raw)]
    ny, nx = shape
    n_lev, nb = len(level_index), 8
    band = np.arange(ny) // -(-ny // nb)
    vals = rng.integers(info.min, info.max + 1, size=(n_outer, n_lev, n_inner, nb))
    top = np.arange(vals.size).reshape(vals.shape) % 50 == 9
    vals[top] = info.max - rng.integers(0, 300, size=int(top.sum()))
    q = vals[..., band][..., None] + rng.integers(-3, 4, size=(n_outer, n_lev, n_inner, ny, nx))
    q = np.clip(q, info.min, info.max).astype(raw)
    q[0, 0, 0] = q_zero
    for f in fills:
        q[q == f] = f + 1 if f < info.max else f - 1
    q = q.reshape(n_outer, n_lev, n_inner, ny * nx)
    for k, l in enumerate(level_index):
        q[:, k][:, :, masks[l] == 0] = fills[0]
    scattered = rng.random(q.shape) < 0.03 / K_MAX
    q[scattered] = np.where(rng.random(int(scattered.sum())) < 0.5, fills[0], fills[-1]).astype(raw)
    return q


def x_of(q, kind):
    """The field one case regrids, and the CFDecode that goes with it (None for float X): kind f32 / f64 -- the host
    decode in that type; pf32 / pf64 -- the raw integers, decoded in the kernels."""
    cf = dec_rule(q.dtype, np.float32 if kind.endswith("32") else np.float64)
    return (q, cf) if kind.startswith("p") else (cf.decode(q), None)


def to_sb(a):
    """(n_outer, n_lev, n_inner, S) -> (n_lev, S, B), batch entry b = o * n_inner + i fastest."""
    n_outer, n_lev, n_inner, s = a.shape
    return np.ascontiguousarray(a.transpose(1, 3, 0, 2).reshape(n_lev, s, n_outer * n_inner))


def sb_dev(a):
    return to_device(to_sb(a), layout="sb")


def sb_of_y(y, transpose):
    """A (n_outer, n_inner, n_lev, D) / (n_lev, n_outer, n_inner, D) result as apply_sb lays it out: (B, n_lev, D) /
    (n_lev, B, D)."""
    if transpose:
        return y.reshape(-1, y.shape[2], y.shape[3])
    return y.reshape(y.shape[0], -1, y.shape[3])


def kept_of_y(y):
    """A transposed (n_outer, n_inner, n_lev, D) result as keep_batch_fastest lays it out: (n_lev, D, B)."""
    return np.ascontiguousarray(y.reshape(-1, y.shape[2], y.shape[3]).transpose(1, 2, 0))


LEVEL_SETS = {"subset": [1, 4, 6], "reversed": [5, 2], "repeated": [3, 3, 0, 7, 3]}
EPILOGUES = [(False, 0.0), (True, 0.0), (True, 0.5)]
XKINDS = ["f32", "f64", "pf32", "pf64"]


def cases(skipna):
    """SKIPNA without any mask has almost no NaN left (only rows whose every link is invalid): it runs masked."""
    return [(m, a) for m, a in EPILOGUES if m or not skipna]


# ---------------------------------------------------------------- 1: the three entries

@pytest.mark.parametrize("kind", XKINDS)
@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_group_entries_equal_encode_of_the_float64_result(hip, raw, kind):
    """All three entries, plain and SKIPNA, every epilogue, both transposes, n_inner = 3, identity levels."""
    rng = np.random.default_rng(211)
    enc = enc_rule(raw)
    lev = np.arange(L, dtype=np.int32)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, raw, 5, lev, 3, g["masks"])
        x, cf = x_of(q, kind)
        dx, dxs = to_device(x), sb_dev(x)
        for masked, area_min in cases(skipna):
            for transpose in (True, False):
                kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna, transpose=transpose, cf=cf)
                what = f"{kind}->{np.dtype(raw).name} masked={masked} area_min={area_min} skipna={skipna} T={transpose}"
                y64 = grp.apply(dx, lev, ml, **kw).to_host()             # the existing entry, float64
                check_expectation(y64, enc, what)
                want = enc.encode(y64)
                got = grp.apply(dx, lev, ml, cf_out=enc, **kw)
                assert got.dtype == np.dtype(raw) and got.shape == y64.shape
                same_bits(got.to_host(), want, what + " native")
                same_bits(grp.apply(dx, lev, ml, cf_out=enc, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host(), want,
                          what + " native, forced SELL")
                want_sb = enc.encode(grp.apply_sb(dxs, lev, ml, **kw).to_host())
                same_bits(want_sb, sb_of_y(want, transpose), what + " the two float64 expectations")
                got = grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw)
                assert got.dtype == np.dtype(raw) and got.layout == "bs"
                same_bits(got.to_host(), want_sb, what + " grouped kernel C")
                with _lib.tuning(sb_packed_y_rows=16):
                    same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw).to_host(), want_sb,
                              what + " grouped kernel C, 16-row tiles")
                same_bits(enc.encode(grp.apply_host(x, lev, ml, **kw)), want, what + " the host float64 expectation")
                got = grp.apply_host(x, lev, ml, cf_out=enc, **kw)
                assert got.dtype == np.dtype(raw)
                same_bits(got, want, what + " host pipeline")
                same_bits(grp.apply_host(x, lev, ml, cf_out=enc, flags=_lib.APPLY_HOST_NO_PACK, **kw), want,
                          what + " host pipeline, whole rows")
            kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna, cf=cf)
            want = enc.encode(grp.apply_sb(dxs, lev, ml, keep_batch_fastest=True, **kw).to_host())
            for rows in (0, 16):
                with _lib.tuning(sb_packed_y_rows=rows):
                    kept = grp.apply_sb(dxs, lev, ml, keep_batch_fastest=True, cf_out=enc, **kw)
                assert kept.layout == "sb" and kept.shape == (L, g["D"], 15) and kept.dtype == np.dtype(raw)
                same_bits(kept.to_host(), want, f"{kind} {kw} grouped kernel C, Y_SB, rows={rows}")


def test_non_dyadic_rule(hip):
    """scale 1.9e-3, offset 2.7e2, int16, for decode and encode alike: a reciprocal multiply or a float32 intermediate
    in a new instantiation shows (t is no longer exact; the comparison is still bit for bit)."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    rng = np.random.default_rng(223)
    lev = np.arange(L, dtype=np.int32)
    enc = CFEncode(1.9e-3, 2.7e2, -32768, np.int16)
    q = raw_levels(rng, np.int16, 7, lev, 1, g["masks"])
    for decode in (np.float32, np.float64):
        cf = CFDecode(1.9e-3, 2.7e2, (-32768, 7), decode)
        for x, rule in ((q, cf), (cf.decode(q), None)):
            for skipna in (False, True):
                kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, cf=rule)
                y64 = grp.apply(to_device(x), lev, ml, **kw).to_host()
                want = enc.encode(y64)
                assert (want == -32768).any() and (want != -32768).any() and np.isnan(y64).any()
                what = f"non-dyadic {np.dtype(decode).name} packed X={rule is not None} skipna={skipna}"
                same_bits(grp.apply(to_device(x), lev, ml, cf_out=enc, **kw).to_host(), want, what + " native")
                for rows in (0, 16):
                    with _lib.tuning(sb_packed_y_rows=rows):
                        same_bits(grp.apply_sb(sb_dev(x), lev, ml, cf_out=enc, **kw).to_host().reshape(want.shape), want,
                                  what + f" grouped kernel C rows={rows}")
                same_bits(grp.apply_host(x, lev, ml, cf_out=enc, **kw), want, what + " host")


# ---------------------------------------------------------------- 2: level sets

@pytest.mark.parametrize("name", ["subset", "reversed", "repeated"])
def test_level_subsets_and_repeats(hip, name):
    lev = np.asarray(LEVEL_SETS[name], dtype=np.int32)
    rng = np.random.default_rng(227)
    raw = np.int16
    enc = enc_rule(raw)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, raw, 9, lev, 2, g["masks"])
        x, cf = x_of(q, "pf32")
        for transpose in (True, False):
            kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, transpose=transpose, cf=cf)
            y64 = grp.apply(to_device(x), lev, ml, **kw).to_host()
            check_expectation(y64, enc, f"{name} skipna={skipna}")
            want = enc.encode(y64)
            same_bits(grp.apply(to_device(x), lev, ml, cf_out=enc, **kw).to_host(), want, f"{name} native")
            same_bits(grp.apply_sb(sb_dev(x), lev, ml, cf_out=enc, **kw).to_host(), sb_of_y(want, transpose),
                      f"{name} grouped C")
            same_bits(grp.apply_host(x, lev, ml, cf_out=enc, **kw), want, f"{name} host")
            same_bits(grp.apply_host(x, lev, ml, cf_out=enc, flags=_lib.APPLY_HOST_NO_PACK, **kw), want, f"{name} host rows")


# ---------------------------------------------------------------- 3: batch shapes

@pytest.mark.parametrize("batch", [1, 2, 3, 8, 31, 32, 131])
def test_batch_shapes(hip, batch):
    """One entry (kernel C's element-wise walk), odd counts (level slabs and Y rows on odd 2-byte elements), the packing
    thresholds of the host pipeline (8, 32), a full and a ragged batch tile (131)."""
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(229 + batch)
    raw = np.uint16
    enc = enc_rule(raw)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, raw, batch, lev, 1, g["masks"])
        x, cf = x_of(q, "pf64")
        kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, cf=cf)
        y64 = grp.apply_sb(sb_dev(x), lev, ml, **kw).to_host()               # (B, L, D)
        check_expectation(y64, enc, f"B={batch} skipna={skipna}")
        want = enc.encode(y64)
        for rows in (0, 16):
            with _lib.tuning(sb_packed_y_rows=rows):
                same_bits(grp.apply_sb(sb_dev(x), lev, ml, cf_out=enc, **kw).to_host(), want, f"grouped C B={batch} rows={rows}")
                kept = grp.apply_sb(sb_dev(x), lev, ml, cf_out=enc, keep_batch_fastest=True, **kw).to_host()   # (L, D, B)
                same_bits(np.ascontiguousarray(kept.transpose(2, 0, 1)), want, f"grouped C Y_SB B={batch} rows={rows}")
        for transpose in (True, False):
            want_h = enc.encode(grp.apply_host(x, lev, ml, transpose=transpose, **kw))
            if transpose:
                same_bits(want_h.reshape(want.shape), want, f"the two expectations B={batch}")
            same_bits(grp.apply_host(x, lev, ml, cf_out=enc, transpose=transpose, **kw), want_h,
                      f"host B={batch} T={transpose}")


# ---------------------------------------------------------------- 4: host chunk forms and bytes

def test_host_chunk_forms_and_bytes(hip):
    """smm_group_apply_host_pk: outer-block chunks of every level, level-major chunks forced through
    SMM_TUNE_HOST_CHUNK_KB down to one level per chunk (the pitched copy of a level range into the transposed
    result, the per-level copies into the other), whole rows, a caller's chunk_outer.  D2H_BYTES is derived: 2 B per
    result cell; H2D_BYTES is what the _cf entry reports for the same call."""
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(233)
    for raw, kind, n_outer, n_inner in ((np.int16, "pf32", 45, 1), (np.uint16, "pf64", 23, 3)):
        enc = enc_rule(raw)
        B = n_outer * n_inner
        for skipna in (False, True):
            g = geometry("deep" if skipna else "std")
            grp, ml, D = g["grp"], g["masked_levels"], g["D"]
            assert g["used"].sum() * 5 <= L * S * 4              # the packing variant applies
            q = raw_levels(rng, raw, n_outer, lev, n_inner, g["masks"])
            x, cf = x_of(q, kind)
            for transpose in (True, False):
                kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, transpose=transpose, cf=cf)
                forms = [(f"kb={kb}", {}, kb) for kb in (0, 1024, 256, 64)]
                forms += [("whole rows", {"flags": _lib.APPLY_HOST_NO_PACK}, 0), ("chunk_outer=7", {"chunk_outer": 7}, 0)]
                want = None
                for label, extra, kb in forms:
                    with _lib.tuning(host_chunk_kb=kb):
                        _lib.host_stats(reset=True)
                        y64 = grp.apply_host(x, lev, ml, **kw, **extra)
                        st64 = _lib.host_stats(reset=True)
                        got = grp.apply_host(x, lev, ml, cf_out=enc, **kw, **extra)
                        st = _lib.host_stats(reset=True)
                    if want is None:
                        check_expectation(y64, enc, f"host chunks B={B} skipna={skipna} T={transpose}")
                        want = enc.encode(y64)
                    what = f"host {label} B={B} skipna={skipna} T={transpose}"
                    same_bits(got, want, what)
                    assert st["d2h_bytes"] == n_outer * n_inner * L * D * 2, (what, st)
                    assert st64["d2h_bytes"] == n_outer * n_inner * L * D * 8, (what, st64)
                    assert st["h2d_bytes"] == st64["h2d_bytes"], (what, st, st64)
                    if kb == 64:                                 # level-major: at most one level per chunk
                        assert st["chunks"] >= L, (what, st)
                    if "chunk_outer" in extra:
                        assert st["chunks"] == -(-n_outer // 7), (what, st)


# ---------------------------------------------------------------- 5: beyond one launch

def test_more_levels_than_one_grouped_launch_grid_limit_and_tile_heights(hip):
    """90 data levels (repeats of the 8 members) at batch 5: two grouped launches of 88 / 2 levels.  Then launch-grid
    limits that leave three levels and one level per grouped launch, one launch per level
    (SMM_TUNE_SB_LEVEL_LAUNCHES), and 16-row tiles against the default 64.  Same bits every time."""
    g = geometry("std")
    grp, ml, D = g["grp"], g["masked_levels"], g["D"]
    rng = np.random.default_rng(239)
    lev = rng.integers(0, L, size=90).astype(np.int32)
    lev[:L] = np.arange(L)
    raw, B = np.int16, 5
    enc = enc_rule(raw)
    q = raw_levels(rng, raw, B, lev, 1, g["masks"])
    x, cf = x_of(q, "pf32")
    dxs = sb_dev(x)
    for skipna in (False, True):
        kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, cf=cf)
        y64 = grp.apply_sb(dxs, lev, ml, **kw).to_host()
        if not skipna:
            check_expectation(y64, enc, "90 levels")
        want = enc.encode(y64)
        want_kept = enc.encode(grp.apply_sb(dxs, lev, ml, keep_batch_fastest=True, **kw).to_host())
        same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw).to_host(), want, "90 levels")
        for rows in (0, 16):
            per_level = -(-D // (rows or 64)) * -(-B // 128)
            try:
                prev_rows = _lib.set_tuning("sb_packed_y_rows", rows)
                same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw).to_host(), want, f"90 levels rows={rows}")
                same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, keep_batch_fastest=True, **kw).to_host(), want_kept,
                          f"90 levels Y_SB rows={rows}")
                for limit in (3 * per_level, per_level):
                    _lib.call("smm_debug_set_grid_limit", limit)
                    same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw).to_host(), want,
                              f"rows={rows} grid limit {limit}")
                    if limit >= 2 * L:          # kernel A: one batch row needs 2 destination blocks x 8 levels
                        got_n = grp.apply(to_device(x[:, :L]), lev[:L], ml, cf_out=enc, **kw).to_host()
                        same_bits(got_n, want[:, :L].reshape(got_n.shape), f"native, grid limit {limit}")
            finally:
                _lib.call("smm_debug_set_grid_limit", 0)
                _lib.set_tuning("sb_packed_y_rows", prev_rows)
        try:
            prev = _lib.set_tuning("sb_level_launches", 1)
            same_bits(grp.apply_sb(dxs, lev, ml, cf_out=enc, **kw).to_host(), want, "one launch per level")
        finally:
            _lib.set_tuning("sb_level_launches", prev)


def test_level_grid_beyond_the_limit_takes_the_per_level_path(hip):
    """A grid limit below one level's own grid (5 destination tiles x 2 batch tiles at batch 131): the fallback, one
    smm_apply_sb per level with its batch cut into runs of batch tiles, passes the encode rule on."""
    g = geometry("std")
    grp, ml, D = g["grp"], g["masked_levels"], g["D"]
    rng = np.random.default_rng(241)
    lev = np.arange(L, dtype=np.int32)
    raw, B = np.uint16, 131
    enc = enc_rule(raw)
    q = raw_levels(rng, raw, B, lev, 1, g["masks"])
    x, cf = x_of(q, "pf64")
    kw = dict(masked=True, remap_area_min=0.5, cf=cf)
    want = enc.encode(grp.apply_sb(sb_dev(x), lev, ml, **kw).to_host())
    per_level = -(-D // 64) * -(-B // 128)
    try:
        _lib.call("smm_debug_set_grid_limit", per_level - 1)
        same_bits(grp.apply_sb(sb_dev(x), lev, ml, cf_out=enc, **kw).to_host(), want, "per-level path")
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)


# ---------------------------------------------------------------- 6: refusals

def test_refusals_and_injected_failure(hip):
    g = geometry("std")
    grp, ml, D = g["grp"], g["masked_levels"], g["D"]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(251)
    raw, B = np.int16, 40
    enc, cf = enc_rule(raw), dec_rule(raw, np.float32)
    other = enc_rule(np.uint16)
    q = raw_levels(rng, raw, B, lev, 1, g["masks"])
    dq, dqs = to_device(q), sb_dev(q)
    kw = dict(masked=True, remap_area_min=0.5, cf=cf)
    want = enc.encode(grp.apply(dq, lev, ml, **kw).to_host())
    assert (want == enc.fill_value).any() and (want != enc.fill_value).any()
    sentinel = 12345

    def code(fn, *a, **k):
        with pytest.raises(_lib.SmmError) as e:
            fn(*a, **k)
        return e.value.code

    y = to_device(np.full((B, 1, L, D), sentinel, raw))
    ys = to_device(np.full((B, L, D), sentinel, raw))
    yu = to_device(np.full((B, 1, L, D), sentinel, np.uint16))
    ysu = to_device(np.full((B, L, D), sentinel, np.uint16))
    # a packed field produces packed results of its own raw type only
    assert code(grp.apply, dq, lev, ml, y=yu, cf_out=other, **kw) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_sb, dqs, lev, ml, y=ysu, cf_out=other, **kw) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_host, q, lev, ml, cf_out=other, **kw) == _lib.SMM_ERR_UNSUPPORTED
    # the LDS tile kernel is not built for packed results; SB_PACKED stays refused for groups
    assert code(grp.apply, dq, lev, ml, y=y, cf_out=enc, flags=_lib.APPLY_KERNEL_TILE, **kw) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_sb, dqs, lev, ml, y=ys, cf_out=enc, flags=_lib.APPLY_KERNEL_TILE, **kw) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_host, q, lev, ml, cf_out=enc, flags=_lib.APPLY_KERNEL_TILE, **kw) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply, to_device(cf.decode(q)), lev, ml, y=y, cf_out=enc, flags=_lib.APPLY_KERNEL_TILE, masked=True,
                remap_area_min=0.5) == _lib.SMM_ERR_UNSUPPORTED                      # float X too
    assert code(grp.apply_sb, dqs, lev, ml, y=ys, cf_out=enc, flags=_lib.APPLY_SB_PACKED, **kw) == _lib.SMM_ERR_UNSUPPORTED
    # a level outside the group: the whole call is validated before the first launch
    bad = lev.copy()
    bad[-1] = L
    assert code(grp.apply_sb, dqs, bad, ml, y=ys, cf_out=enc, **kw) == _lib.SMM_ERR_INVALID
    # a caller's y of another dtype
    with pytest.raises(TypeError):
        grp.apply(dq, lev, ml, y=to_device(np.zeros((B, 1, L, D))), cf_out=enc, **kw)
    with pytest.raises(TypeError):
        grp.apply_sb(dqs, lev, ml, y=yu.reshape(B, L, D), cf_out=enc, **kw)
    with pytest.raises(TypeError):
        grp.apply(dq, lev, ml, cf_out="int16", **kw)
    with pytest.raises(ValueError):
        grp.apply_host(q, lev, ml, cf_out=enc, out_dtype=np.float32, **kw)
    # Y is untouched after every refused call
    for buf in (y, ys, yu, ysu):
        assert (buf.to_host() == sentinel).all()
    # ... and written by the accepted ones
    same_bits(grp.apply(dq, lev, ml, y=y, cf_out=enc, **kw).to_host(), want, "native into the caller's y")
    same_bits(grp.apply_sb(dqs, lev, ml, y=ys, cf_out=enc, **kw).to_host().reshape(want.shape), want, "grouped C into y")
    # the C entries: enc NULL is the _cf entry unchanged
    lib = _lib.load()
    y64 = to_device(np.zeros((B, 1, L, D)))
    lp, mp = lev.ctypes.data_as(ctypes.c_void_p), ml.ctypes.data_as(ctypes.c_void_p)
    st = cf._struct(np.int16)
    rc = lib.smm_group_apply_pk(grp.handle, ctypes.c_void_p(dq.ptr), _lib.SMM_I16, L * S, S, S, ctypes.c_void_p(y64.ptr),
                                _lib.SMM_F64, L * D, D, L * D, B, L, 1, lp, mp, 0.5, _lib.APPLY_MASKED, None,
                                ctypes.byref(st), None)
    assert rc == _lib.SMM_OK, lib.smm_last_error()
    same_bits(enc.encode(y64.to_host()), want, "smm_group_apply_pk, enc NULL")
    # an odd Y address is refused
    buf = to_device(np.zeros(2 + B * L * D, raw))
    est = enc._struct()
    rc = lib.smm_group_apply_sb_pk(grp.handle, ctypes.c_void_p(dqs.ptr), _lib.SMM_I16, S * B, B, ctypes.c_void_p(buf.ptr + 1),
                                   _lib.SMM_I16, D, L * D, B, L, lp, mp, 0.5, _lib.APPLY_MASKED, None, ctypes.byref(st),
                                   ctypes.byref(est))
    assert rc == _lib.SMM_ERR_INVALID
    # an injected chunk failure on the packed-result group pipeline surfaces as SMM_ERR_HIP; the next call succeeds
    for flags in (0, _lib.APPLY_HOST_NO_PACK):
        _lib.call("smm_debug_fail_at_chunk", 0)
        try:
            with pytest.raises(_lib.SmmError) as e:
                grp.apply_host(q, lev, ml, cf_out=enc, flags=flags, **kw)
            assert e.value.code == _lib.SMM_ERR_HIP and "injected failure" in str(e.value)
        finally:
            _lib.call("smm_debug_fail_at_chunk", -1)
        same_bits(grp.apply_host(q, lev, ml, cf_out=enc, flags=flags, **kw), want, "after the failure")
    _lib.call("smm_debug_staging_faults", 0, 0)
    try:
        with pytest.raises(_lib.SmmError) as e:
            grp.apply_host(q, lev, ml, cf_out=enc, **kw)
        assert e.value.code == _lib.SMM_ERR_ALLOC
    finally:
        _lib.call("smm_debug_staging_faults", 0, -1)
    same_bits(grp.apply_host(q, lev, ml, cf_out=enc, **kw), want, "after the staging fault")


# ---------------------------------------------------------------- 7: a chain

@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_chain_level_slab_feeds_a_second_regrid(hip, raw):
    """Level 0's (D, B) slab of a keep_batch_fastest raw result is what SparseOperator.apply_sb(cf=) consumes."""
    g = geometry("std")
    grp, ml, D = g["grp"], g["masked_levels"], g["D"]
    w2 = gridgen.conservative_weights("r24x12", "r12x6")
    op2 = SparseOperator(w2.sizes["src_grid_size"], w2.sizes["dst_grid_size"], w2["src_address"].values,
                         w2["dst_address"].values, w2["remap_matrix"].values, device=0)
    assert op2.n_src == D
    rng = np.random.default_rng(257)
    lev = np.arange(L, dtype=np.int32)
    B = 33
    enc = enc_rule(raw)
    q = raw_levels(rng, raw, B, lev, 1, g["masks"])
    cf1 = dec_rule(raw, np.float32)
    cf2 = CFDecode.from_attrs(enc.attrs(), dtype=np.float64, raw_dtype=raw)
    kw = dict(masked=True, remap_area_min=0.5, cf=cf1, keep_batch_fastest=True)
    mid64 = grp.apply_sb(sb_dev(q), lev, ml, **kw).to_host()                     # (L, D, B) float64
    slab = enc.encode(mid64[0])                                                  # the host statement of the chain
    assert (slab == enc.fill_value).any() and (slab != enc.fill_value).any()
    want = op2.apply(to_device(np.ascontiguousarray(cf2.decode(slab).T))).to_host()
    assert np.isnan(want).any() and np.isfinite(want).any()
    mid = grp.apply_sb(sb_dev(q), lev, ml, cf_out=enc, **kw)
    assert mid.dtype == np.dtype(raw) and mid.layout == "sb" and mid.shape == (L, D, B)
    got = op2.apply_sb(mid.rows(0, 1).reshape(D, B), cf=cf2).to_host()
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])


# ---------------------------------------------------------------- 8: Regridder

def _ocean_da(rng, deep, nt=5, name="so", raw=np.int16):
    """A packed variable on 6 ocean levels whose own attributes decode and encode it (as `_packed_da` of
    tests/test_gpu_packed_out.py), and its host-decoded float twin."""
    g = gridgen.parse_grid(f"r{NX}x{NY}")
    levels = np.array([5.0, 50.0, 200.0, 500.0, 1000.0, 2000.0])
    masks = gridgen.synthetic_ocean_masks(NX, NY, len(levels), top=0.95, bottom=0.3 if deep else 0.6)
    enc_off, _, _, fills = RULES[np.dtype(raw)]
    q = raw_levels(rng, raw, nt, np.arange(len(levels)), 1, masks).reshape(nt, len(levels), NY, NX)
    q[q == fills[1]] = fills[0]                        # one fill attribute
    coords = {"time": np.arange(nt), "lev": levels, "lat": g.lat, "lon": g.lon}
    attrs = {"scale_factor": ENC_SCALE, "add_offset": enc_off, "_FillValue": np.dtype(raw).type(fills[0]), "units": "psu"}
    da = DataArray(q, dims=("time", "lev", "lat", "lon"), coords=coords, name=name, attrs=attrs)
    cf = CFDecode.from_attrs(attrs, raw_dtype=raw)
    dec = DataArray(cf.decode(q), dims=da.dims, coords=coords, name=name, attrs={"units": "psu"})
    return da, dec


def _log_lines(caplog, text):
    return sum(text in r.getMessage() for r in caplog.records)


class _DaskLike:
    """What `lazy.is_dask` recognises (`dask`, `chunks`, `map_blocks`) around a numpy array: regrid3d computes a
    dask-backed field where it needs it, so the stand-in only has to hand its values over when asked."""
    dask = chunks = None

    def __init__(self, values):
        self._values, self.shape, self.dtype, self.ndim = values, values.shape, values.dtype, values.ndim
        self.computed = 0

    def map_blocks(self, *a, **k):
        raise AssertionError("masked-level fields are computed whole")

    def compute(self):
        return self.__array__()

    def __array__(self, dtype=None, copy=None):
        self.computed += 1
        return self._values if dtype is None else self._values.astype(dtype)


@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("packed_levels", [False, True])
def test_regridder_packed_out_levels(hip, caplog, packed_levels, transpose):
    rng = np.random.default_rng(263)
    raw = np.int16
    da, dec = _ocean_da(rng, deep=False)
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    kw = dict(weights=w3, transpose=transpose, packed=True, packed_levels=packed_levels)
    enc = CFEncode.from_attrs(da.attrs, raw)
    f64 = Regridder(**kw).regrid(da)                                  # the existing path: float64
    assert f64.values.dtype == np.float64
    want = enc.encode(f64.values)
    assert (want == enc.fill_value).any() and (want != enc.fill_value).any()
    new = dict(packed_out=True, packed_out_levels=True, loglevel="INFO", **kw)

    def check(got, want, what, dims=f64.dims):
        assert got.dims == dims, what
        assert np.asarray(got.values).dtype == np.dtype(raw), what
        same_bits(np.asarray(got.values), want, what)
        assert got.attrs == da.attrs and all(k in got.attrs for k in PACKING[:3]), what

    with caplog.at_level("INFO"):
        rg = Regridder(**new)
        check(rg.regrid(da), want, "host field")
        dev = DataArray(to_device(da.data), dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs)
        out = rg.regrid(dev)
        assert out.data.dtype == np.dtype(raw) and out.data.layout == "bs"
        check(out, want, "DeviceArray")
        sb_dims = ("lev", "lat", "lon", "time")
        sb = DataArray(to_device(np.ascontiguousarray(da.data.transpose(1, 2, 3, 0)), layout="sb"), dims=sb_dims,
                       coords=da.coords, name=da.name, attrs=da.attrs)
        check(rg.regrid(sb), want, "batch-fastest DeviceArray")
        kept = Regridder(keep_batch_fastest=True, **new).regrid(sb)
        assert kept.data.layout == "sb" and kept.data.dtype == np.dtype(raw)
        lev_axis = f64.dims.index("lev")
        want_kept = np.ascontiguousarray(np.moveaxis(want, lev_axis, 0).transpose(0, 2, 3, 1))   # (lev, lat, lon, time)
        check(kept, want_kept, "kept batch-fastest", dims=("lev", "lat", "lon", "time"))
        lazy = Regridder(lazy=True, **new).regrid(da)
        assert isinstance(lazy.data, LazyArray) and lazy.data.dtype == np.dtype(raw) and not lazy.data.computed
        check(lazy, want, "lazy")
        for is_lazy in (False, True):
            backed = _DaskLike(da.data)
            assert is_dask(backed)
            got = Regridder(lazy=is_lazy, **new).regrid(
                DataArray(backed, dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs))
            check(got, want, f"dask-like, lazy={is_lazy}")
            assert backed.computed >= 1
        try:
            import dask.array as dsa
        except ImportError:
            dsa = None
        if dsa is not None:
            got = rg.regrid(DataArray(dsa.from_array(da.data, chunks=(2, 6, NY, NX)), dims=da.dims, coords=da.coords,
                                      name=da.name, attrs=da.attrs))
            check(got, want, "dask-backed")
    assert _log_lines(caplog, "encoded on the host") == 0 and _log_lines(caplog, "stays float64") == 0
    caplog.clear()
    # without the new keyword the two lines still appear: the default is unchanged
    with caplog.at_level("INFO"):
        old = Regridder(packed_out=True, loglevel="INFO", **kw)
        same_bits(old.regrid(da).values, want, "host encode")
        out = old.regrid(dev)
    assert _log_lines(caplog, "encoded on the host") == 1 and _log_lines(caplog, "stays float64") == 1
    assert out.values.dtype == np.float64 and not set(PACKING) & set(out.attrs)


def test_regridder_dataset_mixing_levels_packed_single_level_and_float(hip, caplog):
    """A Dataset with a packed variable on all levels, a packed single-level variable (a Regridder built from weights
    serves one grid type: the surface variable keeps a `lev` axis of length one), a packed variable without a fill
    attribute and a float variable."""
    rng = np.random.default_rng(269)
    da, dec = _ocean_da(rng, deep=False)
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    other = DataArray(35.0 + rng.standard_normal(dec.data.shape), dims=da.dims, coords=da.coords, name="thetao",
                      attrs={"units": "degC"})
    other.data[np.isnan(dec.data)] = np.nan
    top = DataArray(np.ascontiguousarray(da.data[:, :1]), dims=da.dims, name="sos", attrs=dict(da.attrs),
                    coords={**da.coords, "lev": da.coords["lev"].values[:1]})
    nofill = DataArray(da.data.copy(), dims=da.dims, coords=da.coords, name="so_nofill",
                       attrs={k: v for k, v in da.attrs.items() if k != "_FillValue"})
    ds = Dataset({"so": da, "sos": top, "so_nofill": nofill, "thetao": other}, coords=dict(da.coords))
    kw = dict(weights=w3, packed=True, packed_levels=True)
    today = Regridder(**kw).regrid(ds)
    with caplog.at_level("INFO"):
        out = Regridder(packed_out=True, packed_out_levels=True, loglevel="INFO", **kw).regrid(ds)
    assert _log_lines(caplog, "encoded on the host") == 0 and _log_lines(caplog, "stays float64") == 0
    assert _log_lines(caplog, "comes back as float64") == 1
    enc = CFEncode.from_attrs(da.attrs, np.int16)
    for name in ("so", "sos"):
        assert out[name].values.dtype == np.int16 and out[name].attrs == da.attrs
        same_bits(out[name].values, enc.encode(today[name].values), name)
    for name in ("so_nofill", "thetao"):
        assert out[name].values.dtype == np.float64
        assert np.array_equal(out[name].values.view(np.uint64), today[name].values.view(np.uint64)), name
        assert out[name].attrs == today[name].attrs and not set(PACKING) & set(out[name].attrs)
