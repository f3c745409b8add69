"""CF-packed int16 / uint16 fields on masked-level (3-D) weights regridded raw: `smm_group_apply_cf`,
`smm_group_apply_sb_cf`, `smm_group_apply_host_cf`, `OperatorGroup.*(cf=)` and `Regridder(packed=True,
packed_levels=True)`.  The expectation everywhere is this library's float path on `CFDecode.decode(q)` with the same
flags, compared bit for bit (no tolerance); one case per entry is also compared with the CPU oracle's level walk.
Every expectation has between 1 % and 50 % NaN and is finite elsewhere (asserted on the expectation, share printed)."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (CdoGenerate, CFDecode, DataArray, Dataset, OperatorGroup, Regridder, _lib, gridgen,
                           to_device)
from smmregrid_amd.weights import compute_weights_matrix3d

pytestmark = pytest.mark.gpu
PACKING = ("scale_factor", "add_offset", "_FillValue", "missing_value")
NX, NY, L = 72, 36, 8
S = NX * NY


def bits_equal(a, b, what=""):
    a, b = np.asarray(a), np.asarray(b)
    assert a.shape == b.shape and a.dtype == b.dtype, (what, a.shape, b.shape, a.dtype, b.dtype)
    ia = a.view(np.uint64 if a.dtype == np.float64 else np.uint32)
    ib = b.view(np.uint64 if b.dtype == np.float64 else np.uint32)
    na, nb = np.isnan(a), np.isnan(b)
    assert np.array_equal(na, nb), f"{what}: NaN pattern differs at {np.argwhere(na != nb)[:5]}"
    assert np.array_equal(ia[~na], ib[~nb]), f"{what}: values are not bit identical"


def nan_share_ok(y, what=""):
    """Neither an all-NaN nor a fill-free case may pass silently: 1 % .. 50 % NaN, the rest finite."""
    share = float(np.isnan(y).mean())
    print(f"{what}: NaN share of the host-decoded expectation {share:.4f}")
    assert 0.01 <= share <= 0.50, (what, share)
    assert np.isfinite(y[~np.isnan(y)]).all(), what


# ---------------------------------------------------------------- geometry and fields

_GEO = {}


def geometry(name):
    """Conservative masked-level weights r72x36 -> r24x12 on 8 synthetic ocean levels, built once per session.
    "std": the ocean covers 95 % (top) .. 60 % (bottom) of the cells -- the plain cases; "deep": 95 % .. 30 % --
    the SKIPNA cases, which renormalise the rows that scattered fills would kill and so need more masked rows to
    keep their NaN share.  masked_levels switches the mask of levels 1 and 5 off."""
    if name not in _GEO:
        masks = gridgen.synthetic_ocean_masks(NX, NY, L, top=0.95, bottom=0.6 if name == "std" else 0.3)
        w3 = gridgen.ConservativeLevels(gridgen.regular_grid(NX, NY), "r24x12").stack(masks, np.arange(L, dtype=np.float64))
        ops = compute_weights_matrix3d(w3, "lev", device=0)
        imask = np.stack([op.mask_apply(masks[i]) for i, op in enumerate(ops)])
        frac = w3["dst_grid_frac"].values
        for i, op in enumerate(ops):
            op.set_epilogue(imask[i], frac[i])
        masked_levels = (~(imask == 1).all(axis=1)).astype(np.uint8)
        assert masked_levels.all()
        masked_levels[[1, 5]] = 0
        _GEO[name] = {"masks": masks, "ops": ops, "grp": OperatorGroup(ops), "imask": imask, "frac": frac,
                      "csrs": [op.export_csr() for op in ops], "masked_levels": masked_levels, "D": ops[0].n_dst,
                      "used": np.array([op.n_used_src for op in ops], dtype=np.int64)}
    return _GEO[name]


def rule(dtype, decode):
    """int16: ERA5-like scale and an offset large enough that the float32 decode rounds; uint16: a negative scale.
    Two distinct fill values each, one at the edge of the raw range (-32768 / 65535)."""
    if dtype == np.int16:
        return CFDecode(1.9e-3, 2.7e2, (-32768, 7), decode)
    return CFDecode(-0.25, 12.5, (65535, 300), decode)


def raw_levels(rng, dtype, n_outer, level_index, n_inner, masks, fills, rate=0.03):
    """(n_outer, n_lev, n_inner, S) raw values over the whole range of the type; the first fill value where the
    level's mask is 0 (land / below the sea floor) and either fill value on 3 % of all cells, scattered."""
    info = np.iinfo(dtype)
    q = rng.integers(info.min, info.max + 1, size=(n_outer, len(level_index), n_inner, S)).astype(dtype)
    for f in fills:                                  # the range is full: values that equal a fill by chance move on
        q[q == f] = f + 1 if f < info.max else f - 1
    for k, l in enumerate(level_index):
        q[:, k][:, :, masks[l] == 0] = fills[0]
    scattered = rng.random(q.shape) < rate
    q[scattered] = np.where(rng.random(int(scattered.sum())) < 0.5, fills[0], fills[-1]).astype(dtype)
    return q


def to_sb(a):
    """(n_outer, n_lev, n_inner, S) -> (n_lev, S, B), batch entry b = o * n_inner + i fastest."""
    n_outer, n_lev, n_inner, s = a.shape
    return np.ascontiguousarray(a.transpose(1, 3, 0, 2).reshape(n_lev, s, n_outer * n_inner))


def sb_dev(a):
    return to_device(to_sb(a), layout="sb")


LEVEL_SETS = {"identity": list(range(L)), "subset": [1, 4, 6], "reversed": [5, 2], "repeated": [3, 3, 0, 7, 3]}
EPILOGUES = [(False, 0.0), (True, 0.0), (True, 0.5)]


def cases(skipna):
    """SKIPNA without any mask has almost no NaN left (only rows whose every link is invalid): it runs masked."""
    return [(m, a) for m, a in EPILOGUES if m or not skipna]


# ---------------------------------------------------------------- 1, 2: the three entries

@pytest.mark.parametrize("decode", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dtype", [np.int16, np.uint16], ids=["i16", "u16"])
def test_group_entries_equal_the_host_decode(hip, dtype, decode):
    """All three entries, plain and SKIPNA, every epilogue, both transposes, n_inner = 3, identity levels."""
    rng = np.random.default_rng(101)
    cf = rule(dtype, decode)
    lev = np.arange(L, dtype=np.int32)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, dtype, 5, lev, 3, g["masks"], cf.fill_values)
        x = cf.decode(q)
        assert x.dtype == decode and np.isnan(x).any()
        dq, dx, dqs, dxs = to_device(q), to_device(x), sb_dev(q), sb_dev(x)
        for masked, area_min in cases(skipna):
            for transpose in (True, False):
                kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna, transpose=transpose)
                what = f"{np.dtype(dtype).name}->{np.dtype(decode).name} {kw}"
                want = grp.apply(dx, lev, ml, **kw).to_host()
                nan_share_ok(want, what)
                bits_equal(grp.apply(dq, lev, ml, cf=cf, **kw).to_host(), want, what + " native")
                bits_equal(grp.apply(dq, lev, ml, cf=cf, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host(), want,
                           what + " native, forced SELL")
                want_sb = grp.apply_sb(dxs, lev, ml, **kw).to_host()
                bits_equal(want_sb.reshape(want.shape), want, what + " existing grouped kernel C")
                bits_equal(grp.apply_sb(dqs, lev, ml, cf=cf, **kw).to_host(), want_sb, what + " grouped kernel C")
                want_h = grp.apply_host(x, lev, ml, **kw)
                bits_equal(want_h, want, what + " existing host pipeline")
                bits_equal(grp.apply_host(q, lev, ml, cf=cf, **kw), want, what + " host pipeline")
                bits_equal(grp.apply_host(q, lev, ml, cf=cf, flags=_lib.APPLY_HOST_NO_PACK, **kw), want,
                           what + " host pipeline, whole rows")
            kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
            kept = grp.apply_sb(dqs, lev, ml, cf=cf, keep_batch_fastest=True, **kw)
            assert kept.layout == "sb" and kept.shape == (L, g["D"], 15)
            bits_equal(kept.to_host(), grp.apply_sb(dxs, lev, ml, keep_batch_fastest=True, **kw).to_host(),
                       f"{np.dtype(dtype).name} {kw} grouped kernel C, Y_SB")


@pytest.mark.parametrize("dtype,decode", [(np.int16, np.float32), (np.uint16, np.float64)])
def test_each_entry_against_the_oracle(hip, dtype, decode):
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    rng = np.random.default_rng(103)
    cf = rule(dtype, decode)
    for name in ("identity", "repeated"):
        lev = np.asarray(LEVEL_SETS[name], dtype=np.int32)
        q = raw_levels(rng, dtype, 7, lev, 2, g["masks"], cf.fill_values)
        for transpose in (True, False):
            ref = oracle.apply_levels(g["csrs"], cf.decode(q), 1, lev, ml.astype(bool), g["imask"], g["frac"], 0.5,
                                      transpose=transpose)
            nan_share_ok(ref, f"oracle {name}")
            kw = dict(masked=True, remap_area_min=0.5, transpose=transpose, cf=cf)
            bits_equal(grp.apply(to_device(q), lev, ml, **kw).to_host(), ref, "native vs oracle")
            bits_equal(grp.apply_sb(sb_dev(q), lev, ml, **kw).to_host().reshape(ref.shape), ref, "grouped C vs oracle")
            bits_equal(grp.apply_host(q, lev, ml, **kw), ref, "host pipeline vs oracle")


@pytest.mark.parametrize("name", ["subset", "reversed", "repeated"])
def test_level_subsets_and_repeats(hip, name):
    lev = np.asarray(LEVEL_SETS[name], dtype=np.int32)
    rng = np.random.default_rng(107)
    cf = rule(np.int16, np.float32)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, np.int16, 9, lev, 2, g["masks"], cf.fill_values)
        x = cf.decode(q)
        for transpose in (True, False):
            kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, transpose=transpose)
            want = grp.apply(to_device(x), lev, ml, **kw).to_host()
            nan_share_ok(want, f"{name} skipna={skipna}")
            bits_equal(grp.apply(to_device(q), lev, ml, cf=cf, **kw).to_host(), want, f"{name} native")
            bits_equal(grp.apply_sb(sb_dev(q), lev, ml, cf=cf, **kw).to_host().reshape(want.shape), want, f"{name} grouped C")
            bits_equal(grp.apply_host(q, lev, ml, cf=cf, **kw), want, f"{name} host")
            bits_equal(grp.apply_host(q, lev, ml, cf=cf, flags=_lib.APPLY_HOST_NO_PACK, **kw), want, f"{name} host rows")


# ---------------------------------------------------------------- 3: batch shapes

@pytest.mark.parametrize("batch", [1, 2, 3, 8, 31, 32, 131])
def test_batch_shapes(hip, batch):
    """One entry (kernel C's element-wise walk), odd counts (slabs and rows that start on an odd element), a full
    and a ragged batch tile."""
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(109 + batch)
    cf = rule(np.uint16, np.float32)
    for skipna in (False, True):
        g = geometry("deep" if skipna else "std")
        grp, ml = g["grp"], g["masked_levels"]
        q = raw_levels(rng, np.uint16, batch, lev, 1, g["masks"], cf.fill_values)
        x = cf.decode(q)
        kw = dict(masked=True, remap_area_min=0.5, skipna=skipna)
        want = grp.apply(to_device(x), lev, ml, **kw).to_host()
        nan_share_ok(want, f"B={batch} skipna={skipna}")
        bits_equal(grp.apply(to_device(q), lev, ml, cf=cf, **kw).to_host(), want, f"native B={batch}")
        bits_equal(grp.apply_sb(sb_dev(q), lev, ml, cf=cf, **kw).to_host().reshape(want.shape), want, f"grouped C B={batch}")
        kept = grp.apply_sb(sb_dev(q), lev, ml, cf=cf, keep_batch_fastest=True, **kw).to_host()      # (L, D, B)
        bits_equal(np.ascontiguousarray(kept.transpose(2, 0, 1)).reshape(want.shape), want, f"grouped C Y_SB B={batch}")
        bits_equal(grp.apply_host(q, lev, ml, cf=cf, **kw), want, f"host B={batch}")


def test_host_chunk_forms(hip):
    """smm_group_apply_host_cf: outer-block chunks of every level (batch >= 32), level-major chunks forced through
    SMM_TUNE_HOST_CHUNK_KB down to one level and a block of the outer axis per chunk, with odd batch counts so that
    slabs inside a staging chunk start on odd elements; whole rows; a caller's chunk_outer."""
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(113)
    for dtype, decode, n_outer, n_inner in ((np.int16, np.float32, 45, 1), (np.uint16, np.float64, 23, 3)):
        cf = rule(dtype, decode)
        B = n_outer * n_inner
        for skipna, transpose in ((False, True), (True, False)):
            g = geometry("deep" if skipna else "std")
            grp, ml = g["grp"], g["masked_levels"]
            assert g["used"].sum() * 5 <= L * S * 4              # the packing variant applies
            q = raw_levels(rng, dtype, n_outer, lev, n_inner, g["masks"], cf.fill_values)
            x = cf.decode(q)
            kw = dict(masked=True, remap_area_min=0.5, skipna=skipna, transpose=transpose)
            want = grp.apply(to_device(x), lev, ml, **kw).to_host()
            nan_share_ok(want, f"host chunks B={B} skipna={skipna}")
            for kb in (0, 1024, 256, 64):
                with _lib.tuning(host_chunk_kb=kb):
                    _lib.host_stats(reset=True)
                    got = grp.apply_host(q, lev, ml, cf=cf, **kw)
                    st = _lib.host_stats(reset=True)
                bits_equal(got, want, f"host kb={kb} B={B}")
                assert st["h2d_bytes"] == 2 * g["used"].sum() * B, (kb, st)       # packed in every form, no padding
                if kb == 64:                                     # level-major: at most one level per chunk (a level's
                    assert st["chunks"] >= L, st                 # used cells x 45 entries x 2 B alone exceed 64 KiB)
            bits_equal(grp.apply_host(q, lev, ml, cf=cf, flags=_lib.APPLY_HOST_NO_PACK, **kw), want, "whole rows")
            _lib.host_stats(reset=True)
            bits_equal(grp.apply_host(q, lev, ml, cf=cf, chunk_outer=7, **kw), want, "chunk_outer=7")
            assert _lib.host_stats(reset=True)["chunks"] == -(-n_outer // 7)


# ---------------------------------------------------------------- 4: beyond one launch

def test_more_levels_than_one_grouped_launch_and_grid_limit(hip):
    """200 data levels (repeats of the 8 members): three grouped launches of 88 / 88 / 24 levels.  Then launch-grid
    limits that leave 3 levels per grouped launch, and one below a single level's grid: the per-level path, which
    cuts the batch of each level into runs of batch tiles.  Same bits every time."""
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    rng = np.random.default_rng(127)
    lev = rng.integers(0, L, size=200).astype(np.int32)
    lev[:L] = np.arange(L)
    cf = rule(np.int16, np.float64)
    B = 131
    q = raw_levels(rng, np.int16, B, lev, 1, g["masks"], cf.fill_values)
    dqs, dxs = sb_dev(q), sb_dev(cf.decode(q))
    per_level = -(-g["D"] // 16) * -(-B // 128)
    for skipna in (False, True):
        kw = dict(masked=True, remap_area_min=0.5, skipna=skipna)
        want = grp.apply_sb(dxs, lev, ml, **kw).to_host()
        if not skipna:
            nan_share_ok(want, "200 levels")
        bits_equal(grp.apply_sb(dqs, lev, ml, cf=cf, **kw).to_host(), want, "200 levels")
        for limit in (3 * per_level, per_level - 1):
            _lib.call("smm_debug_set_grid_limit", limit)
            try:
                got = grp.apply_sb(dqs, lev, ml, cf=cf, **kw).to_host()
                got_n = grp.apply(to_device(q[:, :L]), lev[:L], ml, cf=cf, **kw).to_host()
            finally:
                _lib.call("smm_debug_set_grid_limit", 0)
            bits_equal(got, want, f"grid limit {limit}")
            bits_equal(got_n, want[:, :L].reshape(got_n.shape), f"native, grid limit {limit}")
        with _lib.tuning(sb_level_launches=1):
            bits_equal(grp.apply_sb(dqs, lev, ml, cf=cf, **kw).to_host(), want, "one launch per level")


# ---------------------------------------------------------------- 5: bytes

def test_host_pipeline_ships_two_bytes_per_used_cell(hip):
    """Derived, not measured: the packed pipeline ships the used source cells of every selected level once per
    batch entry -- 2 B each for the raw field (the slabs of a chunk lie back to back: no padding), 4 B each for the
    float32 decode; whole rows ship every cell of every level."""
    g = geometry("std")
    grp, ml, used = g["grp"], g["masked_levels"], g["used"]
    rng = np.random.default_rng(131)
    cf = rule(np.int16, np.float32)
    for name, n_outer, n_inner in (("identity", 33, 1), ("repeated", 11, 3), ("identity", 9, 1)):
        lev = np.asarray(LEVEL_SETS[name], dtype=np.int32)
        cells = int(used[lev].sum())
        assert cells * 5 <= lev.size * S * 4                      # the packing variant applies to this selection
        B = n_outer * n_inner
        q = raw_levels(rng, np.int16, n_outer, lev, n_inner, g["masks"], cf.fill_values)
        x = cf.decode(q)
        kw = dict(masked=True, remap_area_min=0.5)
        want = grp.apply(to_device(x), lev, ml, **kw).to_host()
        nan_share_ok(want, f"bytes {name} B={B}")
        _lib.host_stats(reset=True)
        bits_equal(grp.apply_host(q, lev, ml, cf=cf, **kw), want, "raw")
        st = _lib.host_stats(reset=True)
        assert st["h2d_bytes"] == 2 * cells * B, (name, B, st)
        assert st["d2h_bytes"] == 8 * lev.size * g["D"] * B, st
        bits_equal(grp.apply_host(x, lev, ml, **kw), want, "float32")
        assert _lib.host_stats(reset=True)["h2d_bytes"] == 2 * (2 * cells * B)
        bits_equal(grp.apply_host(q, lev, ml, cf=cf, flags=_lib.APPLY_HOST_NO_PACK, **kw), want, "raw whole rows")
        assert _lib.host_stats(reset=True)["h2d_bytes"] == 2 * lev.size * S * B


# ---------------------------------------------------------------- 6: refusals

def test_refusals_and_injected_failure(hip):
    g = geometry("std")
    grp, ml = g["grp"], g["masked_levels"]
    lev = np.arange(L, dtype=np.int32)
    rng = np.random.default_rng(137)
    cf = rule(np.int16, np.float32)
    q = raw_levels(rng, np.int16, 40, lev, 1, g["masks"], cf.fill_values)
    x = cf.decode(q)
    dq, dqs = to_device(q), sb_dev(q)

    def code(fn, *a, **k):
        with pytest.raises(_lib.SmmError) as e:
            fn(*a, **k)
        return e.value.code

    for fn, arg in ((grp.apply, dq), (grp.apply_sb, dqs), (grp.apply_host, q)):
        assert code(fn, arg, lev, ml, cf=cf, out_dtype=np.float32) == _lib.SMM_ERR_UNSUPPORTED     # float32 results
        assert code(fn, arg, lev, ml, cf=cf, flags=_lib.APPLY_NO_FILL) == _lib.SMM_ERR_INVALID     # the decode makes NaN
    assert code(grp.apply, dq, lev, ml, cf=cf, flags=_lib.APPLY_KERNEL_TILE) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_host, q, lev, ml, cf=cf, flags=_lib.APPLY_KERNEL_TILE) == _lib.SMM_ERR_UNSUPPORTED
    assert code(grp.apply_sb, dqs, lev, ml, cf=cf, flags=_lib.APPLY_SB_PACKED) == _lib.SMM_ERR_UNSUPPORTED
    with pytest.raises(TypeError):                               # a rule with a float field
        grp.apply(to_device(x), lev, ml, cf=cf)
    with pytest.raises(TypeError):
        grp.apply_host(x, lev, ml, cf=cf)
    with pytest.raises(TypeError):                               # an integer device field without a rule
        grp.apply(dq, lev, ml)
    # launch info: kernel A for packed groups whatever the group's plan; a forced tile kernel is refused
    for dt in (np.int16, np.uint16):
        info = grp.launch_info(40, L, 1, dt)
        assert info["kernel"] == "sell" and info == grp.launch_info(40, L, 1, np.float32, flags=_lib.APPLY_KERNEL_SELL)
        assert code(grp.launch_info, 40, L, 1, dt, flags=_lib.APPLY_KERNEL_TILE) == _lib.SMM_ERR_UNSUPPORTED
    # the C entries themselves
    lib = _lib.load()
    D = g["D"]
    y = to_device(np.zeros((40, 1, L, D)))
    ys = to_device(np.zeros((40, L, D)))
    out = np.zeros((40, 1, L, D))
    lp, mp = lev.ctypes.data_as(ctypes.c_void_p), ml.ctypes.data_as(ctypes.c_void_p)
    st = cf._struct(np.int16)
    native = lambda entry, ptr, dt, *tail: getattr(lib, entry)(grp.handle, ctypes.c_void_p(ptr), dt, L * S, S, S,
                                                               ctypes.c_void_p(y.ptr), _lib.SMM_F64, L * D, D, L * D,
                                                               40, L, 1, lp, mp, 0.5, _lib.APPLY_MASKED, None, *tail)
    sb = lambda entry, ptr, dt, *tail: getattr(lib, entry)(grp.handle, ctypes.c_void_p(ptr), dt, S * 40, 40,
                                                           ctypes.c_void_p(ys.ptr), _lib.SMM_F64, D, L * D, 40, L,
                                                           lp, mp, 0.5, _lib.APPLY_MASKED, None, *tail)
    host = lambda entry, arr, dt, *tail: getattr(lib, entry)(grp.handle, arr.ctypes.data_as(ctypes.c_void_p), dt,
                                                             out.ctypes.data_as(ctypes.c_void_p), _lib.SMM_F64, 40, L,
                                                             1, 1, lp, mp, 0.5, _lib.APPLY_MASKED, 0, *tail)
    dx, dxs = to_device(x), sb_dev(x)
    want = grp.apply(dx, lev, ml, masked=True, remap_area_min=0.5).to_host()
    nan_share_ok(want, "refusals")
    for call, plain, raw, flt in ((native, "smm_group_apply", dq.ptr, dx.ptr), (sb, "smm_group_apply_sb", dqs.ptr, dxs.ptr),
                                  (host, "smm_group_apply_host", q, x)):
        assert call(plain, raw, _lib.SMM_I16) == _lib.SMM_ERR_UNSUPPORTED, plain       # integer codes, plain entries
        assert call(plain, raw, _lib.SMM_U16) == _lib.SMM_ERR_UNSUPPORTED, plain
        assert call(plain + "_cf", raw, _lib.SMM_I16, None) == _lib.SMM_ERR_INVALID    # integer dtype without cf
        assert call(plain + "_cf", flt, _lib.SMM_F32, ctypes.byref(st)) == _lib.SMM_ERR_INVALID   # cf with a float dtype
        assert call(plain + "_cf", flt, _lib.SMM_F32, None) == _lib.SMM_OK             # cf NULL + float: the plain entry
        assert call(plain + "_cf", raw, _lib.SMM_I16, ctypes.byref(st)) == _lib.SMM_OK
    bits_equal(y.to_host(), want, "smm_group_apply_cf")
    bits_equal(ys.to_host().reshape(want.shape), want, "smm_group_apply_sb_cf")
    bits_equal(out, want, "smm_group_apply_host_cf")
    # an injected chunk failure on the packed group pipeline surfaces as SMM_ERR_HIP; the next call succeeds
    for flags in (0, _lib.APPLY_HOST_NO_PACK):
        _lib.call("smm_debug_fail_at_chunk", 0)
        try:
            with pytest.raises(_lib.SmmError) as e:
                grp.apply_host(q, lev, ml, masked=True, remap_area_min=0.5, cf=cf, flags=flags)
            assert e.value.code == _lib.SMM_ERR_HIP and "injected failure" in str(e.value)
        finally:
            _lib.call("smm_debug_fail_at_chunk", -1)
        bits_equal(grp.apply_host(q, lev, ml, masked=True, remap_area_min=0.5, cf=cf, flags=flags), want, "after the failure")
    _lib.call("smm_debug_staging_faults", 0, 0)
    try:
        with pytest.raises(_lib.SmmError) as e:
            grp.apply_host(q, lev, ml, masked=True, remap_area_min=0.5, cf=cf)
        assert e.value.code == _lib.SMM_ERR_ALLOC
    finally:
        _lib.call("smm_debug_staging_faults", 0, -1)
    bits_equal(grp.apply_host(q, lev, ml, masked=True, remap_area_min=0.5, cf=cf), want, "after the staging fault")


# ---------------------------------------------------------------- 7: Regridder

def _ocean_da(rng, deep, nt=5, name="so"):
    g = gridgen.parse_grid(f"r{NX}x{NY}")
    levels = np.array([5.0, 50.0, 200.0, 500.0, 1000.0, 2000.0])
    masks = gridgen.synthetic_ocean_masks(NX, NY, len(levels), top=0.95, bottom=0.3 if deep else 0.6)
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    q = raw_levels(rng, np.int16, nt, np.arange(len(levels)), 1, masks, cf.fill_values).reshape(nt, len(levels), NY, NX)
    coords = {"time": np.arange(nt), "lev": levels, "lat": g.lat, "lon": g.lon}
    attrs = {"scale_factor": 1.0e-3, "add_offset": 20.0, "_FillValue": np.int16(-32768), "units": "psu"}
    da = DataArray(q, dims=("time", "lev", "lat", "lon"), coords=coords, name=name, attrs=attrs)
    dec = DataArray(cf.decode(q), dims=da.dims, coords=coords, name=name, attrs={"units": "psu"})
    return da, dec, cf


def _same_array(got, want, what):
    assert got.dims == want.dims and got.values.dtype == want.values.dtype, what
    bits_equal(np.asarray(got.values), np.asarray(want.values), what)
    assert got.attrs == want.attrs, what
    assert list(got.coords) == list(want.coords), what
    for k in got.coords:
        assert np.array_equal(got.coords[k].values, want.coords[k].values), (what, k)


def _host_decode_lines(caplog):
    return sum("decoded on the host" in r.getMessage() for r in caplog.records)


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("transpose", [True, False])
def test_regridder_packed_levels_equals_decoded(hip, caplog, skipna, transpose):
    rng = np.random.default_rng(139)
    da, dec, cf = _ocean_da(rng, deep=skipna)
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    kw = dict(weights=w3, skipna=skipna, transpose=transpose)
    want = Regridder(**kw).regrid(dec)
    nan_share_ok(want.values, f"regridder skipna={skipna}")
    rg = Regridder(packed=True, packed_levels=True, loglevel="INFO", **kw)
    with caplog.at_level("INFO"):
        _same_array(rg.regrid(da), want, "host DataArray")
        dev = DataArray(to_device(da.data), dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs)
        _same_array(rg.regrid(dev), want, "DeviceArray")
        sb = DataArray(to_device(np.ascontiguousarray(da.data.transpose(1, 2, 3, 0)), layout="sb"),
                       dims=("lev", "lat", "lon", "time"), coords=da.coords, name=da.name, attrs=da.attrs)
        sbx = DataArray(to_device(np.ascontiguousarray(dec.data.transpose(1, 2, 3, 0)), layout="sb"),
                        dims=sb.dims, coords=dec.coords, name=dec.name, attrs=dec.attrs)
        _same_array(rg.regrid(sb), Regridder(**kw).regrid(sbx), "batch-fastest DeviceArray")
        lazy = Regridder(packed=True, packed_levels=True, lazy=True, loglevel="INFO", **kw).regrid(da)
        _same_array(lazy, want, "lazy")
    assert _host_decode_lines(caplog) == 0
    assert want.attrs == {"units": "psu"}
    caplog.clear()
    # float32 results: the fallback, in both settings; one line each
    want32 = Regridder(out_dtype=np.float32, **kw).regrid(dec)
    for levels_on in (True, False):
        with caplog.at_level("INFO"):
            got32 = Regridder(packed=True, packed_levels=levels_on, out_dtype=np.float32, loglevel="INFO", **kw).regrid(da)
        assert _host_decode_lines(caplog) == 1
        caplog.clear()
        _same_array(got32, want32, "float32")
    # the default: packed=True alone still decodes 3-D variables on the host, one line
    with caplog.at_level("INFO"):
        got = Regridder(packed=True, loglevel="INFO", **kw).regrid(da)
    assert _host_decode_lines(caplog) == 1
    _same_array(got, want, "packed_levels=False")


def test_regridder_dataset_mixing_levels_packed_2d_and_float(hip, caplog):
    """A Dataset with a packed variable on all levels, a packed surface variable and a float variable: every variable
    equals its decoded twin; nothing is decoded on the host.  The surface variable keeps a `lev` axis of length one
    (selected with a slice): a Regridder built from weights serves one grid type, so a variable without the mask
    dimension cannot share a Dataset with the 3-D ones (regrid() refuses it); packed 2-D variables on 2-D weights are
    what test_gpu_packed.py covers."""
    rng = np.random.default_rng(149)
    da, dec, cf = _ocean_da(rng, deep=False)
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    other = DataArray(35.0 + rng.standard_normal(dec.data.shape), dims=da.dims, coords=da.coords, name="thetao",
                      attrs={"units": "degC"})
    other.data[np.isnan(dec.data)] = np.nan
    top = DataArray(np.ascontiguousarray(da.data[:, :1]), dims=da.dims, name="sos", attrs=dict(da.attrs),
                    coords={**da.coords, "lev": da.coords["lev"].values[:1]})
    top_dec = DataArray(np.ascontiguousarray(dec.data[:, :1]), dims=da.dims, name="sos", attrs=dict(dec.attrs),
                        coords=dict(top.coords))
    plain = Regridder(weights=w3)
    with caplog.at_level("INFO"):
        out = Regridder(weights=w3, packed=True, packed_levels=True, loglevel="INFO").regrid(
            Dataset({"so": da, "sos": top, "thetao": other}, coords=dict(da.coords)))
    assert _host_decode_lines(caplog) == 0
    nan_share_ok(plain.regrid(dec).values, "dataset")
    _same_array(out["so"], plain.regrid(dec), "packed 3-D variable")
    _same_array(out["sos"], plain.regrid(top_dec), "packed single-level variable")
    _same_array(out["thetao"], plain.regrid(other), "float variable")
    assert not set(PACKING) & set(out["so"].attrs) and out["thetao"].attrs == {"units": "degC"}


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


def test_regridder_dask_backed_field(hip, caplog):
    from smmregrid_amd.lazy import is_dask
    rng = np.random.default_rng(151)
    da, dec, cf = _ocean_da(rng, deep=False)
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    want = Regridder(weights=w3).regrid(dec)
    nan_share_ok(want.values, "dask")
    for lazy in (False, True):
        backed = _DaskLike(da.data)
        assert is_dask(backed)
        lazy_in = DataArray(backed, dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs)
        with caplog.at_level("INFO"):
            got = Regridder(weights=w3, packed=True, packed_levels=True, lazy=lazy, loglevel="INFO").regrid(lazy_in)
            bits_equal(np.asarray(got.values), want.values, f"dask-backed, lazy={lazy}")
        assert _host_decode_lines(caplog) == 0 and backed.computed >= 1
        assert got.attrs == want.attrs and got.dims == want.dims
