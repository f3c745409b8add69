"""smm_apply_mode on the device -- `SparseOperator.apply_mode`, `apply_mode_host`, `Regridder(categorical=...)` -- against
`categorical.ModeRule`, bit for bit, y and share.  The inputs are those of tests/mode_cases.py (tests/test_mode_rule.py
checks on the CPU that each holds a tie, a missing link, every kind of dead row and a winner that is not the heaviest
link).  The row pitches of X, Y and the share are padded, and the pads must come back untouched."""
import ctypes
import functools

import numpy as np
import pytest

from smmregrid_amd import DeviceArray, ModeRule, Regridder, SparseOperator, _lib, gridgen, to_device
from smmregrid_amd.xrlite import DataArray, Dataset
from tests import far_cases as fc
from tests import mode_cases as mc
from tests.test_gpu_far_offsets import F64, U16, Far, far      # noqa: F401  (far: the fixture)

pytestmark = pytest.mark.gpu

SEED = 5
SHAPES = tuple(zip((1, 63, 64, 65, 255, 256, 257, 600), (9, 1, 2, 3, 4, 5, 9, 2), ("u16", "f32", "i16", "f64") * 2))
VALUES = tuple((kind, n_classes, n_fill) for kind in mc.DTYPES
               for n_classes, n_fill in ((1, 1), (2, 0), (2, 1), (5, 2), ("own", 1)))
SENTINEL = 0x42


def host_cases():
    """(D, B, kind, field keywords) of every generated case below: tests/test_mode_rule.py counts what each covers."""
    for D, B, kind in SHAPES:
        yield D, B, kind, dict(n_classes=5, n_fill=1, seed=SEED, pitch=7)
    for kind, n_classes, n_fill in VALUES:
        yield 65, 2, kind, dict(n_classes=n_classes, n_fill=n_fill, seed=SEED, pitch=3)
    for kind in mc.DTYPES:
        yield 257, 3, kind, dict(n_classes=5, n_fill=2, seed=SEED, pitch=7)


@functools.lru_cache(maxsize=None)
def device_operator(D, long_rows=()):
    case = mc.operator(D, seed=SEED, long_rows=dict(long_rows))
    op = SparseOperator(case.n_src, D, case.src, case.dst, case.w, device=0)
    op.set_epilogue(case.imask, case.frac)
    rowptr, col, val = op.export_csr()
    assert np.array_equal(rowptr, case.csr[0]) and np.array_equal(col, case.csr[1])
    assert mc.bits(val).tolist() == mc.bits(case.csr[2]).tolist()
    return case, op


def padded(shape, dtype, pad):
    """A DeviceArray (B, D + pad) filled with the sentinel byte."""
    return DeviceArray((shape[0], shape[1] + pad), dtype).fill_bytes(SENTINEL)


def run(op, case, x, rule, masked, area_min, flags=0):
    """apply_mode into padded Y and share; the pads are checked; (y, share) of the true columns."""
    B, D = x.shape[0], case.n_dst
    Y, SH = padded((B, D), x.dtype, 5), padded((B, D), np.float64, 3)
    got = op.apply_mode(to_device(x), y=Y, masked=masked, remap_area_min=area_min, fill=rule.fill, fill_out=rule.fill_out,
                        share=SH, flags=flags)
    assert got[0] is Y and got[1] is SH
    y, sh = Y.to_host(), SH.to_host()
    assert (y[:, D:].view(np.uint8) == SENTINEL).all() and (sh[:, D:].view(np.uint8) == SENTINEL).all()
    return np.ascontiguousarray(y[:, :D]), np.ascontiguousarray(sh[:, :D])


def check(case, op, x, rule, masked, area_min, what, flags=0):
    want_y, want_sh = rule.apply(case.csr, x, masked=masked, dst_imask=case.imask, dst_frac=case.frac,
                                 remap_area_min=area_min)
    y, sh = run(op, case, x, rule, masked, area_min, flags)
    mc.assert_bits(y, want_y, f"{what}: y")
    mc.assert_bits(sh, want_sh, f"{what}: share")
    return y, sh


@pytest.mark.parametrize("D, B, kind", SHAPES)
def test_shapes_and_row_lengths(hip, D, B, kind):
    """Every D and B of the list, rows of 0 .. 65 links.  The slices take turns (tests/mode_cases.py): rows up to 17 links,
    up to 64 -- the capacity of the 4-byte types to the slot, past that of float64 -- and up to 65, past every capacity:
    from D = 255 on both forms run in one launch."""
    case, op = device_operator(D)
    x, rule = mc.field(case, B, kind, n_classes=5, n_fill=1, seed=SEED, pitch=7)
    info = op.mode_launch_info(x.dtype)
    assert info["capacity"] == (32 if kind == "f64" else 64) and info["lds_slots"] == min(info["capacity"], op.max_row_nnz)
    assert info["lds_slices"] >= 1 and (D < 255 or info["global_slices"] >= 1)
    for masked, area_min in ((False, 0.0), (True, 0.3)):
        check(case, op, x, rule, masked, area_min, f"D={D} B={B} {kind} masked={masked} area_min={area_min}")


@pytest.mark.parametrize("kind, n_classes, n_fill", VALUES)
def test_fields_of_one_two_five_and_all_distinct_classes(hip, kind, n_classes, n_fill):
    case, op = device_operator(65)
    x, rule = mc.field(case, 2, kind, n_classes=n_classes, n_fill=n_fill, seed=SEED, pitch=3)
    check(case, op, x, rule, True, 0.3, f"{kind} {n_classes} classes, {n_fill} fills")
    check(case, op, x, rule, False, 0.0, f"{kind} {n_classes} classes, {n_fill} fills, plain",
          flags=_lib.APPLY_KERNEL_SELL)


@pytest.mark.parametrize("kind", mc.DTYPES)
def test_mask_and_area_threshold_and_the_hand_over_between_the_two_forms(hip, kind):
    """D = 257: slice 1 is ragged -- one row past the capacity among shorter ones --, slice 2 lies past it as a whole,
    slices 0 and 3 are short and slice 4 is one row.  The capacity is asked of the library."""
    cap = device_operator(1)[1].mode_launch_info(mc.DTYPES[kind])["capacity"]
    long_rows = {70: cap + 5, **{d: cap + 1 + d % 3 for d in range(128, 192)}}
    case, op = device_operator(257, tuple(sorted(long_rows.items())))
    rowlen = np.diff(case.csr[0])
    assert rowlen[70] > cap and (np.delete(rowlen[64:128], 6) <= 64).all() and (rowlen[128:192] > cap).all()
    assert (rowlen[:64] <= 17).all() and (rowlen[192:256] <= 17).all()
    info = op.mode_launch_info(mc.DTYPES[kind])
    assert info["lds_slots"] == cap and info["global_slices"] >= 2 and info["lds_slices"] >= 2 and info["lds_slices"] + info["global_slices"] == 5
    assert info["lds_bytes"] == 4 * cap * 64 * (8 if kind == "f64" else 4) <= 64 << 10
    x, rule = mc.field(case, 3, kind, n_classes=5, n_fill=2, seed=SEED, pitch=7)
    for masked in (False, True):
        for area_min in mc.AREA_MINS:
            check(case, op, x, rule, masked, area_min, f"{kind} masked={masked} area_min={area_min}")


def test_the_share_is_the_existing_sell_apply_on_the_winners_indicator_field(hip):
    case, op = device_operator(257)
    x, rule = mc.field(case, 3, "u16", n_classes=5, n_fill=1, seed=SEED)
    y, sh = run(op, case, x, rule, False, 0.0)
    alive = sh > 0
    assert alive.sum() > 500
    seen = 0
    for c in np.unique(y[alive]):
        ind = ((x == c) & ~rule.missing(x)).astype(np.float64)
        plain = op.apply(to_device(ind), flags=_lib.APPLY_KERNEL_SELL).to_host()
        won = alive & (y == c)
        mc.assert_bits(sh[won], plain[won], f"class {c}")
        seen += int(won.sum())
    assert seen == alive.sum()


def test_a_launch_cut_by_the_grid_limit(hip):
    """D = 600 is three workgroups a batch row: a limit of 7 cuts the batch, a limit of 2 the destination blocks too."""
    case, op = device_operator(600)
    x, rule = mc.field(case, 5, "i16", n_classes=5, n_fill=1, seed=SEED, pitch=7)
    for limit in (7, 2, 1):
        _lib.call("smm_debug_set_grid_limit", limit)
        try:
            check(case, op, x, rule, True, 0.3, f"grid limit {limit}")
        finally:
            _lib.call("smm_debug_set_grid_limit", 0)


def test_refusals_that_need_an_operator(hip):
    case, op = device_operator(65)
    bare = SparseOperator(case.n_src, 65, case.src, case.dst, case.w, device=0)
    S, D = case.n_src, 65
    x, y, sh = DeviceArray((2, S), np.float32), DeviceArray((2, D), np.float32), DeviceArray((2, D), np.float64)
    vp = lambda a: ctypes.c_void_p(a.ptr)

    def status(handle=op.handle, ldx=S, ldy=D, ld_share=D, share=sh, area_min=0.0, flags=0, n_batch=2):
        rc = _lib.load().smm_apply_mode(handle, vp(x), _lib.SMM_F32, ldx, vp(y), ldy, None if share is None else vp(share),
                                        ld_share, n_batch, area_min, flags, None, None)
        return rc, (_lib.load().smm_last_error() or b"").decode()

    for kw, word in ((dict(ldx=S - 1), "ldx/ldy"), (dict(ldy=D - 1), "ldx/ldy"), (dict(ld_share=D - 1), "ld_share"),
                     (dict(handle=bare.handle, flags=_lib.APPLY_MASKED), "dst_imask"),
                     (dict(handle=bare.handle, area_min=0.3), "dst_frac"), (dict(area_min=1.5), "remap_area_min")):
        rc, msg = status(**kw)
        assert rc == _lib.SMM_ERR_INVALID and word in msg, (kw, rc, msg)
    assert status(ld_share=0, share=None)[0] == _lib.SMM_OK          # no share: its pitch is not looked at
    assert status(n_batch=0, ldx=0, ldy=0)[0] == _lib.SMM_OK
    with pytest.raises(TypeError, match="float32, float64, int16, uint16"):
        op.apply_mode(DeviceArray((2, S), np.float16))
    with pytest.raises(ValueError, match="batch-fastest"):
        op.apply_mode(DeviceArray((S, 2), np.float32, layout="sb"))
    with pytest.raises(ValueError, match="fill_out"):
        op.apply_mode(DeviceArray((2, S), np.int16))


def test_an_operator_with_weight_columns_works_through_its_column_0(hip):
    case, _ = device_operator(65)
    w = np.stack([case.w, case.w * 3.0 + 1.0, -case.w], axis=1)
    op = SparseOperator(case.n_src, 65, case.src, case.dst, w, device=0, columns=True)
    op.set_epilogue(case.imask, case.frac)
    assert op.n_cols == 3
    x, rule = mc.field(case, 2, "f32", seed=SEED)
    check(case, op, x, rule, True, 0.3, "columns=True")


# ------------------------------------------------------------------ offsets past 2^31 and 2^32 elements

@pytest.mark.parametrize("side", ["x", "y", "share"])
def test_far_rows_of_a_uint16_field_a_result_and_a_share(far, side):
    """5 rows on a pitch of 2^30 + K: `b * ldx`, `b * ldy` and `b * ld_share` cross 2^31 and 2^32 elements in the kernel,
    and with one batch row a launch `r0 * ldx` ... on the host."""
    D, B = 300, 5
    case, op = device_operator(D)
    x, rule = mc.field(case, B, "u16", n_classes=5, n_fill=1, seed=SEED)
    want_y, want_sh = rule.apply(case.csr, x, masked=True, dst_imask=case.imask, dst_frac=case.frac, remap_area_min=0.3)
    S = case.n_src
    lay = {k: fc.rows_layout(B, n) if k == side else (fc.near_layout(B, n), n) for k, n in (("x", S), ("y", D), ("share", D))}
    assert lay[side][1] > 1 << 30 and lay[side][0].crossed() == (3, 1)
    X, Y, SH = far.x(lay["x"][0], U16, x), far.y(lay["y"][0], U16), far.y(lay["share"][0], F64)
    struct = _lib.ModeRuleStruct(len(rule.fill), (ctypes.c_int32 * 2)(rule.fill[0], 0), rule.fill_out, 0)
    for limit in (0, 2):
        Y.arr.fill_bytes(fc.SENTINEL)
        SH.arr.fill_bytes(fc.SENTINEL)
        _lib.call("smm_debug_set_grid_limit", limit)
        try:
            _lib.call("smm_apply_mode", op.handle, X.ptr, _lib.SMM_U16, lay["x"][1], Y.ptr, lay["y"][1], SH.ptr,
                      lay["share"][1], B, 0.3, _lib.APPLY_MASKED, ctypes.byref(struct), None)
        finally:
            _lib.call("smm_debug_set_grid_limit", 0)
        Y.check(want_y, f"far {side}, grid limit {limit}: y")
        SH.check(want_sh, f"far {side}, grid limit {limit}: share")


# ------------------------------------------------------------------ host fields and the Regridder

def test_apply_mode_host_in_three_chunks_with_a_short_last_one(hip):
    case, op = device_operator(257)
    for kind, own in (("i16", np.int8), ("u16", np.uint8), ("f32", np.float32), ("u16", np.uint16)):
        x, _ = mc.field(case, 7, kind, n_classes=3, n_fill=0, seed=SEED)
        x = x.astype(own)                                     # classes 1, 2, 7 fit every type
        rule = ModeRule((2,), 0) if np.dtype(own).kind != "f" else ModeRule()
        want_y, want_sh = rule.apply(case.csr, x, masked=True, dst_imask=case.imask, dst_frac=case.frac, remap_area_min=0.3)
        y, sh = op.apply_mode_host(x, masked=True, remap_area_min=0.3, fill=rule.fill, fill_out=rule.fill_out, share=True,
                                   chunk_rows=3)
        mc.assert_bits(y, want_y, f"{np.dtype(own)} y")
        mc.assert_bits(sh, want_sh, f"{np.dtype(own)} share")
        whole = op.apply_mode_host(x, masked=True, remap_area_min=0.3, fill=rule.fill, fill_out=rule.fill_out)
        mc.assert_bits(whole, want_y, f"{np.dtype(own)} one chunk")
    for bad in (np.int32, np.int64, np.float16):
        with pytest.raises(TypeError, match="float32, float64, int16, uint16"):
            op.apply_mode_host(np.zeros((1, case.n_src), dtype=bad))
    with pytest.raises(ValueError, match="no value of uint8"):
        op.apply_mode_host(np.zeros((1, case.n_src), dtype=np.uint8), fill=(2,), fill_out=300)


def test_regridder_mixes_a_class_variable_and_a_temperature(hip, caplog):
    w = gridgen.generate_weights("r36x18", "r12x6", method="con")
    src = gridgen.parse_grid("r36x18")
    rng = np.random.default_rng(SEED)
    nt = 3
    lc = rng.integers(1, 6, size=(nt, 18, 36)).astype(np.uint8)
    lc[:, 4:9, 10:20] = 255
    tas = (280.0 + rng.standard_normal((nt, 18, 36))).astype(np.float32)
    tas[0, 2, 3] = np.nan
    coords = {"time": np.arange(nt), "lat": np.asarray(src.lat), "lon": np.asarray(src.lon)}
    attrs = {"flag_values": np.arange(1, 6, dtype=np.uint8), "flag_meanings": "a b c d e", "_FillValue": np.uint8(255)}
    ds = Dataset({"lc": DataArray(lc, dims=("time", "lat", "lon"), coords=coords, attrs=attrs, name="lc"),
                  "tas": DataArray(tas, dims=("time", "lat", "lon"), coords=coords, attrs={"units": "K"}, name="tas")})
    plain = Regridder(weights=w).regrid(ds)
    named = Regridder(weights=w, categorical=["lc"])
    out = named.regrid(ds)
    assert np.asarray(out["tas"].values).dtype == np.float64
    mc.assert_bits(np.asarray(out["tas"].values), np.asarray(plain["tas"].values), "tas beside a class variable")

    grid = named.grids[0]
    csr = grid.weights_matrix.export_csr()
    masked = bool(np.asarray(grid.masked).any())
    kw = dict(masked=masked, dst_imask=np.asarray(w["dst_grid_imask"].values), dst_frac=np.asarray(w["dst_grid_frac"].values),
              remap_area_min=0.5)
    want, _ = ModeRule((255,), 255).apply(csr, lc.reshape(nt, -1), **kw)
    got = np.asarray(out["lc"].values)
    assert got.dtype == np.uint8 and got.shape == (nt, 6, 12)
    mc.assert_bits(got.reshape(nt, -1), want, "lc")
    assert (got == 255).any() and (got != 255).any()
    assert out["lc"].attrs["flag_meanings"] == "a b c d e" and out["lc"].attrs["_FillValue"] == 255
    assert (np.asarray(plain["lc"].values) != got).any()      # the weighted sum of class codes is something else

    # categorical=True: every variable, the float32 one too (NaN is its missing value); device-resident fields as well
    every = Regridder(weights=w, categorical=True)
    out = every.regrid(ds)
    mc.assert_bits(np.asarray(out["lc"].values).reshape(nt, -1), want, "lc, categorical=True")
    want_t, _ = ModeRule().apply(csr, tas.reshape(nt, -1), **kw)
    assert np.asarray(out["tas"].values).dtype == np.float32
    mc.assert_bits(np.asarray(out["tas"].values).reshape(nt, -1), want_t, "tas as classes")
    dev = DataArray(to_device(lc.astype(np.int16)), dims=("time", "lat", "lon"), coords=coords, attrs={"_FillValue": 255},
                    name="lc")
    res = every.regrid(dev)
    assert isinstance(res.data, DeviceArray) and res.data.dtype == np.int16
    mc.assert_bits(res.data.to_host().reshape(nt, -1).astype(np.uint8), want, "device-resident lc")

    # without a fill attribute: one WARNING, and the dtype's edge stands for a dead cell
    bare = DataArray(lc.astype(np.int16), dims=("time", "lat", "lon"), coords=coords, name="lc")
    with caplog.at_level("WARNING", logger="smmregrid.Regrid"):
        caplog.clear()
        res = every.regrid(bare)
    assert sum("names no _FillValue" in r.getMessage() for r in caplog.records) == 1
    want_b, _ = ModeRule((-32768,), -32768).apply(csr, lc.astype(np.int16).reshape(nt, -1), **kw)
    mc.assert_bits(np.asarray(res.values).reshape(nt, -1), want_b, "no fill attribute")
    with pytest.raises(ValueError, match="batch-fastest"):
        every.regrid(DataArray(DeviceArray((18, 36, nt), np.float32, layout="sb"), dims=("lat", "lon", "time"),
                               coords=coords, name="lc"))
