"""`gradients=True` on the device: smm_gradients against `GradientRule.gradients`, smm_apply_cols against the "stacked"
statement of include/smmregrid_amd.h -- the existing apply on an operator of K * S source cells, link (d, s, k) at
s * K + k, and the field X[b, s * K + k] -- through the C oracle and through an existing SparseOperator, the parity of
the columns, every refusal, and the Regridder end to end.  Comparisons are bit equality unless said otherwise."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (CdoGenerate, DataArray, DeviceArray, GradientRule, Regridder, SparseOperator, _lib, gridgen,
                           to_device)
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu
SELL = _lib.APPLY_KERNEL_SELL


# ------------------------------------------------------------------ smm_gradients

GRIDS = {"36x19 periodic": (36, 19, True, 0), "37x5 regional, padded rows": (37, 5, False, 3),
         "130x3": (130, 3, True, 0), "2x2": (2, 2, True, 0), "1x4": (1, 4, True, 1), "300x40 regional": (300, 40, False, 0)}


def grid_rule(nx, ny, periodic, num_wgts, descending=False):
    lon = np.radians((np.arange(nx) + 0.5) * (360.0 if periodic else 70.0) / nx)
    lat = np.radians(-90.0 + (np.arange(ny) + 0.5) * 180.0 / ny)
    lat[0], lat[-1] = (-np.pi / 2, np.pi / 2) if ny > 2 else (lat[0], lat[-1])      # pole rows: ci = 0 (sphere kind)
    return GradientRule(lon, lat[::-1] if descending else lat, num_wgts)


def rough_field(rng, n_batch, nx, ny, dtype):
    x = (250.0 + 30.0 * rng.standard_normal((n_batch, ny, nx))).astype(dtype)
    bad = rng.random(x.shape) < 0.06
    x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=int(bad.sum()))
    if ny > 2:
        x[0, 1, :] = np.nan                       # a whole NaN row
        x[-1, 0, :] = np.nan                      # a NaN pole row
    return x.reshape(n_batch, -1)


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("num_wgts", [3, 4])
@pytest.mark.parametrize("grid", list(GRIDS))
def test_gradients_match_the_rule(hip, rng, grid, num_wgts, dtype):
    nx, ny, periodic, pad = GRIDS[grid]
    S = nx * ny
    op = SparseOperator(S, 1, np.array([1], np.int32), np.array([1], np.int32), np.array([1.0]), device=0)
    for descending in (False, True):
        rule = grid_rule(nx, ny, periodic, num_wgts, descending)
        assert rule.periodic == periodic
        for n_batch in (1, 3, 5):
            x = rough_field(rng, n_batch, nx, ny, dtype)
            xp = np.full((n_batch, S + pad), 7.0, dtype=dtype)      # ldx > S: the pad is never read into a plane
            xp[:, :S] = x
            got = op.gradients(to_device(xp), rule).to_host()
            ref = rule.gradients_rows(x)
            assert got.shape == (n_batch, rule.n_planes, S)
            assert np.isfinite(ref).all()
            bits_equal(got, ref)


def test_gradients_are_cut_along_the_batch_beyond_the_grid_limit(hip, rng):
    rule = grid_rule(36, 19, True, 4)
    op = SparseOperator(rule.size, 1, np.array([1], np.int32), np.array([1], np.int32), np.array([1.0]), device=0)
    x = rough_field(rng, 7, 36, 19, np.float64)
    _lib.call("smm_debug_set_grid_limit", 3)                     # one row needs one workgroup here: three rows a launch
    try:
        got = op.gradients(to_device(x), rule).to_host()
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    bits_equal(got, rule.gradients_rows(x))


# ------------------------------------------------------------------ smm_apply_cols

def stacked_links(src, dst, w):
    """Link (d, s, k) of an operator with K columns at source index s * K + k of one with K * S source cells."""
    K = w.shape[1]
    s = ((np.asarray(src, dtype=np.int64) - 1)[:, None] * K + np.arange(K)[None, :] + 1).astype(np.int32)
    return s.ravel(), np.repeat(np.asarray(dst, dtype=np.int32), K), np.ascontiguousarray(w).ravel()


class Case:
    """An operator with columns, its rule, and the stacked statement: the C oracle's CSR and an existing SparseOperator."""

    def __init__(self, src, dst, w, rule, n_dst, imask=None, frac=None):
        self.rule, self.S, self.D, self.K = rule, rule.size, n_dst, w.shape[1]
        self.op = SparseOperator(self.S, n_dst, src, dst, w, device=0, columns=True)
        self.op0 = SparseOperator(self.S, n_dst, src, dst, w, device=0)
        ss, sd, sw = stacked_links(src, dst, w)
        self.csr = oracle.coo_to_csr_c(self.S * self.K, n_dst, ss, sd, sw)
        self.op_s = SparseOperator(self.S * self.K, n_dst, ss, sd, sw, device=0)
        self.imask, self.frac = imask, frac
        for o in (self.op, self.op0, self.op_s):
            o.set_epilogue(imask, frac)

    def ref(self, x, masked=False, area_min=0.0):
        X = self.rule.stacked(x)
        y = oracle.apply_c(self.csr, X, masked=masked, dst_imask=self.imask, dst_frac=self.frac, area_min=area_min)
        for flags in (0, SELL):      # the existing apply on the stacked operator says the same
            y_s = self.op_s.apply(to_device(X), masked=masked, remap_area_min=area_min, flags=flags).to_host()
            bits_equal(y_s, y)
        return y


def gridgen_case(rng, method, src, dst):
    w = gridgen.generate_weights(src, dst, method=method)
    D = w.sizes["dst_grid_size"]
    imask = (rng.random(D) > 0.2).astype(np.int32)
    frac = rng.random(D)
    return Case(w["src_address"].values, w["dst_address"].values, w["remap_matrix"].values,
                GradientRule.from_weights(w), D, imask, frac)


@pytest.fixture(scope="module")
def cases(hip):
    rng = np.random.default_rng(20261020)
    return {"bic": gridgen_case(rng, "bic", "r36x19", "r20x10"), "con2": gridgen_case(rng, "con2", "r36x18", "r24x12")}


def smooth_field(rng, n_batch, S, dtype, nan_frac=0.0):
    x = (250.0 + 30.0 * rng.standard_normal((n_batch, S))).astype(dtype)
    if nan_frac:
        x[rng.random(x.shape) < nan_frac] = np.nan
    return x


@pytest.mark.parametrize("dtype", [np.float32, np.float64])
@pytest.mark.parametrize("n_batch", [1, 3, 5, 9])
@pytest.mark.parametrize("name", ["bic", "con2"])
def test_apply_cols_equals_the_stacked_statement(cases, rng, name, n_batch, dtype):
    c = cases[name]
    assert c.op.n_cols == c.K == c.rule.n_planes + 1
    x = smooth_field(rng, n_batch, c.S, dtype)
    for masked, area_min in ((False, 0.0), (True, 0.0), (False, 0.5), (True, 0.3)):
        got = c.op.apply(to_device(x), masked=masked, remap_area_min=area_min, gradients=c.rule).to_host()
        ref = c.ref(x, masked, area_min)
        bits_equal(got, ref)
        assert np.isnan(ref).any() == (masked or area_min > 0)
    # column 0 of the operator is the operator without columns: every existing entry sees that alone
    bits_equal(c.op.apply(to_device(x)).to_host(), c.op0.apply(to_device(x)).to_host())


def raw_apply_cols(op, rule, x, scratch_bytes, flags=0, area_min=0.0):
    """smm_apply_cols as the library answers it: (status, message)."""
    y = DeviceArray((x.shape[0], op.n_dst), np.float64)
    scratch = DeviceArray((max(scratch_bytes, 8),), np.uint8)
    rc = _lib.load().smm_apply_cols(op.handle, rule.plan(0), ctypes.c_void_p(x.ptr), _lib.SMM_F64, x.shape[1],
                                    ctypes.c_void_p(y.ptr), _lib.SMM_F64, op.n_dst, x.shape[0], area_min, flags,
                                    ctypes.c_void_p(scratch.ptr), scratch_bytes, None)
    _lib.call("smm_device_sync")
    return rc, (_lib.load().smm_last_error() or b"").decode()


@pytest.mark.parametrize("name", ["bic", "con2"])
def test_scratch_for_two_rows_walks_five_in_three_rounds(cases, rng, name):
    c = cases[name]
    x = smooth_field(rng, 5, c.S, np.float64)
    whole = c.op.apply(to_device(x), gradients=c.rule).to_host()
    for rows in (2, 1, 4):
        bits_equal(c.op.apply(to_device(x), gradients=c.rule, scratch_rows=rows).to_host(), whole)
    bits_equal(whole, c.ref(x))
    need = ctypes.c_size_t(0)
    _lib.call("smm_apply_cols_scratch", c.op.handle, 5, ctypes.byref(need))
    assert need.value == 5 * c.rule.n_planes * c.S * 8
    rc, msg = raw_apply_cols(c.op, c.rule, to_device(x), scratch_bytes=c.rule.n_planes * c.S * 8 - 8)
    assert rc == _lib.SMM_ERR_INVALID and "one batch row" in msg      # not even one row's planes fit


def test_nan_footprint_is_the_footprint_of_column_0(cases, rng):
    for name, c in cases.items():
        x = smooth_field(rng, 4, c.S, np.float32, nan_frac=0.03)
        x[2, 5] = np.inf
        got = c.op.apply(to_device(x), gradients=c.rule).to_host()
        col0 = c.op0.apply(to_device(x), flags=SELL).to_host()
        bits_equal(got, c.ref(x))
        assert np.array_equal(np.isnan(got), np.isnan(col0)) and np.isnan(got).any() and not np.isnan(got).all()


def test_duplicate_links_a_row_without_links_and_pruning(hip, rng):
    nx, ny, D = 12, 7, 150
    rule = grid_rule(nx, ny, True, 4)
    S = rule.size
    n = 1400
    src = rng.integers(1, S + 1, size=n).astype(np.int32)
    dst = rng.integers(1, D + 1, size=n).astype(np.int32)
    dst[dst == 17] = 18                                        # row 16 (0-based) has no link
    dst[dst == 130] = 129                                      # ... and one in the last slice
    pick = rng.integers(0, n, size=300)
    src[:300], dst[:300] = src[pick], dst[pick]                # duplicates, summed in link order
    w = rng.uniform(-0.5, 1.5, size=(n, 4))
    w[rng.random(n) < 0.1] = 0.0                               # links whose columns are all zero
    w[rng.random(n) < 0.1, 0] = 0.0                            # ... and whose column 0 alone is
    perm = rng.permutation(n)
    src, dst, w = src[perm], dst[perm], w[perm]
    c = Case(src, dst, w, rule, D)
    # export_cols equals the host statement: the stacked CSR, de-interleaved
    rowptr, col, val = c.op.export_csr()
    cols = c.op.export_cols()
    s_rowptr, s_col, s_val = c.csr
    assert cols.shape == (c.op.nnz, 4) and np.array_equal(rowptr * 4, s_rowptr)
    assert np.array_equal(np.repeat(col.astype(np.int64) * 4, 4) + np.tile(np.arange(4), col.size), s_col)
    bits_equal(cols.ravel(), s_val)
    bits_equal(cols[:, 0], val)
    bits_equal(val, c.op0.export_csr()[2])
    x = smooth_field(rng, 6, S, np.float64, nan_frac=0.02)
    got = c.op.apply(to_device(x), gradients=rule).to_host()
    bits_equal(got, c.ref(x))
    assert (got[:, 16] == 0.0).all() and (got[:, 129] == 0.0).all()
    pruned = SparseOperator(S, D, src, dst, w, device=0, columns=True, prune_zeros=True)
    keep = (cols != 0.0).any(axis=1)
    assert pruned.nnz == int(keep.sum()) < c.op.nnz
    bits_equal(pruned.export_cols(), cols[keep])
    assert (pruned.export_cols()[:, 0] == 0.0).any()
    bits_equal(pruned.apply(to_device(x), gradients=rule).to_host(), got)


def test_every_refusal_returns_its_status(cases, rng):
    c = cases["bic"]
    x = to_device(smooth_field(rng, 2, c.S, np.float64))

    def code(fn):
        with pytest.raises(_lib.SmmError) as err:
            fn()
        assert str(err.value)
        return err.value.code

    U, I = _lib.SMM_ERR_UNSUPPORTED, _lib.SMM_ERR_INVALID
    assert code(lambda: c.op.apply(x, gradients=c.rule, skipna=True)) == U
    assert code(lambda: c.op.apply(x, gradients=c.rule, flags=_lib.APPLY_KERNEL_TILE)) == U
    for fl in (_lib.APPLY_SB_PACKED, _lib.APPLY_SB_Y_SB, _lib.APPLY_HOST_NO_PACK):
        assert code(lambda: c.op.apply(x, gradients=c.rule, flags=fl)) == U
    for dt in (np.float16, np.float32):
        assert code(lambda: c.op.apply(x, gradients=c.rule, out_dtype=dt)) == U
    half = DeviceArray((2, c.S), np.float16)
    assert code(lambda: c.op.apply(half, gradients=c.rule)) == U
    assert code(lambda: c.op.gradients(half, c.rule)) == U
    # handles that do not fit each other
    assert code(lambda: c.op0.apply(x, gradients=c.rule)) == I                     # an operator without columns
    assert code(lambda: c.op.apply(x, gradients=GradientRule(c.rule.lon, c.rule.lat, 3))) == I      # 2 planes, 4 columns
    with pytest.raises(ValueError, match="cells"):
        c.op.apply(x, gradients=cases["con2"].rule)                                # another grid
    whole = c.rule.n_planes * c.S * 8 * 2
    rc, msg = raw_apply_cols(c.op, grid_rule(20, 30, True, 4), x, whole)           # the library's own check of the grid
    assert rc == I and "600 cells" in msg
    assert raw_apply_cols(c.op, c.rule, x, whole, area_min=2.0)[0] == I
    assert raw_apply_cols(c.op, c.rule, x, whole)[0] == _lib.SMM_OK
    for kw in (dict(cf=object()), dict(cf_out=object()), dict(keep_batch_fastest=True)):
        with pytest.raises(ValueError, match="gradients="):
            c.op.apply(x, gradients=c.rule, **kw)
    with pytest.raises(ValueError, match="gradients="):
        c.op.apply(DeviceArray((c.S, 2), np.float64, layout="sb"), gradients=c.rule)
    # the flags that are built
    ref = c.ref(x.to_host())
    for fl in (SELL, _lib.APPLY_NO_FILL):
        bits_equal(c.op.apply(x, gradients=c.rule, flags=fl).to_host(), ref)


# ------------------------------------------------------------------ end to end

@pytest.fixture(scope="module")
def facade(hip):
    w = CdoGenerate("r36x19", "r20x10").weights(method="bic")
    sg, dg = gridgen.parse_grid("r36x19"), gridgen.parse_grid("r20x10")
    rule = GradientRule.from_weights(w)
    ss, sd, sw = stacked_links(w["src_address"].values, w["dst_address"].values, w["remap_matrix"].values)
    csr = oracle.coo_to_csr_c(rule.size * 4, w.sizes["dst_grid_size"], ss, sd, sw)
    return w, sg, dg, rule, csr


def as_field(x, sg):
    return DataArray(x, dims=("time", "lat", "lon"), coords={"time": np.arange(x.shape[0]), "lat": sg.lat, "lon": sg.lon},
                     name="tas")


def test_regridder_equals_the_stacked_statement(facade, rng):
    w, sg, dg, rule, csr = facade
    x = 250.0 + 30.0 * rng.standard_normal((5, 19, 36))
    x[1, 4, 7:9] = np.nan
    rg = Regridder(weights=w, gradients=True, device=0)
    masked = bool(oracle.check_mask(rg.grids[0].weights["dst_grid_imask"].values))
    ref = oracle.apply_c(csr, rule.stacked(x.reshape(5, -1)), masked=masked,
                         dst_imask=rg.grids[0].weights["dst_grid_imask"].values,
                         dst_frac=w["dst_grid_frac"].values, area_min=0.5).reshape(5, 10, 20)
    host = rg.regrid(as_field(x, sg))
    assert host.shape == (5, 10, 20)
    bits_equal(np.asarray(host.values), ref)
    dev = rg.regrid(as_field(to_device(x), sg))
    assert isinstance(dev.data, DeviceArray)
    bits_equal(dev.data.to_host(), ref)
    lazy = Regridder(weights=w, gradients=True, device=0, lazy=True).regrid(as_field(x, sg))
    assert not isinstance(lazy.data, np.ndarray)
    bits_equal(np.asarray(lazy.values), ref)
    f32 = rg.regrid(as_field(x.astype(np.float32), sg))
    ref32 = oracle.apply_c(csr, rule.stacked(x.astype(np.float32).reshape(5, -1)), masked=masked,
                           dst_imask=rg.grids[0].weights["dst_grid_imask"].values,
                           dst_frac=w["dst_grid_frac"].values, area_min=0.5).reshape(5, 10, 20)
    assert f32.values.dtype == np.float64
    bits_equal(np.asarray(f32.values), ref32)
    with pytest.raises(ValueError, match="batch-fastest"):
        rg.regrid(DataArray(DeviceArray((19, 36, 5), np.float64, layout="sb"), dims=("lat", "lon", "time"),
                            coords={"lat": sg.lat, "lon": sg.lon, "time": np.arange(5)}, name="tas"))


def test_regridder_reproduces_a_field_linear_in_latitude(facade):
    w, sg, dg, rule, csr = facade
    lon, lat = np.meshgrid(sg.lon, sg.lat)
    dlon, dlat = dg.centers()
    interior = ((dlat > sg.lat[1]) & (dlat < sg.lat[-2])).reshape(10, 20)
    assert interior.sum() == 160
    f = (3.0 + 0.25 * lat)[None]
    exact = (3.0 + 0.25 * dlat).reshape(10, 20)
    got = np.asarray(Regridder(weights=w, gradients=True, device=0).regrid(as_field(f, sg)).values)[0]
    plain = np.asarray(Regridder(weights=w, device=0).regrid(as_field(f, sg)).values)[0]
    err, err0 = np.abs(got - exact)[interior].max(), np.abs(plain - exact)[interior].max()
    print(f"all columns {err:.3e}, column 0 alone {err0:.3e}")
    assert err <= 32 * np.spacing(np.abs(f).max()) and err0 > 0.1


def test_without_the_keyword_the_result_is_todays(facade, rng):
    w, sg, dg, rule, csr = facade
    x = 250.0 + 30.0 * rng.standard_normal((3, 19, 36))
    rg = Regridder(weights=w, device=0)
    assert rg.grids[0].weights_matrix.n_cols == 1
    c0 = oracle.coo_to_csr_c(rule.size, w.sizes["dst_grid_size"], w["src_address"].values, w["dst_address"].values,
                             w["remap_matrix"].values)
    masked = bool(oracle.check_mask(rg.grids[0].weights["dst_grid_imask"].values))
    ref = oracle.apply_c(c0, x.reshape(3, -1), masked=masked, dst_imask=rg.grids[0].weights["dst_grid_imask"].values,
                         dst_frac=w["dst_grid_frac"].values, area_min=0.5).reshape(3, 10, 20)
    bits_equal(np.asarray(rg.regrid(as_field(x, sg)).values), ref)
    # ... and an operator with columns gives that result too through every existing entry
    op = Regridder(weights=w, gradients=True, device=0).grids[0].weights_matrix
    assert op.n_cols == 4
    bits_equal(np.array(op.apply_host(x.reshape(3, -1), masked=masked, remap_area_min=0.5)).reshape(3, 10, 20), ref)


def test_apply_host_in_three_chunks_equals_one(cases, rng):
    c = cases["con2"]
    x = smooth_field(rng, 7, c.S, np.float32, nan_frac=0.01)
    one = np.array(c.op.apply_host(x, gradients=c.rule, masked=True, remap_area_min=0.3))
    three = np.array(c.op.apply_host(x, gradients=c.rule, masked=True, remap_area_min=0.3, chunk_rows=3))
    bits_equal(one, three)
    bits_equal(one, c.ref(x, True, 0.3))
