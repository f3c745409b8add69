"""SMM_APPLY_SKIPNA (skipna=True): every kernel form against a numpy restatement of the rule in
include/smmregrid_amd.h, bit for bit; bit-identity with the plain apply where no link is invalid; equality with
weights regenerated from each step's validity; the facade, groups and the refusals."""
import os

import numpy as np
import pytest

from smmregrid_amd import DataArray, OperatorGroup, Regridder, SparseOperator, _lib, gridgen, to_device
from tests.helpers import bits_equal, field, kernel_forms, random_links, ragged_links, skipna_ref

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(__file__), "golden")
SK = _lib.APPLY_SKIPNA
T, S_ = _lib.APPLY_KERNEL_TILE, _lib.APPLY_KERNEL_SELL
REG, DMA = _lib.STAGING_REGISTERS, _lib.STAGING_DMA
# tile_split_rows=1: part-of-a-slice blocks without split rows (split rows have no skipna variant)
TILE_KNOBS = (dict(tile_staging=REG), dict(tile_staging=REG, tile_rows_per_step=1), dict(tile_staging=DMA),
              dict(tile_staging=DMA, tile_rows_per_step=2, tile_walk=3), dict(tile_staging=DMA, tile_rows_per_step=4),
              dict(tile_split_rows=1), dict(tile_split_rows=1, tile_staging=DMA))


def all_forms(op, x, masked, area_min, out_dtype):
    """Every path skipna runs through: the kernel forms, the batch-fastest kernel (whole and packed), the host
    pipeline (packed and whole rows)."""
    outs = {}
    dx = to_device(x)
    for flags, knobs in kernel_forms(*TILE_KNOBS):
        if flags == T and not op.plan_info()["tile_plan"]:
            continue
        with _lib.tuning(**knobs):
            try:
                outs[f"dev{flags}{knobs}"] = op.apply(dx, masked=masked, remap_area_min=area_min,
                                                     out_dtype=out_dtype, flags=flags, skipna=True).to_host()
            except _lib.SmmError as e:
                # a forced tile kernel whose planned form has split rows: refused, and the library's own choice
                # runs kernel A instead
                assert flags == T and e.code == _lib.SMM_ERR_UNSUPPORTED and "split" in str(e), str(e)
                assert op.launch_info(x.shape[0], x.dtype, flags=SK)["kernel"] == "sell"
                assert op.launch_info(x.shape[0], x.dtype)["kernel"] != "sell"
    sb = to_device(np.ascontiguousarray(x.T))
    outs["sb"] = op.apply_sb(sb, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=True).to_host()
    used = op.used_sources()
    sbp = to_device(np.ascontiguousarray(x[:, used].T))
    outs["sb_packed"] = op.apply_sb(sbp, masked=masked, remap_area_min=area_min, packed=True, out_dtype=out_dtype,
                                    skipna=True).to_host()
    outs["host"] = np.array(op.apply_host(x, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=True))
    outs["host_rows"] = np.array(op.apply_host(x, masked=masked, remap_area_min=area_min, out_dtype=out_dtype,
                                               flags=_lib.APPLY_HOST_NO_PACK, skipna=True))
    return outs


def _gridgen_op(method, src, dst):
    w = gridgen.generate_weights(src, dst, method=method)
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    return op, w["dst_grid_frac"].values if "dst_grid_frac" in w else None


def _make(case, rng):
    if case == "random":          # duplicates, negative and zero weights, empty rows
        src, dst, w = random_links(rng, 3000, 700, 5000, zero_frac=0.05)
        op = SparseOperator(3000, 700, src, dst, w, device=0)
        return op, rng.random(700)
    if case == "ragged":          # rows of 0 .. 40 links
        src, dst, w = ragged_links(rng, 4000, 500, max_len=40)
        return SparseOperator(4000, 500, src, dst, w, device=0), None
    return _gridgen_op(*case)


# 4 links (4-wave, LDS-DMA steps of 2 rows), 9 (4-wave), 20 (single-wave, 32), 42 (single-wave, 48)
CASES = [("bil", "r360x180", "r90x45"), ("con", "r144x72", "r48x24"), ("con", "r144x72", "r36x18"),
         ("con", "r720x360", "r120x60"), "random", "ragged"]


@pytest.mark.parametrize("case", CASES, ids=lambda c: c if isinstance(c, str) else "_".join(c))
@pytest.mark.parametrize("xdt,ydt", [(np.float64, np.float64), (np.float32, np.float32), (np.float32, np.float64),
                                     (np.float64, np.float32)])
def test_skipna_matches_restatement_on_every_form(hip, rng, case, xdt, ydt):
    op, frac = _make(case, rng)
    imask = (rng.random(op.n_dst) > 0.1).astype(np.int32)
    op.set_epilogue(imask, frac)
    csr = op.export_csr()
    x = field(rng, 37, op.n_src, dtype=xdt, nan_frac=0.03, inf_frac=0.005)
    x[3] = field(rng, 1, op.n_src, dtype=xdt, nan_frac=0.6)[0]        # rows with every link invalid
    x[5, : op.n_src // 3] = np.nan                                      # a patch
    x[7] = xdt(1e20)                                                    # finite but huge: valid, > 1e19 -> NaN
    for masked in (False, True):
        for area_min in ((0.0, 0.37, 1.0) if frac is not None else (0.0,)):   # area_min needs dst_frac
            ref = skipna_ref(csr, x, masked, imask, frac, area_min, ydt)
            for name, y in all_forms(op, x, masked, area_min, ydt).items():
                try:
                    bits_equal(y, ref)
                except AssertionError as e:
                    raise AssertionError(f"{name} masked={masked} area_min={area_min}: {e}") from None


@pytest.mark.parametrize("geom", [("bil", "r1440x721", "r360x180"), ("con", "r720x360", "r120x60")])
def test_skipna_is_plain_where_no_link_is_invalid(hip, rng, geom):
    op, frac = _gridgen_op(*geom)
    op.set_epilogue((rng.random(op.n_dst) > 0.1).astype(np.int32), frac)
    B = 522 if geom[1] == "r1440x721" else 40
    x = field(rng, B, op.n_src, dtype=np.float32)
    dx = to_device(x)
    for flags, knobs in kernel_forms(dict(tile_staging=REG), dict(tile_staging=DMA), dict(tile_split_rows=1),
                                     dict(tile_split_rows=1, tile_staging=DMA)):
        with _lib.tuning(**knobs):
            a = op.apply(dx, masked=True, remap_area_min=0.5, flags=flags).to_host()
            try:
                b = op.apply(dx, masked=True, remap_area_min=0.5, flags=flags, skipna=True).to_host()
            except _lib.SmmError as e:      # forced tile kernel on split rows (no skipna variant)
                assert flags == T and e.code == _lib.SMM_ERR_UNSUPPORTED and "split" in str(e), str(e)
                continue
        bits_equal(b, a)
    # NaN on some rows' links only: every other row stays bit-identical to the plain apply
    rowptr, col, _ = op.export_csr()
    x[::3, np.unique(col[: rowptr[op.n_dst // 4]])[::5]] = np.nan
    touched = np.zeros(op.n_dst, dtype=bool)
    bad_src = np.zeros(op.n_src, dtype=bool)
    bad_src[np.unique(np.nonzero(np.isnan(x).any(axis=0))[0])] = True
    rows = np.repeat(np.arange(op.n_dst), np.diff(rowptr))
    touched[np.unique(rows[bad_src[col]])] = True
    dx = to_device(x)
    a = op.apply(dx, masked=True, remap_area_min=0.5).to_host()
    b = op.apply(dx, masked=True, remap_area_min=0.5, skipna=True).to_host()
    sb = op.apply_sb(to_device(np.ascontiguousarray(x.T)), masked=True, remap_area_min=0.5, skipna=True).to_host()
    bits_equal(b[:, ~touched], a[:, ~touched])
    bits_equal(sb, b)
    # (bilinear between aligned grids: a row's one non-zero weight decides, NaN stays NaN -- no weight is left)
    assert np.isnan(b[:, touched]).sum() <= np.isnan(a[:, touched]).sum()
    if geom[0] == "con":
        assert np.isnan(b[:, touched]).sum() < np.isnan(a[:, touched]).sum()


def _regen_cmp(y, ref, frac_regen, area_min):
    keep = np.abs(frac_regen - area_min) >= 1e-9 if area_min > 0 else np.ones(frac_regen.shape, bool)
    y, ref = y[keep], ref[keep]
    assert np.array_equal(np.isnan(y), np.isnan(ref))
    ok = ~np.isnan(y)
    np.testing.assert_allclose(y[ok], ref[ok], rtol=1e-12, atol=0)


@pytest.mark.parametrize("area_min", [0.0, 0.37])
def test_skipna_equals_regenerated_conservative_weights(hip, rng, area_min):
    src, dst = "r144x72", "r36x18"
    w = gridgen.conservative_weights(src, dst, norm="fracarea")
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    op.set_epilogue(np.ones(op.n_dst, np.int32), w["dst_grid_frac"].values)
    nt = 4
    x = field(rng, nt, op.n_src)
    lat, lon = np.divmod(np.arange(op.n_src), 144)
    for t in range(nt):   # a random rectangular NaN patch per time step, plus scattered NaN
        la, lo = rng.integers(0, 60), rng.integers(0, 120)
        x[t, (lat >= la) & (lat < la + 10 + 3 * t) & (lon >= lo) & (lon < lo + 20)] = np.nan
        x[t, rng.random(op.n_src) < 0.03] = np.nan
    y = op.apply(to_device(x), remap_area_min=area_min, skipna=True).to_host()
    for t in range(nt):
        wr = gridgen.conservative_weights(src, dst, src_mask=np.isfinite(x[t]).astype(np.int32), norm="fracarea")
        opr = SparseOperator(op.n_src, op.n_dst, wr["src_address"].values, wr["dst_address"].values,
                             wr["remap_matrix"].values, device=0)
        fr = wr["dst_grid_frac"].values
        opr.set_epilogue(np.ones(op.n_dst, np.int32), fr)
        ref = opr.apply(to_device(x[t:t + 1]), remap_area_min=area_min).to_host()[0]
        # a target cell whose sources are all masked: no links -> 0 in the regenerated product, NaN under skipna
        ref = np.where(fr > 0, ref, np.nan)
        _regen_cmp(y[t], ref, fr, area_min)


def test_skipna_equals_regenerated_bilinear_weights(hip, rng):
    src, dst = "r144x72", "r60x30"
    w = gridgen.bilinear_weights(src, dst)
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    x = field(rng, 3, op.n_src)
    x[rng.random(x.shape) < 0.2] = np.nan
    y = op.apply(to_device(x), skipna=True).to_host()
    rowptr, col, val = op.export_csr()
    for t in range(3):
        valid = np.isfinite(x[t])
        wr = gridgen.bilinear_weights(src, dst, src_mask=valid.astype(np.int32))
        opr = SparseOperator(op.n_src, op.n_dst, wr["src_address"].values, wr["dst_address"].values,
                             wr["remap_matrix"].values, device=0)
        ref = opr.apply(to_device(x[t:t + 1])).to_host()[0]
        # rows whose valid corners all carry weight 0 ("flat" rows: gridgen shares them equally) and rows without
        # a valid corner (no link after regeneration) are left out
        wsum = np.add.reduceat(np.where(valid[col], val, 0.0), rowptr[:-1]) if col.size else np.zeros(op.n_dst)
        nvalid = np.add.reduceat(valid[col].astype(int), rowptr[:-1])
        keep = (wsum != 0.0) & (nvalid > 0)
        _regen_cmp(y[t][keep], ref[keep], np.ones(keep.sum()), 0.0)


def test_real_field_through_facade(hip):
    z = np.load(os.path.join(GOLDEN, "ua_ipsl_t0.npz"))
    ua = z["ua"]                                                          # (plev, lat, lon), 3 % NaN
    da = DataArray(ua, dims=("plev", "lat", "lon"), coords={"plev": z["plev"], "lat": z["lat"], "lon": z["lon"]},
                   name="ua")
    # weights made once for the grid (a field without NaN: no source mask), applied to every level
    grid = DataArray(np.zeros(ua.shape[1:]), dims=("lat", "lon"), coords={"lat": z["lat"], "lon": z["lon"]}, name="g")
    plain = Regridder(source_grid=grid, target_grid="r90x45").regrid(da).values
    out = Regridder(source_grid=grid, target_grid="r90x45", skipna=True).regrid(da).values
    assert out.shape == (19, 45, 90)
    n_plain = np.isnan(plain).reshape(19, -1).sum(axis=1)
    n_skip = np.isnan(out).reshape(19, -1).sum(axis=1)
    n_src = np.isnan(ua).reshape(19, -1).sum(axis=1)
    lowest = np.argsort(-n_src)[:3]                                       # the levels that reach below ground
    assert n_src[lowest].min() > 0
    assert (n_skip <= n_plain).all() and (n_skip[lowest] < n_plain[lowest]).all()
    # each level against weights regenerated from its own NaN mask
    src = gridgen.regular_grid_from_centers(z["lon"], z["lat"])
    for lev in range(19):
        valid = np.isfinite(ua[lev]).ravel()
        wr = gridgen.generate_weights(src, "r90x45", method="con", src_mask=valid.astype(np.int32))
        opr = SparseOperator(valid.size, 4050, wr["src_address"].values, wr["dst_address"].values,
                             wr["remap_matrix"].values, device=0)
        fr = wr["dst_grid_frac"].values
        opr.set_epilogue(np.ones(4050, np.int32), fr)
        ref = opr.apply(to_device(ua[lev].reshape(1, -1)), remap_area_min=0.5).to_host()[0]
        _regen_cmp(out[lev].ravel(), np.where(fr > 0, ref, np.nan), fr, 0.5)


def _masked_levels_group():
    z = np.load(os.path.join(GOLDEN, "con_masked_levels.npz"))
    ll = z["link_length"]
    ops = []
    for i in range(ll.size):
        op = SparseOperator(int(z["n_src"]), int(z["n_dst"]), z["src_address"][i, :ll[i]], z["dst_address"][i, :ll[i]],
                            z["remap_matrix"][i, :ll[i]], device=0)
        op.set_epilogue(z["dst_imask"][i], z["dst_frac"][i])
        ops.append(op)
    return z, ops


def test_group_equals_members(hip, rng):
    z, ops = _masked_levels_group()
    grp = OperatorGroup(ops)
    T_, L, S = 6, 4, int(z["n_src"])
    x = (250 + 30 * rng.standard_normal((T_, L, S)))
    x[rng.random(x.shape) < 0.05] = np.nan                                  # NaNs that change per time step
    for t in range(T_):
        x[t, :, (t * 97) % S: (t * 97) % S + 60] = np.nan
    lev = z["level_index"].astype(np.int32)
    ml = z["masked_levels"].astype(np.uint8)
    amin = float(z["area_min"])
    ref = np.empty((T_, L, ops[0].n_dst))
    for l in range(L):
        op = ops[lev[l]]
        y = op.apply(to_device(np.ascontiguousarray(x[:, l])), masked=bool(ml[lev[l]]), remap_area_min=amin,
                     skipna=True).to_host()
        bits_equal(y, skipna_ref(op.export_csr(), x[:, l], bool(ml[lev[l]]), z["dst_imask"][lev[l]],
                                 z["dst_frac"][lev[l]], amin))
        ref[:, l] = y
    y = grp.apply(to_device(x.reshape(T_, L, 1, S)), lev, ml, masked=True, remap_area_min=amin, skipna=True)
    bits_equal(y.to_host().reshape(T_, L, -1), ref)
    for flags, knobs in kernel_forms():
        with _lib.tuning(**knobs):
            y = grp.apply(to_device(x.reshape(T_, L, 1, S)), lev, ml, masked=True, remap_area_min=amin, flags=flags,
                          skipna=True)
        bits_equal(y.to_host().reshape(T_, L, -1), ref)
    xsb = to_device(np.ascontiguousarray(x.transpose(1, 2, 0)))            # (L, S, T)
    y = grp.apply_sb(xsb, lev, ml, masked=True, remap_area_min=amin, skipna=True).to_host()
    bits_equal(np.asarray(y).reshape(T_, L, -1), ref)
    y = grp.apply_host(x.reshape(T_, L, 1, S), lev, ml, masked=True, remap_area_min=amin, skipna=True)
    bits_equal(np.asarray(y).reshape(T_, L, -1), ref)
    y = grp.apply_host(x.reshape(T_, L, 1, S), lev, ml, masked=True, remap_area_min=amin, skipna=True,
                       flags=_lib.APPLY_HOST_NO_PACK)
    bits_equal(np.asarray(y).reshape(T_, L, -1), ref)


def test_lazy_and_dask_blocks_equal_eager(hip, rng):
    x = field(rng, 6, 72 * 36, nan_frac=0.05).reshape(6, 36, 72)
    lat, lon = np.arange(-87.5, 90, 5.0), np.arange(0, 360, 5.0)
    da = DataArray(x, dims=("time", "lat", "lon"), coords={"time": np.arange(6), "lat": lat, "lon": lon}, name="v")
    eager = Regridder(source_grid=da, target_grid="r36x18", skipna=True).regrid(da).values
    plain = Regridder(source_grid=da, target_grid="r36x18").regrid(da).values
    assert np.isnan(eager).sum() < np.isnan(plain).sum()
    lazy = Regridder(source_grid=da, target_grid="r36x18", skipna=True, lazy=True).regrid(da)
    bits_equal(np.asarray(lazy.values), eager)
    try:
        import dask.array as dsa
    except ImportError:
        dsa = None
    if dsa is not None:
        dd = DataArray(dsa.from_array(x, chunks=(2, 36, 72)), dims=da.dims, coords=da.coords, name="v")
        out = Regridder(source_grid=da, target_grid="r36x18", skipna=True, lazy=True).regrid(dd)
        bits_equal(np.asarray(out.data.compute()), eager)


def test_refusals(hip, rng):
    op, _ = _gridgen_op("con", "r144x72", "r36x18")        # 20 links: single-wave tile plan
    dx = to_device(field(rng, 4, op.n_src))
    with pytest.raises(_lib.SmmError) as e:
        op.apply(dx, flags=_lib.APPLY_NO_FILL, skipna=True)
    assert e.value.code == _lib.SMM_ERR_INVALID
    assert op.plan_info()["tile_plan"]
    with _lib.tuning(tile_links=1):                         # the streamed-link form has no skipna variant
        assert op.launch_info(4, flags=T)["kernel"] == "tile"
        assert op.launch_info(4, flags=SK)["kernel"] == "sell"
        with pytest.raises(_lib.SmmError) as e:
            op.apply(dx, flags=T, skipna=True)
        assert e.value.code == _lib.SMM_ERR_UNSUPPORTED
        y = op.apply(dx, skipna=True).to_host()             # the library's own choice runs kernel A
    bits_equal(y, op.apply(dx, flags=T, skipna=True).to_host())
    assert op.launch_info(4, flags=SK | T)["kernel"] in ("tile", "tile-dma")
