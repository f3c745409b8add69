"""CF-packed int16 / uint16 fields regridded raw (`cf=`, `Regridder(packed=True)`, the `_cf` entries): every result
is compared bit for bit with the existing path on the host-decoded field -- `op.apply(to_device(cf.decode(q)))` and
friends, which the other GPU tests tie to the oracle -- plus one direct oracle comparison per kernel."""
import ctypes
import hashlib

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (CdoGenerate, CFDecode, DataArray, Dataset, Regridder, SparseOperator, _lib, gridgen,
                           pinned_empty, to_device)

pytestmark = pytest.mark.gpu
PARENT_SHA256 = "ae59235d9c1a4d1c8e164c39b42473c07a31cc5e48abbc334dfe8a4d37652088"
PACKING = ("scale_factor", "add_offset", "_FillValue", "missing_value")


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


# ---------------------------------------------------------------- operators and fields

def _op_of(w):
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    return op, (w["dst_grid_frac"].values if "dst_grid_frac" in w else None)


def _banded_scattered(rng, nx=500, ny=200, n_dst=1500, k=12, band=4):
    """Every row draws its links anywhere inside a band of `band` source latitudes of its own: neighbouring rows
    share nothing, a block's footprint is far beyond an LDS tile, and the operator plans the SELL kernel."""
    src, dst, w = [], [], []
    for d in range(n_dst):
        j0 = int(rng.integers(0, ny - band + 1))
        cols = np.unique(j0 * nx + rng.integers(0, band * nx, size=k))
        ww = rng.random(cols.size) + 0.05
        src.append(cols + 1)
        dst.append(np.full(cols.size, d + 1))
        w.append(ww / ww.sum())
    src, dst, w = np.concatenate(src).astype(np.int32), np.concatenate(dst).astype(np.int32), np.concatenate(w)
    perm = rng.permutation(src.size)
    return SparseOperator(nx * ny, n_dst, src[perm], dst[perm], w[perm], device=0)


_OPS = {}


def operator(name):
    """(operator, dst_frac or None, (ny, nx) of the source, batch): built once per session."""
    if name not in _OPS:
        rng = np.random.default_rng(20261016)
        if name == "cfg2":          # config-2 geometry at a reduced, odd batch (two batch tiles of kernel C, one ragged)
            op, frac = _op_of(gridgen.bilinear_weights("r1440x721", "r360x180"))
            shape, batch = (721, 1440), 131
        elif name == "con":         # conservative, 9 links per row, with dst_frac
            op, frac = _op_of(gridgen.conservative_weights("r144x72", "r48x24"))
            shape, batch = (72, 144), 37
        else:                       # scattered: plans SELL
            op, frac = _banded_scattered(rng), None
            shape, batch = (200, 500), 21
        imask = (rng.random(op.n_dst) > 0.1).astype(np.int32)          # 10 % masked rows (< 30 %)
        op.set_epilogue(imask, frac)
        _OPS[name] = (op, frac, imask, shape, batch)
    return _OPS[name]


def raw_field(rng, dtype, batch, shape, k_max, fills):
    """Raw values over the whole range of the type; the fill values on one lon/lat rectangle of ~5 % of the cells
    plus scattered cells at a rate of 0.1 / k_max (k_max: the operator's longest row)."""
    info = np.iinfo(dtype)
    ny, nx = shape
    q = rng.integers(info.min, info.max + 1, size=(batch, ny, nx)).astype(dtype)
    q[:, 0, :5] = np.array([info.min, info.max, 0, 1, info.max - 1], dtype=dtype)
    for f in fills:                                  # the range is full: values that equal a fill by chance move on
        q[q == f] = f + 1 if f < info.max else f - 1
    hy = max(1, int(round(0.05 * ny)))               # full longitude circle x 5 % of the latitudes: contiguous cells
    y0 = ny // 3
    q[:, y0:y0 + hy, :] = fills[0]
    scattered = rng.random(q.shape) < 0.1 / k_max
    q[scattered] = np.where(rng.random(int(scattered.sum())) < 0.5, fills[0], fills[-1]).astype(dtype)
    return q.reshape(batch, ny * nx)


def rule(dtype, decode):
    """int16: ERA5-like scale and an offset large enough that the float32 decode rounds; uint16: a negative scale.
    Two distinct fill values each, one at the edge of the raw range (-32768 / 65535)."""
    if dtype == np.int16:
        return CFDecode(1.9e-3, 2.7e2, (-32768, 7), decode)
    return CFDecode(-0.25, 12.5, (65535, 300), decode)


EPILOGUES = [(False, 0.0), (True, 0.0), (True, 0.5)]


@pytest.mark.parametrize("decode", [np.float32, np.float64], ids=["f32", "f64"])
@pytest.mark.parametrize("dtype", [np.int16, np.uint16], ids=["i16", "u16"])
@pytest.mark.parametrize("name", ["cfg2", "con", "scattered"])
def test_kernels_a_and_c_equal_the_host_decode(hip, name, dtype, decode):
    op, frac, imask, shape, batch = operator(name)
    rng = np.random.default_rng(7 + batch)
    cf = rule(dtype, decode)
    q = raw_field(rng, dtype, batch, shape, op.max_row_nnz, cf.fill_values)
    x = cf.decode(q)
    assert x.dtype == decode and np.isnan(x).any()
    if decode == np.float32 and dtype == np.int16:   # the offset makes the float32 decode round
        assert not np.array_equal(x.astype(np.float64), CFDecode(1.9e-3, 2.7e2, (-32768, 7), np.float64).decode(q))
    if name == "scattered":
        assert not op.plan_info()["tile_preferred"]
    dq, dx = to_device(q), to_device(x)
    dqt, dxt = to_device(np.ascontiguousarray(q.T), layout="sb"), to_device(np.ascontiguousarray(x.T), layout="sb")
    used = op.used_sources()
    dqp, dxp = to_device(np.ascontiguousarray(q.T[used])), to_device(np.ascontiguousarray(x.T[used]))
    for masked, area_min in EPILOGUES:
        if area_min > 0.0 and frac is None:
            continue
        for skipna in (False, True):
            kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
            what = f"{name} {np.dtype(dtype).name}->{np.dtype(decode).name} {kw}"
            want = op.apply(dx, **kw).to_host()
            nan_share_ok(want, what)
            bits_equal(op.apply(dq, cf=cf, **kw).to_host(), want, what + " kernel A")
            bits_equal(op.apply(dq, cf=cf, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host(), want, what + " forced SELL")
            want_sb = op.apply_sb(dxt, **kw).to_host()
            bits_equal(want_sb, want, what + " existing kernel C")
            bits_equal(op.apply(dqt, cf=cf, **kw).to_host(), want, what + " kernel C")
            bits_equal(op.apply_sb(dqp, packed=True, cf=cf, **kw).to_host(),
                       op.apply_sb(dxp, packed=True, **kw).to_host(), what + " kernel C SB_PACKED")
            kept = op.apply_sb(dqt, keep_batch_fastest=True, cf=cf, **kw)
            assert kept.layout == "sb" and kept.shape == (op.n_dst, batch)
            bits_equal(kept.to_host(), op.apply_sb(dxt, keep_batch_fastest=True, **kw).to_host(), what + " kernel C Y_SB")


@pytest.mark.parametrize("dtype,decode", [(np.int16, np.float32), (np.uint16, np.float64)])
def test_each_kernel_against_the_oracle(hip, dtype, decode):
    op, frac, imask, shape, batch = operator("con")
    rng = np.random.default_rng(11)
    cf = rule(dtype, decode)
    q = raw_field(rng, dtype, batch, shape, op.max_row_nnz, cf.fill_values)
    ref = oracle.apply_c(op.export_csr(), cf.decode(q), True, imask, frac, 0.5)
    nan_share_ok(ref, "oracle")
    bits_equal(op.apply(to_device(q), masked=True, remap_area_min=0.5, cf=cf).to_host(), ref, "kernel A vs oracle")
    bits_equal(op.apply_sb(to_device(np.ascontiguousarray(q.T)), masked=True, remap_area_min=0.5, cf=cf).to_host(), ref,
               "kernel C vs oracle")
    bits_equal(op.apply_host(q, masked=True, remap_area_min=0.5, cf=cf), ref, "host pipeline vs oracle")


def test_tiny_and_ragged_batches(hip):
    """Kernel C's element-wise walk (one batch entry) and odd / short batches of both kernels."""
    op, frac, imask, shape, _ = operator("con")
    rng = np.random.default_rng(5)
    cf = rule(np.uint16, np.float32)
    for batch in (1, 2, 3, 5, 129):
        q = raw_field(rng, np.uint16, batch, shape, op.max_row_nnz, cf.fill_values)
        for skipna in (False, True):
            want = op.apply(to_device(cf.decode(q)), masked=True, remap_area_min=0.5, skipna=skipna).to_host()
            bits_equal(op.apply(to_device(q), masked=True, remap_area_min=0.5, skipna=skipna, cf=cf).to_host(), want,
                       f"A B={batch}")
            bits_equal(op.apply_sb(to_device(np.ascontiguousarray(q.T)), masked=True, remap_area_min=0.5, skipna=skipna,
                                   cf=cf).to_host(), want, f"C B={batch}")


def test_launch_info_and_refusals(hip):
    op, frac, imask, shape, batch = operator("cfg2")
    info_f = op.launch_info(batch, np.float32)
    assert info_f["kernel"] in ("tile", "tile-dma"), info_f                    # config 2 plans the LDS tile kernel for float fields
    for dtype in (np.int16, np.uint16):
        info = op.launch_info(batch, dtype)
        assert info["kernel"] == "sell" and info["rows_per_block"] == 256, info          # ... and kernel A for packed ones
        assert info == op.launch_info(batch, np.float32, flags=_lib.APPLY_KERNEL_SELL)
        with pytest.raises(_lib.SmmError) as e:
            op.launch_info(batch, dtype, flags=_lib.APPLY_KERNEL_TILE)
        assert e.value.code == _lib.SMM_ERR_UNSUPPORTED
    cf = rule(np.int16, np.float32)
    q = raw_field(np.random.default_rng(3), np.int16, 4, shape, op.max_row_nnz, cf.fill_values)
    dq = to_device(q)
    with pytest.raises(_lib.SmmError) as e:                      # forced tile kernel: not built for packed fields
        op.apply(dq, cf=cf, flags=_lib.APPLY_KERNEL_TILE)
    assert e.value.code == _lib.SMM_ERR_UNSUPPORTED
    with pytest.raises(_lib.SmmError) as e:                      # the decode makes NaN: NO_FILL cannot hold
        op.apply(dq, cf=cf, flags=_lib.APPLY_NO_FILL)
    assert e.value.code == _lib.SMM_ERR_INVALID
    nofill = CFDecode(1.9e-3, 2.7e2, (), np.float32)             # without fill values NO_FILL is the caller's promise
    bits_equal(op.apply(dq, cf=nofill, flags=_lib.APPLY_NO_FILL).to_host(),
               op.apply(to_device(nofill.decode(q)), flags=_lib.APPLY_NO_FILL).to_host(), "NO_FILL")
    with pytest.raises(_lib.SmmError) as e:                      # float32 results are not built
        op.apply(dq, cf=cf, out_dtype=np.float32)
    assert e.value.code == _lib.SMM_ERR_UNSUPPORTED
    with pytest.raises(TypeError):                               # an integer field without a rule: as before
        op.apply(dq)
    with pytest.raises(TypeError):
        op.apply(to_device(q.astype(np.float32)), cf=cf)
    # the plain entries still refuse the packed dtype codes
    lib = _lib.load()
    y = to_device(np.zeros((4, op.n_dst)))
    for entry in ("smm_apply", "smm_apply_sb"):
        rc = getattr(lib, entry)(op.handle, ctypes.c_void_p(dq.ptr), _lib.SMM_I16, op.n_src, ctypes.c_void_p(y.ptr),
                                 _lib.SMM_F64, op.n_dst, 4, 0.0, 0, None)
        assert rc == _lib.SMM_ERR_UNSUPPORTED, entry
    out = np.zeros((4, op.n_dst))
    rc = lib.smm_apply_host(op.handle, q.ctypes.data_as(ctypes.c_void_p), _lib.SMM_I16, op.n_src,
                            out.ctypes.data_as(ctypes.c_void_p), _lib.SMM_F64, op.n_dst, 4, 0.0, 0, 0)
    assert rc == _lib.SMM_ERR_UNSUPPORTED
    # cf == NULL with a float dtype is the plain entry
    x = nofill.decode(q)
    y2 = to_device(np.zeros((4, op.n_dst)))
    assert lib.smm_apply_cf(op.handle, ctypes.c_void_p(to_device(x).ptr), _lib.SMM_F32, op.n_src, ctypes.c_void_p(y2.ptr),
                            _lib.SMM_F64, op.n_dst, 4, 0.0, 0, None, None) == _lib.SMM_OK
    bits_equal(y2.to_host(), op.apply(to_device(x)).to_host(), "cf NULL")


# ---------------------------------------------------------------- host pipeline

@pytest.mark.parametrize("dtype", [np.int16, np.uint16], ids=["i16", "u16"])
def test_apply_host_packed_ships_two_bytes_per_cell(hip, dtype):
    """Odd n_src (row starts only 2-byte aligned), a batch that is no multiple of the chunk, a caller's chunk_rows,
    a row pitch beyond n_src, pageable and pinned input; packed and whole-row staging; 2 B per shipped cell."""
    op, frac = _op_of(gridgen.bilinear_weights("r143x71", "r36x18"))
    assert op.n_src % 2 == 1 and op.n_used_src * 5 <= op.n_src * 4
    rng = np.random.default_rng(17)
    imask = (rng.random(op.n_dst) > 0.1).astype(np.int32)
    op.set_epilogue(imask, frac)
    cf = rule(dtype, np.float32)
    B, S, U, D = 203, op.n_src, op.n_used_src, op.n_dst
    q = raw_field(rng, dtype, B, (71, 143), op.max_row_nnz, cf.fill_values)
    x = cf.decode(q)
    wide = np.zeros((B, S + 5), dtype)
    wide[:, :S] = q
    pinned = pinned_empty((B, S), dtype)
    pinned[...] = q
    for skipna in (False, True):
        kw = dict(masked=True, skipna=skipna)
        want = op.apply(to_device(x), **kw).to_host()
        nan_share_ok(want, f"host {skipna}")
        for label, arr, extra, cells in (("packed", q, {}, U), ("packed chunk 48", q, {"chunk_rows": 48}, U),
                                         ("whole rows", q, {"flags": _lib.APPLY_HOST_NO_PACK}, S),
                                         ("whole rows chunk 50", q, {"flags": _lib.APPLY_HOST_NO_PACK, "chunk_rows": 50}, S),
                                         ("pitch", wide[:, :S], {}, U), ("pitch whole rows", wide[:, :S],
                                                                          {"flags": _lib.APPLY_HOST_NO_PACK}, S),
                                         ("pinned", pinned, {}, U),
                                         ("pinned whole rows", pinned, {"flags": _lib.APPLY_HOST_NO_PACK}, S)):
            _lib.host_stats(reset=True)
            got = op.apply_host(arr, cf=cf, **kw, **extra)
            st = _lib.host_stats(reset=True)
            bits_equal(got, want, f"{label} skipna={skipna}")
            assert st["h2d_bytes"] == 2 * cells * B, (label, st)
            assert st["d2h_bytes"] == 8 * D * B, (label, st)
            if "chunk_rows" in extra:
                assert st["chunks"] == -(-B // extra["chunk_rows"]), (label, st)
        # the same calls on the float32 decode ship 4 B per cell
        for extra, cells in (({}, U), ({"flags": _lib.APPLY_HOST_NO_PACK}, S)):
            _lib.host_stats(reset=True)
            bits_equal(op.apply_host(x, **kw, **extra), want, "float32 host path")
            assert _lib.host_stats(reset=True)["h2d_bytes"] == 4 * cells * B


def test_apply_host_config2_rows(hip):
    """The path the feature is for: config-2 rows through the packing pipeline (streaming 2-byte pack, kernel C)."""
    op, frac, imask, shape, batch = operator("cfg2")
    rng = np.random.default_rng(23)
    cf = rule(np.int16, np.float64)
    q = raw_field(rng, np.int16, 96, shape, op.max_row_nnz, cf.fill_values)
    want = op.apply(to_device(cf.decode(q)), masked=True, skipna=True).to_host()
    nan_share_ok(want, "cfg2 host")
    _lib.host_stats(reset=True)
    got = op.apply_host(q, masked=True, skipna=True, cf=cf)
    st = _lib.host_stats(reset=True)
    bits_equal(got, want, "cfg2 host packed")
    assert st["h2d_bytes"] == 2 * op.n_used_src * 96, st


# ---------------------------------------------------------------- Regridder

def _packed_da(rng, nt=6, name="t2m"):
    src = gridgen.parse_grid("r180x90")
    cf = CFDecode(1.9e-3, 2.7e2, (-32768, 7), np.float32)
    q = raw_field(rng, np.int16, nt, (90, 180), 4, cf.fill_values).reshape(nt, 90, 180)
    attrs = {"scale_factor": 1.9e-3, "add_offset": 2.7e2, "_FillValue": np.int16(-32768), "missing_value": np.int16(7),
             "units": "K", "long_name": "2 metre temperature"}
    coords = {"time": np.arange(nt), "lat": src.lat, "lon": src.lon}
    da = DataArray(q, dims=("time", "lat", "lon"), coords=coords, name=name, attrs=attrs)
    dec = DataArray(cf.decode(q), dims=da.dims, coords=coords, name=name,
                    attrs={k: v for k, v in attrs.items() if k not in PACKING})
    return da, dec, cf


@pytest.mark.parametrize("skipna", [False, True])
def test_regridder_packed_equals_decoded(hip, skipna):
    rng = np.random.default_rng(29)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da, dec, cf = _packed_da(rng)
    want = Regridder(weights=w, skipna=skipna).regrid(dec)
    got = Regridder(weights=w, skipna=skipna, packed=True).regrid(da)
    nan_share_ok(want.values, f"regridder skipna={skipna}")
    assert got.dims == want.dims and got.values.dtype == np.float64
    bits_equal(got.values, want.values, "Regridder")
    assert got.attrs == want.attrs == {"units": "K", "long_name": "2 metre temperature"}
    assert list(got.coords) == list(want.coords)
    for k in got.coords:
        assert np.array_equal(got.coords[k].values, want.coords[k].values)
    # a device-resident packed field, both layouts; lazy; float32 results (decoded on the host)
    rg = Regridder(weights=w, skipna=skipna, packed=True)
    dev = DataArray(to_device(da.data), dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs)
    bits_equal(rg.regrid(dev).values, want.values, "device field")
    sb = DataArray(to_device(np.ascontiguousarray(da.data.transpose(1, 2, 0)), layout="sb"), dims=("lat", "lon", "time"),
                   coords=da.coords, name=da.name, attrs=da.attrs)
    bits_equal(rg.regrid(sb).values, want.values, "batch-fastest device field")
    lazy = Regridder(weights=w, skipna=skipna, packed=True, lazy=True).regrid(da)
    bits_equal(np.asarray(lazy.values), want.values, "lazy")
    got32 = Regridder(weights=w, skipna=skipna, packed=True, out_dtype=np.float32).regrid(da)
    bits_equal(got32.values, Regridder(weights=w, skipna=skipna, out_dtype=np.float32).regrid(dec).values, "float32")
    assert not set(PACKING) & set(got32.attrs)


def test_regridder_dataset_mixing_packed_and_float(hip):
    rng = np.random.default_rng(31)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da, dec, cf = _packed_da(rng)
    other = DataArray(250.0 + rng.standard_normal((6, 90, 180)), dims=da.dims, coords=da.coords, name="tas",
                      attrs={"units": "K"})
    out = Regridder(weights=w, packed=True).regrid(Dataset({"t2m": da, "tas": other}, coords=dict(da.coords)))
    plain = Regridder(weights=w)
    bits_equal(out["t2m"].values, plain.regrid(dec).values, "packed variable")
    bits_equal(out["tas"].values, plain.regrid(other).values, "float variable")
    assert not set(PACKING) & set(out["t2m"].attrs) and out["tas"].attrs == {"units": "K"}


def test_regridder_packed_false_is_the_parent(hip):
    """packed=False (the default) on the same int16 input: the integers are regridded as numbers, as before.
    sha256 of the (6, 45, 90) float64 output, C order, of the parent commit's library on this input:
    ae59235d9c1a4d1c8e164c39b42473c07a31cc5e48abbc334dfe8a4d37652088 (also what the CPU oracle gives on
    q.astype(float64))."""
    rng = np.random.default_rng(37)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da, dec, cf = _packed_da(rng)
    csr = oracle.coo_to_csr_c(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                              w["dst_address"].values, w["remap_matrix"].values)
    imask = oracle.mask_apply_c(csr, w["src_grid_imask"].values)
    ref = oracle.apply_c(csr, da.data.reshape(6, -1).astype(np.float64), masked=oracle.check_mask(imask), dst_imask=imask,
                         dst_frac=w["dst_grid_frac"].values, area_min=0.5)
    for rg in (Regridder(weights=w), Regridder(weights=w, packed=False)):
        out = rg.regrid(da)
        bits_equal(out.values.reshape(6, -1), ref, "packed=False")
        assert out.attrs == da.attrs                  # nothing dropped
        assert hashlib.sha256(np.ascontiguousarray(out.values).tobytes()).hexdigest() == PARENT_SHA256


def test_regridder_levels_fall_back_to_the_host_decode(hip, caplog):
    """3-D weights (masked levels) take no packed input at the ABI: decoded on the host, one INFO line, same bits."""
    rng = np.random.default_rng(41)
    g = gridgen.parse_grid("r72x36")
    levels, nt = (5.0, 50.0, 500.0, 2000.0), 3
    masks = gridgen.synthetic_ocean_masks(72, 36, len(levels), top=0.95, bottom=0.6)   # land = fill: 5 .. 40 % per level
    cf = CFDecode(1.0e-3, 20.0, (-32768,), np.float32)
    q = rng.integers(-32767, 32768, size=(nt, len(levels), 36, 72)).astype(np.int16)
    for l in range(len(levels)):
        q[:, l].reshape(nt, -1)[:, masks[l] == 0] = -32768
    coords = {"time": np.arange(nt), "lev": np.asarray(levels), "lat": g.lat, "lon": g.lon}
    attrs = {"scale_factor": 1.0e-3, "add_offset": 20.0, "_FillValue": np.int16(-32768), "units": "psu"}
    da = DataArray(q, dims=("time", "lev", "lat", "lon"), coords=coords, name="so", attrs=attrs)
    dec = DataArray(cf.decode(q), dims=da.dims, coords=coords, name="so", attrs={"units": "psu"})
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    want = Regridder(weights=w3).regrid(dec)
    rg = Regridder(weights=w3, packed=True, loglevel="INFO")
    with caplog.at_level("INFO"):
        got = rg.regrid(da)
    assert sum("decoded on the host" in r.getMessage() for r in caplog.records) == 1
    nan_share_ok(want.values, "levels")
    bits_equal(got.values, want.values, "levels")
    assert got.attrs == want.attrs == {"units": "psu"} and got.dims == want.dims
