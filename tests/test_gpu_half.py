"""float16 / bfloat16 fields and results regridded inside the kernels (SMM_F16 / SMM_BF16).  Every comparison is bit
equality.  The expectation is the CPU oracle (`oracle.apply_c`, `helpers.skipna_ref` for skipna) applied to the field
widened to float32 on the host, narrowed on the host by `astype(np.float16)` or -- bfloat16 -- by the integer rounding
of tests/half_cases.py, which tests/test_half_abi.py checks against exact rational arithmetic.  NaN results must be the
canonical quiet NaN (0x7E00 / 0x7FC0)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (DataArray, DeviceArray, OperatorGroup, Regridder, SparseOperator, _lib, bfloat16, gridgen,
                           to_device)
from tests import half_cases as hc
from tests import sb_cases
from tests.helpers import skipna_ref

pytestmark = pytest.mark.gpu

F16, F32, F64 = np.dtype(np.float16), np.dtype(np.float32), np.dtype(np.float64)
NP_OF = {"f16": F16, "bf16": bfloat16, "f32": F32, "f64": F64}
# the built rows with a half type, as smm_built.hpp lists them: (field, result)
ROWS = [(r.x, r.y) for r in sb_cases.ROWS if {"f16", "bf16"} & {r.x, r.y}]
BATCHES = (1, 3, 70, 130)
N_DST = (70, 130)
EPILOGUES = ((False, 0.0), (True, 0.3))           # (masked, remap_area_min)


def narrow(y64, kind):
    """The float64 expectation as the bits Y must hold."""
    if kind == "f64":
        return np.where(np.isnan(y64), np.uint64(0x7FF8000000000000), y64.view(np.uint64))
    if kind == "f16":
        with np.errstate(over="ignore"):
            bits = y64.astype(np.float16).view(np.uint16)
        return np.where(np.isnan(y64), np.uint16(0x7E00), bits)
    return hc.round_bits(y64, kind)


def bits_of(y, kind):
    y = np.asarray(y)
    if kind == "f64":
        return np.where(np.isnan(y), np.uint64(0x7FF8000000000000), y.view(np.uint64))     # f64 NaN: by class
    return y.view(np.uint16)


def same_bits(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} of {got.size} differ, first {bad[:3].tolist()}: " \
                          f"{[hex(int(got[tuple(i)])) for i in bad[:3]]} != {[hex(int(want[tuple(i)])) for i in bad[:3]]}"


@functools.lru_cache(maxsize=None)
def single(n_dst):
    """(operator, csr, imask, frac)"""
    src, dst, w = hc.small_links(n_dst, seed=n_dst)
    imask, frac = hc.epilogue_vectors(n_dst, seed=n_dst)
    op = SparseOperator(hc.N_SRC, n_dst, src, dst, w, device=0)
    op.set_epilogue(imask, frac)
    return op, oracle.coo_to_csr_c(hc.N_SRC, n_dst, src, dst, w), imask, frac


@functools.lru_cache(maxsize=None)
def levels(n_dst=70):
    """Three levels, the middle one masked, and the data levels (2, 0, 1) -> a subset in another order."""
    ops, csrs, imasks, fracs = [], [], [], []
    for lev in range(3):
        src, dst, w = hc.small_links(n_dst, seed=100 + lev)
        imask, frac = hc.epilogue_vectors(n_dst, seed=100 + lev)
        if lev != 1:
            imask = np.ones(n_dst, np.int32)
        op = SparseOperator(hc.N_SRC, n_dst, src, dst, w, device=0)
        op.set_epilogue(imask, frac)
        ops.append(op)
        csrs.append(oracle.coo_to_csr_c(hc.N_SRC, n_dst, src, dst, w))
        imasks.append(imask)
        fracs.append(frac)
    return OperatorGroup(ops), csrs, imasks, fracs, np.array([0, 1, 0], np.uint8)


@functools.lru_cache(maxsize=None)
def field(xk, shape, seed=5):
    """(array in the field's own dtype, the float32 / float64 array the oracle takes)"""
    if xk in ("f16", "bf16"):
        bits = hc.half_field(xk, shape, seed)
        return bits.view(NP_OF[xk]), hc.widen(bits, xk)
    x = hc.float_field(NP_OF[xk], shape, seed)
    return x, x


@functools.lru_cache(maxsize=None)
def expected(n_dst, xk, batch, skipna, masked, area_min):
    _, csr, imask, frac = single(n_dst)
    ref_x = field(xk, (batch, hc.N_SRC))[1]
    if skipna:
        return skipna_ref(csr, ref_x, masked=masked, imask=imask, frac=frac, area_min=area_min)
    return oracle.apply_c(csr, ref_x, masked=masked, dst_imask=imask, dst_frac=frac, area_min=area_min)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("xk,yk", ROWS, ids=[f"{x}-{y}" for x, y in ROWS])
def test_every_built_row_on_kernels_a_and_c(hip, xk, yk, skipna):
    for n_dst in N_DST:
        op = single(n_dst)[0]
        for batch in BATCHES:
            x = field(xk, (batch, hc.N_SRC))[0]
            dx = to_device(x)
            dxt = to_device(np.ascontiguousarray(x.T), layout="sb")
            for masked, area_min in EPILOGUES:
                want = narrow(expected(n_dst, xk, batch, skipna, masked, area_min), yk)
                what = f"{xk}->{yk} D={n_dst} B={batch} masked={masked} area_min={area_min}"
                kw = dict(masked=masked, remap_area_min=area_min, out_dtype=NP_OF[yk], skipna=skipna)
                y = op.apply(dx, **kw)
                assert y.dtype == NP_OF[yk]
                same_bits(bits_of(y.to_host(), yk), want, "kernel A " + what)
                same_bits(bits_of(op.apply_sb(dxt, **kw).to_host(), yk), want, "kernel C " + what)
                ysb = op.apply_sb(dxt, keep_batch_fastest=True, **kw)
                assert ysb.layout == "sb" and ysb.shape == (n_dst, batch)
                same_bits(bits_of(ysb.to_host(), yk).T, want, "kernel C, Y batch-fastest " + what)
            if yk != "f64" and batch == 130:       # the 16-row tile of a 2-byte Y
                with _lib.tuning(sb_packed_y_rows=16):
                    same_bits(bits_of(op.apply_sb(dxt, **kw).to_host(), yk), want, "kernel C, 16-row tiles " + what)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("xk,yk", ROWS, ids=[f"{x}-{y}" for x, y in ROWS])
def test_every_built_row_on_a_level_group(hip, xk, yk, skipna):
    group, csrs, imasks, fracs, masked_levels = levels()
    level_index = np.array([2, 0, 1], np.int32)
    for n_lev, batch in ((3, 3), (2, 130), (3, 70)):
        lev = level_index[:n_lev]
        x, ref_x = field(xk, (n_lev, batch, hc.N_SRC), seed=9)
        for area_min in (0.0, 0.3):
            want = []
            for l, w in enumerate(lev):
                m = bool(masked_levels[w])
                if skipna:
                    want.append(skipna_ref(csrs[w], ref_x[l], masked=m, imask=imasks[w], frac=fracs[w], area_min=area_min))
                else:
                    want.append(oracle.apply_c(csrs[w], ref_x[l], masked=m, dst_imask=imasks[w], dst_frac=fracs[w],
                                               area_min=area_min))
            want = narrow(np.stack(want), yk)                                     # (n_lev, B, D)
            what = f"{xk}->{yk} levels={lev.tolist()} B={batch} area_min={area_min}"
            kw = dict(masked=True, remap_area_min=area_min, out_dtype=NP_OF[yk], skipna=skipna, transpose=False)
            dx = to_device(np.ascontiguousarray(x.reshape(n_lev, 1, batch, hc.N_SRC).transpose(1, 0, 2, 3)))
            y = group.apply(dx, lev, masked_levels, **kw).to_host()               # (n_lev, 1, B, D)
            same_bits(bits_of(y, yk)[:, 0], want, "group kernel A " + what)
            dxs = to_device(np.ascontiguousarray(x.transpose(0, 2, 1)), layout="sb")        # (n_lev, S, B)
            y = group.apply_sb(dxs, lev, masked_levels, **kw).to_host()
            same_bits(bits_of(y, yk), want, "grouped kernel C " + what)
            y = group.apply_sb(dxs, lev, masked_levels, keep_batch_fastest=True, **kw).to_host()     # (n_lev, D, B)
            same_bits(bits_of(y, yk).transpose(0, 2, 1), want, "grouped kernel C, Y batch-fastest " + what)


def _identity(n, two_links=False):
    """Row d = 1.0 * x[d] (+ 1.0 * x[n], a cell that holds +0.0, with two_links)."""
    d = np.arange(1, n + 1, dtype=np.int32)
    if not two_links:
        return SparseOperator(n, n, d, d, np.ones(n), device=0)
    return SparseOperator(n + 1, n, np.concatenate([d, np.full(n, n + 1, np.int32)]), np.concatenate([d, d]),
                          np.ones(2 * n), device=0)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_encode_is_one_correctly_rounded_conversion(hip, kind):
    """float64 X through one-link rows of weight 1 and two-link rows (x + 0.0): the stored bits are those of the exact
    rounding of the epilogue's value -- no float32 in between, overflow to inf, subnormals kept, canonical NaN."""
    vals = hc.adversarial(kind)
    n = vals.size
    v = np.where(vals > 1e19, np.nan, vals)                    # the epilogue comes first
    v = np.where(np.isfinite(vals), v, np.nan)                 # non-finite X: filled with 1e20, beyond 1e19 -> NaN
    v = v + 0.0                                                # a row's sum starts at +0.0: a -0.0 element gives +0.0
    want = np.array([hc.exact_bits(float(t), kind) for t in v], dtype=np.uint16)
    assert np.array_equal(want, narrow(v, kind))
    first = {"f16": 0x3C01, "bf16": 0x3F81}[kind]              # 1 + ulp/2 + 2**-40 rounds up; via float32 it would be 1.0
    assert want[0] == first
    # a bfloat16 result just below / above 1e19: finite / NaN by the epilogue
    below, above = int(np.argmax(vals == np.nextafter(1e19, 0.0))), int(np.argmax(vals == np.nextafter(1e19, np.inf)))
    assert want[above] == hc.KINDS[kind][2]
    assert want[below] == 0x7C00 if kind == "f16" else (want[below] & 0x7F80) != 0x7F80       # inf / a finite bfloat16
    for two in (False, True):
        op = _identity(n, two)
        x = np.concatenate([vals, [0.0]]) if two else vals
        xb = np.stack([x, x[::-1].copy() if not two else x, x])          # three batch rows
        want2 = np.stack([want, want[::-1] if not two else want, want])
        y = op.apply(to_device(xb), out_dtype=NP_OF[kind]).to_host().view(np.uint16)
        same_bits(y, want2, f"kernel A {kind} two_links={two}")
        y = op.apply_sb(to_device(np.ascontiguousarray(xb.T), layout="sb"), out_dtype=NP_OF[kind]).to_host().view(np.uint16)
        same_bits(y, want2, f"kernel C {kind} two_links={two}")


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_decode_of_every_pattern_is_exact(hip, kind):
    """All 65 536 patterns through an identity operator: the float64 result is the widened value where it is finite and
    not beyond 1e19, NaN where the fill rule makes it so -- subnormals included, nothing flushed."""
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    x32 = hc.widen(bits, kind)
    op = _identity(65536)
    fin = np.isfinite(x32)
    want64 = np.where(fin & ~(x32.astype(np.float64) > 1e19), x32.astype(np.float64), np.nan) + 0.0   # -0.0 sums to +0.0
    rowptr = np.arange(65537, dtype=np.int64)
    ref = oracle.apply_c((rowptr, np.arange(65536, dtype=np.int32), np.ones(65536)), x32[None, :])
    assert np.array_equal(narrow(ref, "f64")[0], narrow(want64, "f64"))           # the oracle says the same
    x = np.stack([bits, bits[::-1]]).view(NP_OF[kind])
    want = np.stack([narrow(want64, "f64"), narrow(want64, "f64")[::-1]])
    y = op.apply(to_device(x)).to_host()
    same_bits(bits_of(y, "f64"), want, f"kernel A {kind}")
    y = op.apply_sb(to_device(np.ascontiguousarray(x.T), layout="sb")).to_host()
    same_bits(bits_of(y, "f64"), want, f"kernel C {kind}")
    # and back into the same half type: every finite pattern that survives the epilogue is stored as it came
    y = op.apply(to_device(x), out_dtype=NP_OF[kind]).to_host().view(np.uint16)[0]
    keep = ~np.isnan(want64) & (bits != 0x8000)
    assert np.array_equal(y[keep], bits[keep]) and (y[np.isnan(want64)] == hc.KINDS[kind][2]).all() and y[0x8000] == 0


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_host_pipelines_ship_two_byte_cells(hip, kind):
    """smm_apply_host (used cells packed, and whole rows) and smm_group_apply_host with half X and half Y: the bits of
    the device entries, in two chunks, 2 bytes per cell in each direction."""
    n_dst, batch, used = 130, 24, 100
    src, dst, w = hc.small_links(n_dst, seed=77, used=used)            # half of the source cells carry links
    imask, frac = hc.epilogue_vectors(n_dst, seed=77)
    op = SparseOperator(hc.N_SRC, n_dst, src, dst, w, device=0)
    op.set_epilogue(imask, frac)
    assert op.n_used_src * 5 <= hc.N_SRC * 4
    x = field(kind, (batch, hc.N_SRC), seed=21)[0]
    kw = dict(masked=True, remap_area_min=0.3, out_dtype=NP_OF[kind])
    want = op.apply(to_device(x), **kw).to_host().view(np.uint16)
    for flags, cells in ((0, op.n_used_src), (_lib.APPLY_HOST_NO_PACK, hc.N_SRC)):
        _lib.host_stats(reset=True)
        y = op.apply_host(x, flags=flags, chunk_rows=12, half=True, **kw)
        st = _lib.host_stats()
        assert y.dtype == NP_OF[kind]
        same_bits(y.view(np.uint16), want, f"apply_host {kind} flags={flags}")
        assert st["chunks"] == 2
        assert st["h2d_bytes"] == 2 * cells * batch and st["d2h_bytes"] == 2 * n_dst * batch
    # skipna and a float64 result on the same pipeline
    want = op.apply(to_device(x), skipna=True, remap_area_min=0.3).to_host()
    y = op.apply_host(x, skipna=True, remap_area_min=0.3, chunk_rows=12, half=True)
    same_bits(bits_of(y, "f64"), bits_of(want, "f64"), f"apply_host {kind} -> f64 skipna")

    group, _, _, _, masked_levels = levels()
    lev = np.array([2, 0, 1], np.int32)
    xg = field(kind, (2, 3, 5, hc.N_SRC), seed=23)[0]                  # (n_outer, n_lev, n_inner, S)
    gkw = dict(masked=True, remap_area_min=0.3, out_dtype=NP_OF[kind])
    want = group.apply(to_device(xg), lev, masked_levels, **gkw).to_host().view(np.uint16)
    for flags in (0, _lib.APPLY_HOST_NO_PACK):
        _lib.host_stats(reset=True)
        y = group.apply_host(xg, lev, masked_levels, flags=flags, chunk_outer=1, half=True, **gkw)
        st = _lib.host_stats()
        same_bits(y.view(np.uint16), want, f"group apply_host {kind} flags={flags}")
        assert st["chunks"] >= 2
        assert st["d2h_bytes"] == 2 * want.size and st["h2d_bytes"] <= 2 * xg.size


def test_refusals(hip):
    op = single(70)[0]
    x = to_device(field("f16", (3, hc.N_SRC))[0])
    y = DeviceArray((3, 70), np.float32)

    def status(entry, *args):
        return getattr(hip.load(), entry)(*args), (hip.load().smm_last_error() or b"").decode()

    p = lambda a: ctypes.c_void_p(a.ptr)
    for yc in (hip.SMM_BF16, hip.SMM_F32):                             # F16 -> BF16, F16 -> F32: not built
        rc, msg = status("smm_apply", op.handle, p(x), hip.SMM_F16, hc.N_SRC, p(y), yc, 70, 3, 0.0, 0, None)
        assert rc == hip.SMM_ERR_UNSUPPORTED and "SMM_F16 / SMM_BF16" in msg and "not built" in msg
        rc, msg = status("smm_apply_sb", op.handle, p(x), hip.SMM_F16, 3, p(y), yc, 70, 3, 0.0, 0, None)
        assert rc == hip.SMM_ERR_UNSUPPORTED and "not built" in msg
    cf = hip.CfDecodeStruct(1.0, 0.0, (ctypes.c_int32 * 2)(0, 0), 0, hip.SMM_F32)
    rc, msg = status("smm_apply_cf", op.handle, p(x), hip.SMM_F16, hc.N_SRC, p(y), hip.SMM_F64, 70, 3, 0.0, 0, None,
                     ctypes.byref(cf))
    assert rc == hip.SMM_ERR_INVALID and "SMM_F16" in msg
    rc, msg = status("smm_apply_cf", op.handle, p(x), hip.SMM_I16, hc.N_SRC, p(y), hip.SMM_F16, 70, 3, 0.0, 0, None,
                     ctypes.byref(cf))
    assert rc == hip.SMM_ERR_INVALID
    enc = hip.CfEncodeStruct(1.0, 0.0, 0, 0)
    rc, msg = status("smm_apply_pk", op.handle, p(x), hip.SMM_F32, hc.N_SRC, p(y), hip.SMM_F16, 70, 3, 0.0, 0, None, None,
                     ctypes.byref(enc))
    assert rc == hip.SMM_ERR_INVALID
    rc, msg = status("smm_apply", op.handle, p(x), hip.SMM_F16, hc.N_SRC, p(y), hip.SMM_F64, 70, 3, 0.0,
                     hip.APPLY_KERNEL_TILE, None)
    assert rc == hip.SMM_ERR_UNSUPPORTED and "tile kernel" in msg
    assert op.launch_info(3, dtype=np.float16)["kernel"] == "sell" and op.launch_info(3, dtype=bfloat16)["kernel"] == "sell"
    with pytest.raises(TypeError, match="float16 -> float64"):         # the Python layer names the built pairs
        op.apply(x, out_dtype=np.float32)
    with pytest.raises(TypeError, match="is not built"):
        op.apply(x, out_dtype=bfloat16)


# ---------------------------------------------------------------- facade

def _weights2d():
    return gridgen.bilinear_weights("r36x18", "r12x7")


def _da(values, dims, src):
    coords = {"lat": src.lat, "lon": src.lon}
    return DataArray(values, dims=dims, coords=coords, name="tas")


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_regridder_half_on_2d_weights(hip, kind):
    w = _weights2d()
    src = gridgen.parse_grid("r36x18")
    bits = hc.half_field(kind, (5, 18, 36), seed=31)
    x, x32 = bits.view(NP_OF[kind]), hc.widen(bits, kind)
    for skipna in (False, True):
        ref = Regridder(weights=w, device=0, skipna=skipna).regrid(_da(x32, ("time", "lat", "lon"), src)).values
        out = Regridder(weights=w, device=0, half=True, skipna=skipna).regrid(_da(x, ("time", "lat", "lon"), src))
        assert out.values.dtype == NP_OF[kind] and out.shape == (5, 7, 12)
        same_bits(out.values.view(np.uint16), narrow(ref, kind), f"half=True {kind} skipna={skipna}")
        out = Regridder(weights=w, device=0, half=True, out_dtype=np.float64, skipna=skipna).regrid(
            _da(x, ("time", "lat", "lon"), src))
        assert out.values.dtype == F64
        same_bits(bits_of(out.values, "f64"), bits_of(ref, "f64"), f"half=True {kind} -> float64 skipna={skipna}")
    # a float32 field into a half result
    out = Regridder(weights=w, device=0, out_dtype=NP_OF[kind]).regrid(_da(x32, ("time", "lat", "lon"), src))
    ref = Regridder(weights=w, device=0).regrid(_da(x32, ("time", "lat", "lon"), src)).values
    same_bits(out.values.view(np.uint16), narrow(ref, kind), f"float32 -> {kind}")
    # device-resident, both layouts, no switch needed
    ref = Regridder(weights=w, device=0).regrid(_da(x32, ("time", "lat", "lon"), src)).values
    out = Regridder(weights=w, device=0).regrid(_da(to_device(x), ("time", "lat", "lon"), src))
    assert isinstance(out.data, DeviceArray) and out.data.dtype == F64
    same_bits(bits_of(out.data.to_host(), "f64"), bits_of(ref, "f64"), f"device {kind} -> float64")
    xsb = to_device(np.ascontiguousarray(x.transpose(1, 2, 0)), layout="sb")
    out = Regridder(weights=w, device=0, half=True, keep_batch_fastest=True).regrid(_da(xsb, ("lat", "lon", "time"), src))
    assert out.data.layout == "sb" and out.data.dtype == NP_OF[kind] and out.shape == (7, 12, 5)
    same_bits(out.data.to_host().view(np.uint16).transpose(2, 0, 1), narrow(ref, kind), f"device sb {kind}, kept batch-fastest")
    with pytest.raises(TypeError, match="is not built"):
        Regridder(weights=w, device=0, out_dtype=np.float32).regrid(_da(to_device(x), ("time", "lat", "lon"), src))


def test_regridder_keeps_promoting_host_float16_without_the_switch(hip):
    w = _weights2d()
    src = gridgen.parse_grid("r36x18")
    x = hc.half_field("f16", (3, 18, 36), seed=33).view(np.float16)
    out = Regridder(weights=w, device=0).regrid(_da(x, ("time", "lat", "lon"), src))
    ref = Regridder(weights=w, device=0).regrid(_da(x.astype(np.float64), ("time", "lat", "lon"), src))
    assert out.values.dtype == F64
    same_bits(bits_of(out.values, "f64"), bits_of(ref.values, "f64"), "host float16 without half=True")
    with pytest.raises(ValueError, match="out_dtype must be float32 or float64"):
        Regridder(weights=w, device=0, out_dtype=np.int16)


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_regridder_half_on_masked_level_weights(hip, kind):
    levs = np.array([5.0, 50.0, 500.0])
    src = gridgen.parse_grid("r36x18")
    bits = hc.half_field(kind, (2, 3, 18, 36), seed=43)
    x, x32 = bits.view(NP_OF[kind]), hc.widen(bits, kind)
    # a level-dependent land mask in the weights: built through the project's own 3-D generator on a masked sample
    from smmregrid_amd import CdoGenerate
    sample = np.ones((1, 3, 18, 36))
    sample[0, 1, :6] = np.nan
    sample[0, 2, :, :9] = np.nan
    da = DataArray(sample, dims=("time", "lev", "lat", "lon"),
                   coords={"time": np.arange(1), "lev": levs, "lat": src.lat, "lon": src.lon}, name="thetao")
    w3 = CdoGenerate(da, "r12x7").weights(method="con", mask_dim="lev")

    def field_of(v):
        return DataArray(v, dims=("time", "lev", "lat", "lon"),
                         coords={"time": np.arange(2), "lev": levs, "lat": src.lat, "lon": src.lon}, name="thetao")
    ref = Regridder(weights=w3, device=0).regrid(field_of(x32)).values
    out = Regridder(weights=w3, device=0, half=True).regrid(field_of(x))
    assert out.values.dtype == NP_OF[kind] and out.shape == ref.shape
    same_bits(out.values.view(np.uint16), narrow(ref, kind), f"3-D weights, host {kind}")
    out = Regridder(weights=w3, device=0, half=True, out_dtype=np.float64).regrid(field_of(x))
    same_bits(bits_of(out.values, "f64"), bits_of(ref, "f64"), f"3-D weights, host {kind} -> float64")
    out = Regridder(weights=w3, device=0, half=True).regrid(field_of(to_device(x)))
    same_bits(out.data.to_host().view(np.uint16), narrow(ref, kind), f"3-D weights, device {kind}")


def test_half_does_not_mix_with_packed_or_mixed_chunks(hip):
    w = _weights2d()
    src = gridgen.parse_grid("r36x18")
    q = np.arange(3 * 18 * 36, dtype=np.int16).reshape(3, 18, 36)
    da = _da(q, ("time", "lat", "lon"), src)
    da.attrs.update(scale_factor=0.5, add_offset=1.0, _FillValue=np.int16(-32768))
    with pytest.raises(ValueError, match="half-precision out_dtype"):
        Regridder(weights=w, device=0, packed=True, out_dtype=np.float16).regrid(da)
    # a lazy field that promised float16 and delivers another dtype
    from smmregrid_amd.lazy import LazyArray
    lazy = LazyArray((3, 18, 36), np.float16, lambda: np.zeros((3, 18, 36), np.float32))
    with pytest.raises(ValueError, match="a chunk of dtype float32"):
        Regridder(weights=w, device=0, half=True).regrid(_da(lazy, ("time", "lat", "lon"), src)).values


def test_from_interface_round_trip(hip):
    for dtype in (np.float16, np.float32, np.float64):
        host = np.arange(24, dtype=dtype).reshape(4, 6)
        owner = to_device(host)
        view = DeviceArray.from_interface(owner)
        assert view.ptr == owner.ptr and view.shape == (4, 6) and view.dtype == np.dtype(dtype) and view.base is owner
        assert np.array_equal(view.to_host(), host)
        view.copy_from_host(host + 1)
        assert np.array_equal(owner.to_host(), host + 1)           # the same memory
        view.free()
        assert owner.ptr != 0
    # a foreign half tensor regrids as it is
    op = single(70)[0]
    x = field("f16", (3, hc.N_SRC))[0]
    owner = to_device(x)
    y = op.apply(DeviceArray.from_interface(owner), out_dtype=np.float16).to_host()
    same_bits(y.view(np.uint16), narrow(expected(70, "f16", 3, False, False, 0.0), "f16"), "from_interface")
