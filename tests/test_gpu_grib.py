"""GRIB simple-packed fields regridded raw (smm_apply_grib, smm_apply_host_grib, `Regridder(packed=True)` on a file opened
with decode=False): every result is compared bit for bit -- uint64 views, NaNs included -- with smm_apply on the float32
field a host decode gives (SMM_F32 X, SMM_APPLY_KERNEL_SELL), which is also checked against the oracle.  The fields are
built from chosen integers (tests/grib_cases.py): q = 0 / all ones / random, every width of the list, byte offsets of all
four residues, rows out of buffer order, a row ending exactly at x_bytes with x_bytes % 4 != 0."""
import ctypes
import os

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import CdoGenerate, GribField, Regridder, SparseOperator, _lib, pinned_empty, to_device
from smmregrid_amd.io import open_dataset
from smmregrid_amd.lazy import LazyArray
from tests import grib_cases
from tests.grib_cases import WIDTHS
from tests.test_griblite import encode, encode2

pytestmark = pytest.mark.gpu
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f"{what}: {int(diff.sum())} results differ in their bits, first at {np.argwhere(diff)[:3].tolist()}"


_OPS = {}


def operator(name):
    """(operator, csr, dst_imask, dst_frac): the two goldens and a tiny hand-made operator with a row without links and
    an n_dst that is no multiple of 64."""
    if name not in _OPS:
        if name == "tiny":
            rng = np.random.default_rng(3)
            n_src, n_dst = 37, 70
            dst = np.repeat(np.arange(1, n_dst + 1), 3)
            dst = dst[dst != 6]                                    # destination row 6 has no links
            src = rng.integers(1, n_src + 1, size=dst.size)
            src[:3] = (1, n_src, n_src)                            # the first and the last source cell, a duplicate
            w = rng.random(dst.size)
            imask = (rng.random(n_dst) > 0.2).astype(np.int32)
            frac = rng.random(n_dst)
        else:
            z = np.load(os.path.join(GOLDEN, name + ".npz"))
            n_src, n_dst = int(z["n_src"]), int(z["n_dst"])
            src, dst, w = z["src_address"], z["dst_address"], z["remap_matrix"]
            imask, frac = z["dst_imask"], z["dst_frac"]
        op = SparseOperator(n_src, n_dst, src, dst, w, device=0)
        op.set_epilogue(imask, frac)
        _OPS[name] = (op, oracle.coo_to_csr_c(n_src, n_dst, src, dst, w), imask, frac)
    return _OPS[name]


def expected(name, field, masked=False, area_min=0.0):
    """smm_apply with SMM_F32 X and the SELL kernel on the host-decoded field -- after it has been tied to the oracle."""
    op, csr, imask, frac = operator(name)
    want = op.apply(to_device(field), masked=masked, remap_area_min=area_min, flags=_lib.APPLY_KERNEL_SELL).to_host()
    ref = oracle.apply_c(csr, field, masked=masked, dst_imask=imask, dst_frac=frac, area_min=area_min)
    assert np.array_equal(np.isnan(want), np.isnan(ref)) and np.array_equal(want[~np.isnan(ref)], ref[~np.isnan(ref)])
    return want


def device_bytes(buf):
    """The packed bytes in HBM: an allocation of x_bytes rounded up to 4 (the tail holds garbage, not zeros)."""
    padded = np.full((buf.size + 3) // 4 * 4, 0xA5, dtype=np.uint8)
    padded[:buf.size] = buf
    return to_device(padded)


def run_grib(name, buf, rows, masked=False, area_min=0.0):
    op = operator(name)[0]
    return op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, masked=masked, remap_area_min=area_min).to_host()


def check_all(name, buf, rows, field, what):
    """plain, and with SMM_APPLY_MASKED and remap_area_min > 0 on the operator's dst_imask / dst_frac"""
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        same_bits(run_grib(name, buf, rows, masked, area_min), expected(name, field, masked, area_min),
                  f"{what} masked={masked} area_min={area_min}")


@pytest.mark.parametrize("nbits", WIDTHS)
@pytest.mark.parametrize("name", ["bil_r180x90_r90x45", "ragged_random"])
def test_apply_grib_matches_apply_on_the_decoded_field(hip, name, nbits):
    """One width per case, n_batch 1 / 5 / 9 (the tails of the 4 rows a thread holds), per-row ref / E / offset residue,
    rows not in buffer order, D cycling through 0 / 2 / -1 from five rows on."""
    rng = np.random.default_rng(1000 + nbits)
    S = operator(name)[0].n_src
    for n_batch in (1, 5, 9):
        specs = grib_cases.row_specs(rng, S, n_batch, (nbits,), D=(0,) if n_batch == 1 else (0, 2, -1))
        buf, rows, field = grib_cases.build(specs, rng, tail_residue=1 + n_batch % 3)
        assert buf.size % 4 != 0 or nbits == 0
        assert np.isfinite(field).all()
        check_all(name, buf, rows, field, f"{name} nbits={nbits} B={n_batch}")


@pytest.mark.parametrize("name", ["bil_r180x90_r90x45", "ragged_random", "tiny"])
def test_mixed_widths_in_one_call_with_a_constant_row(hip, name):
    rng = np.random.default_rng(5)
    S = operator(name)[0].n_src
    specs = grib_cases.row_specs(rng, S, 11, (16, 0, 12, 32, 1, 25, 7, 0, 31, 17, 24), D=(0, 0, 1, -1))
    buf, rows, field = grib_cases.build(specs, rng, tail_residue=3)
    assert set(rows["nbits"].tolist()) == {16, 0, 12, 32, 1, 25, 7, 31, 17, 24} and buf.size % 4 == 3
    assert len(set((rows["byte_off"] % 4).tolist())) == 4 and (np.diff(rows["byte_off"].astype(np.int64)) < 0).any()
    check_all(name, buf, rows, field, f"{name} mixed")
    # only constant fields: not one data byte
    const = [dict(q=np.zeros(S, np.uint64), nbits=0, E=3, D=1, ref=-7.25, residue=0) for _ in range(3)]
    buf0, rows0, field0 = grib_cases.build(const, rng)
    assert buf0.size == 0 and (field0 == np.float32(-0.725)).all()
    op = operator(name)[0]
    got = op.apply_grib(0, rows0, x_bytes=0).to_host()
    same_bits(got, expected(name, field0), f"{name} constant rows, no bytes")


def test_both_instantiations_on_the_same_integers(hip):
    """All ddiv == 1 runs the kernel without the division, one row with D != 0 the kernel with it: on the same q, the
    rows with D = 0 have the same bits either way."""
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(6)
    S = operator(name)[0].n_src
    specs = grib_cases.row_specs(rng, S, 6, (16, 12, 25), D=(0,))
    buf, rows, field = grib_cases.build(specs, rng)
    assert (rows["ddiv"] == 1.0).all()
    nodiv = run_grib(name, buf, rows)
    same_bits(nodiv, expected(name, field), "DIV = false")
    mixed = [dict(s, D=(0, 2, 0, -1, 0, 0)[i]) for i, s in enumerate(specs)]
    buf2, rows2, field2 = grib_cases.build(mixed, rng)
    assert set(rows2["ddiv"].tolist()) == {1.0, 100.0, 0.1}
    div = run_grib(name, buf2, rows2)
    same_bits(div, expected(name, field2), "DIV = true")
    same_bits(div[[0, 2, 4, 5]], nodiv[[0, 2, 4, 5]], "rows with D = 0 under either instantiation")


def test_a_page_locked_row_table_may_be_reused_on_return(hip):
    """`rows` in page-locked memory: an asynchronous copy would read it after the call has returned.  The table is
    overwritten right after the call, on a stream that is kept busy in front of it; the bits are the pageable call's."""
    from smmregrid_amd.device import Stream
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(13)
    op = operator(name)[0]
    buf, rows, field = grib_cases.build(grib_cases.row_specs(rng, op.n_src, 9, (16, 12, 7)), rng)
    want = run_grib(name, buf, rows)
    same_bits(want, expected(name, field), "pageable table")
    pinned = pinned_empty(rows.size * 40, np.uint8).view(grib_cases.GRIB_ROW_DTYPE)
    x = device_bytes(buf)
    stream = Stream()
    big = to_device(np.zeros(1 << 24))
    for _ in range(8):                                  # copies queued in front of the table's upload
        _lib.call("smm_memcpy_d2d", ctypes.c_void_p(big.ptr), ctypes.c_void_p(big.ptr + big.nbytes // 2), big.nbytes // 2,
                  stream.handle)
    pinned[:] = rows
    y = op.apply_grib(x, pinned, x_bytes=buf.size, stream=stream)
    pinned[:] = np.zeros(rows.size, grib_cases.GRIB_ROW_DTYPE)       # a table of nonsense: nbits 0, bscale 0
    stream.synchronize()
    same_bits(y.to_host(), want, "page-locked table overwritten on return")


def test_adversarial_values_subnormals_overflow_and_ties(hip):
    name = "ragged_random"
    rng = np.random.default_rng(8)
    S = operator(name)[0].n_src
    q32, q25, q16 = (grib_cases.random_q(rng, S, n) for n in (32, 25, 16))
    specs = [dict(q=q16, nbits=16, E=-140, D=0, ref=0.0, residue=1),          # float32 subnormals, produced and kept
             dict(q=q32, nbits=32, E=100, D=0, ref=-1.0e30, residue=2),       # beyond float32: inf -> fill -> NaN results
             dict(q=q32, nbits=32, E=0, D=0, ref=0.0, residue=3),             # float64 -> float32 ties
             dict(q=q25, nbits=25, E=0, D=0, ref=0.0, residue=0),
             dict(q=q16, nbits=16, E=-3, D=2, ref=-273.15, residue=1)]        # negative ref, D = 2
    buf, rows, field = grib_cases.build(specs, rng, tail_residue=2)
    tiny = np.abs(field[0][field[0] != 0])
    assert tiny.size and (tiny < np.finfo(np.float32).tiny).any()          # subnormals among them
    assert np.isinf(field[1]).any() and np.isfinite(field[1]).any()
    odd = (q25 > (1 << 24)) & (q25 % 2 == 1)
    assert odd.any() and (field[3][odd].astype(np.float64) != q25[odd].astype(np.float64)).all()     # ties were rounded
    want = expected(name, field)
    assert np.isnan(want[1]).any() and not np.isnan(want[0]).any() and (want[0] != 0).any()
    same_bits(run_grib(name, buf, rows), want, "adversarial")
    same_bits(run_grib(name, buf, rows, True, 0.5), expected(name, field, True, 0.5), "adversarial, masked")


def test_refusals_that_need_the_operator(hip):
    op = operator("tiny")[0]
    rng = np.random.default_rng(9)
    buf, rows, _ = grib_cases.build(grib_cases.row_specs(rng, op.n_src, 2, (12,)), rng)
    x, y = device_bytes(buf), np.zeros((2, op.n_dst))
    lib = _lib.load()
    rp = ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))
    yd = to_device(y)

    def device(x_bytes, ldy, handle=op.handle):
        return lib.smm_apply_grib(handle, ctypes.c_void_p(x.ptr), x_bytes, rp, ctypes.c_void_p(yd.ptr), _lib.SMM_F64, ldy, 2,
                                  0.0, 0, None)

    def host(x_bytes, ldy, handle=op.handle):
        return lib.smm_apply_host_grib(handle, buf.ctypes.data, x_bytes, rp, y.ctypes.data, _lib.SMM_F64, ldy, 2, 0.0, 0, 0)

    for fn in (device, host):
        # the row laid last ends exactly at x_bytes: one byte less and it leaves the buffer
        assert fn(buf.size - 1, op.n_dst) == _lib.SMM_ERR_INVALID and b"leave the buffer" in lib.smm_last_error()
        assert fn(buf.size, op.n_dst - 1) == _lib.SMM_ERR_INVALID and b"ldy" in lib.smm_last_error()
        assert fn(buf.size, op.n_dst, None) == _lib.SMM_ERR_INVALID and b"null operator" in lib.smm_last_error()
        assert fn(buf.size, op.n_dst) == _lib.SMM_OK
    assert (y == yd.to_host()).all() and not (y == 0).all()


# ---------------------------------------------------------------------------------------------- host pipeline

def host_case():
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(10)
    S = operator(name)[0].n_src
    specs = grib_cases.row_specs(rng, S, 7, (16, 12, 0, 24, 17, 7, 32), D=(0, 1))
    buf, rows, field = grib_cases.build(specs, rng, tail_residue=1)
    return name, buf, rows, field


def staged_bytes(rows, S):
    return int(sum(40 + ((S * int(n) + 7) // 8 + 3) // 4 * 4 for n in rows["nbits"]))


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("chunk_rows", [0, 1, 3])
def test_apply_host_grib_has_the_bits_of_the_device_entry(hip, pinned, chunk_rows):
    name, buf, rows, field = host_case()
    op = operator(name)[0]
    S, D = op.n_src, op.n_dst
    x_host = buf
    if pinned:
        x_host = pinned_empty(buf.size, np.uint8)
        x_host[:] = buf
    want = run_grib(name, buf, rows, True, 0.5)
    same_bits(want, expected(name, field, True, 0.5), "device entry")
    _lib.host_stats(reset=True)
    got = op.apply_host_grib(x_host, rows, masked=True, remap_area_min=0.5, chunk_rows=chunk_rows)
    st = _lib.host_stats(reset=True)
    same_bits(got, want, f"host entry pinned={pinned} chunk_rows={chunk_rows}")
    assert st["calls"] == 1 and st["chunks"] == {0: 1, 1: 7, 3: 3}[chunk_rows]
    # deterministic counts: every row's data bytes rounded up to 4 plus a 40-B table record per row; the f64 result
    assert st["h2d_bytes"] == staged_bytes(rows, S) and st["d2h_bytes"] == 7 * D * 8
    # ldy > D, into pinned and pageable Y
    for y in (np.full((7, D + 3), -1.0), pinned_empty((7, D + 3), np.float64)):
        y[:] = -1.0
        _lib.call("smm_apply_host_grib", op.handle, x_host.ctypes.data, buf.size,
                  ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)), y.ctypes.data, _lib.SMM_F64, D + 3, 7,
                  0.5, _lib.APPLY_MASKED, chunk_rows)
        same_bits(np.ascontiguousarray(y[:, :D]), want, "ldy > D")
        assert (y[:, D:] == -1.0).all()


def test_a_failed_chunk_drains_the_pipeline_and_the_next_call_succeeds(hip):
    name, buf, rows, field = host_case()
    op = operator(name)[0]
    want = expected(name, field)
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        with pytest.raises(_lib.SmmError, match="injected failure"):
            op.apply_host_grib(buf, rows, chunk_rows=3)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    same_bits(op.apply_host_grib(buf, rows, chunk_rows=3), want, "after the injected failure")


# ---------------------------------------------------------------------------------------------- Regridder

def grib1_16bit(tmp_path, rng):
    ni, nj = 36, 18
    lat = 85.0 - 10.0 * np.arange(nj)
    msgs = [encode(250.0 + 30.0 * np.cos(np.radians(lat))[:, None] + rng.standard_normal((nj, ni)) + day,
                   0, ni, nj, 85, 0, -85, 350, 10000, param=167, date=(2021, 3, day, 12), nbits=16) for day in (1, 2, 3)]
    path = tmp_path / "t2m.grib"
    path.write_bytes(b"".join(msgs))
    return str(path), "t2m"


def grib2_12bit(tmp_path, rng):
    ni, nj = 36, 18
    grid = dict(template=0, ni=ni, nj=nj, la1=85.0, lo1=0.0, la2=-85.0, lo2=350.0, n_or_dj=10000000)
    msgs = [encode2([dict(values=220.0 + 30 * rng.random((nj, ni)) + lev / 1e4, category=0, number=0, surface=(100, lev),
                          nbits=12, decimal=1, step=step) for lev in (85000, 50000)], **grid) for step in (0, 6)]
    path = tmp_path / "t.grib2"
    path.write_bytes(b"".join(msgs))
    return str(path), "t"


def same_arrays(got, want, what):
    same_bits(np.asarray(got.values), np.asarray(want.values), what)
    assert got.dims == want.dims and got.attrs == want.attrs and got.name == want.name, what
    assert list(got.coords) == list(want.coords), what
    for k in got.coords:
        assert np.array_equal(got.coords[k].values, want.coords[k].values), (what, k)


@pytest.mark.parametrize("make", [grib1_16bit, grib2_12bit])
def test_regridder_ships_a_grib_file_raw(hip, tmp_path, caplog, make):
    path, var = make(tmp_path, np.random.default_rng(11))
    dec, raw = open_dataset(path), open_dataset(path, decode=False)
    assert isinstance(raw[var].data, GribField) and raw[var].data.rows.size == (3 if var == "t2m" else 4)
    w = CdoGenerate(dec[var], "r12x6").weights(method="con")
    want = Regridder(weights=w).regrid(dec)
    caplog.clear()                                       # the weights generator has its own say about cdo
    assert want[var].dtype == np.float64 and np.isfinite(want[var].values).any()
    _lib.host_stats(reset=True)
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, loglevel="INFO").regrid(raw)
    st = _lib.host_stats(reset=True)
    assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
    rows = raw[var].data.rows
    assert st["calls"] == 1 and st["h2d_bytes"] == staged_bytes(rows, 36 * 18)        # the raw bits crossed PCIe
    assert list(got.data_vars) == list(want.data_vars) and got.attrs == want.attrs
    same_arrays(got[var], want[var], "packed=True on the raw file")
    # packed_out does not apply (no CF attributes): float64, no warning
    caplog.clear()
    with caplog.at_level("INFO"):
        out = Regridder(weights=w, packed=True, packed_out=True, loglevel="INFO").regrid(raw)
    assert not [r for r in caplog.records if r.levelname == "WARNING" or "packed" in r.getMessage()]
    same_arrays(out[var], want[var], "packed_out")
    # without packed=True everything is as before, through np.asarray
    same_arrays(Regridder(weights=w).regrid(raw)[var], want[var], "packed=False")
    # lazy
    lazy = Regridder(weights=w, packed=True, lazy=True).regrid(raw)[var]
    assert isinstance(lazy.data, LazyArray)
    same_bits(np.asarray(lazy.values), want[var].values, "lazy")
    # the fallbacks decode on the host with one INFO line each and give the bits of today
    for kw, word in ((dict(skipna=True), "skipna"), (dict(out_dtype=np.float32), "out_dtype float32")):
        caplog.clear()
        with caplog.at_level("INFO"):
            fb = Regridder(weights=w, packed=True, loglevel="INFO", **kw).regrid(raw)[var]
        lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
        assert len(lines) == 1 and word in lines[0], lines
        ref = Regridder(weights=w, **kw).regrid(dec)[var]
        assert fb.dtype == ref.dtype and np.array_equal(fb.values.view(np.uint8), ref.values.view(np.uint8)), word


def test_regridder_masked_levels_decode_on_the_host(hip, tmp_path, caplog):
    path, var = grib2_12bit(tmp_path, np.random.default_rng(12))
    dec, raw = open_dataset(path), open_dataset(path, decode=False)
    w3 = CdoGenerate(dec[var], "r12x6").weights(method="con", mask_dim="isobaricInhPa")
    want = Regridder(weights=w3).regrid(dec[var])
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w3, packed=True, loglevel="INFO").regrid(raw[var])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "masked levels" in lines[0]
    same_arrays(got, want, "masked levels")
