"""CF-packed int16 / uint16 RESULTS (`cf_out=`, `Regridder(packed_out=True)`, the `_pk` entries).  Every comparison is
bit equality against `CFEncode.encode` of the float64 result of the existing entry on the same inputs -- a result the
other GPU tests pin to the CPU oracle.

The fields are built in the arithmetic of the encode rule.  With dyadic scales and offsets the decoded source values
are multiples of 1/8 and the encoded t = (y - offset) / scale is a half-integer wherever a result equals a source value
(config 2's bilinear weights are 1 and 0: every second result is a tie) and on one batch row whose sources decode to
exactly 0 (t = n + 0.5 on every geometry).  The values are plateaus over the whole raw range, placed so that one to
three per cent of the results round beyond its upper end; fill values on a rectangle and scattered cells, the static mask
and remap_area_min make NaN.
Non-dyadic rules and values that tell a wrong division or rounding apart: tests/test_gpu_packed_out_exact.py."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (CdoGenerate, CFDecode, CFEncode, DataArray, Dataset, Regridder, SparseOperator, _lib, gridgen,
                           pinned_empty, to_device)
from smmregrid_amd.lazy import LazyArray

pytestmark = pytest.mark.gpu
PACKING = ("scale_factor", "add_offset", "_FillValue", "missing_value")

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


def check_expectation(y64, enc, what, need_nan=True):
    """The float64 expectation must exercise the rule: ties, overflow (a small share, but present), NaN."""
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
    if need_nan:
        assert 0.01 <= nan <= 0.6, (what, nan)
    return ties, over, nan


# ---------------------------------------------------------------- operators and fields

def _op_of(w):
    op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                        w["dst_address"].values, w["remap_matrix"].values, device=0)
    return op, (w["dst_grid_frac"].values if "dst_grid_frac" in w else None)


def _banded_scattered(rng, nx=500, ny=200, n_dst=1500, k=12, band=4):
    """Every row draws its links anywhere inside a band of `band` source latitudes of its own: plans the SELL kernel."""
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
    """(operator, dst_frac or None, dst_imask, (ny, nx) of the source, batch): built once per session."""
    if name not in _OPS:
        rng = np.random.default_rng(20261016)
        if name == "cfg2":          # config-2 geometry at a reduced, odd batch (two batch tiles of kernel C, one ragged)
            op, frac = _op_of(gridgen.bilinear_weights("r1440x721", "r360x180"))
            shape, batch = (721, 1440), 131
        elif name == "con":         # conservative, 9 links per row, with dst_frac
            op, frac = _op_of(gridgen.conservative_weights("r144x72", "r48x24"))
            shape, batch = (72, 144), 37
        elif name == "odd":         # n_dst = 648: no multiple of 16 or 64 rows (ragged last tile of kernels A and C)
            op, frac = _op_of(gridgen.bilinear_weights("r143x71", "r36x18"))
            shape, batch = (71, 143), 203
        else:                       # scattered: plans SELL
            op, frac = _banded_scattered(rng), None
            shape, batch = (200, 500), 21
        imask = (rng.random(op.n_dst) > 0.1).astype(np.int32)          # 10 % masked rows
        op.set_epilogue(imask, frac)
        _OPS[name] = (op, frac, imask, shape, batch)
    return _OPS[name]


def raw_field(rng, raw, batch, shape, k_max):
    """Raw source values (batch, ny * nx): eight latitude bands per batch row, each a plateau drawn from the whole raw
    range plus a few counts of noise, so that averaging stencils keep the spread; one band in a hundred sits in the top
    300 counts, whose results round beyond the raw range.  Batch row 0 decodes to 0.0 everywhere.  The fill values
    cover a rectangle of ~5 % of the cells plus scattered cells at a rate of 0.03 / k_max (a fill under a small weight stays below the 1e19
    threshold of the epilogue: such a result is huge, not NaN, and must come out as the fill value too)."""
    info = np.iinfo(raw)
    _, _, q_zero, fills = RULES[np.dtype(raw)]
    ny, nx = shape
    nb = 8
    band = np.arange(ny) // -(-ny // nb)
    vals = rng.integers(info.min, info.max + 1, size=(batch, nb))
    top = (np.arange(batch)[:, None] * nb + np.arange(nb)[None, :]) % 100 == 7
    vals[top] = info.max - rng.integers(0, 300, size=int(top.sum()))
    q = vals[:, band][:, :, None] + rng.integers(-3, 4, size=(batch, ny, nx))
    q = np.clip(q, info.min, info.max).astype(raw)
    q[0] = q_zero
    for f in fills:
        q[q == f] = f + 1 if f < info.max else f - 1
    hy = max(1, int(round(0.05 * ny)))
    q[:, ny // 3:ny // 3 + hy, :] = fills[0]
    scattered = rng.random(q.shape) < 0.03 / k_max
    q[scattered] = np.where(rng.random(int(scattered.sum())) < 0.5, fills[0], fills[-1]).astype(raw)
    return q.reshape(batch, ny * nx)


def x_of(q, kind):
    """The field one case regrids, and the CFDecode that goes with it (None for float X): kind f32 / f64 -- the host
    decode in that type; pf32 / pf64 -- the raw integers, decoded in the kernels."""
    cf = dec_rule(q.dtype, np.float32 if kind.endswith("32") else np.float64)
    return (q, cf) if kind.startswith("p") else (cf.decode(q), None)


EPILOGUES = [(False, 0.0), (True, 0.0), (True, 0.5)]
XKINDS = ["f32", "f64", "pf32", "pf64"]


@pytest.mark.parametrize("kind", XKINDS)
@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
@pytest.mark.parametrize("name", ["cfg2", "con", "scattered"])
def test_kernels_a_and_c_equal_encode_of_the_float64_result(hip, name, raw, kind):
    op, frac, imask, shape, batch = operator(name)
    rng = np.random.default_rng(7 + batch)
    enc = enc_rule(raw)
    q = raw_field(rng, raw, batch, shape, op.max_row_nnz)
    x, cf = x_of(q, kind)
    if name == "scattered":
        assert not op.plan_info()["tile_preferred"]
    dx = to_device(x)
    dxt = to_device(np.ascontiguousarray(x.T), layout="sb")
    dxp = to_device(np.ascontiguousarray(x.T[op.used_sources()]))
    for masked, area_min in EPILOGUES:
        if area_min > 0.0 and frac is None:
            continue
        for skipna in (False, True):
            kw = dict(masked=masked, remap_area_min=area_min, skipna=skipna, cf=cf)
            what = f"{name} {kind}->{np.dtype(raw).name} masked={masked} area_min={area_min} skipna={skipna}"
            y64 = op.apply(dx, **kw).to_host()                       # the existing entry, float64
            check_expectation(y64, enc, what, need_nan=masked or not skipna)
            want = enc.encode(y64)
            got = op.apply(dx, cf_out=enc, **kw)
            assert got.dtype == np.dtype(raw) and got.shape == (batch, op.n_dst)
            same_bits(got.to_host(), want, what + " kernel A")
            same_bits(op.apply(dx, cf_out=enc, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host(), want, what + " forced SELL")
            same_bits(op.apply(dxt, cf_out=enc, **kw).to_host(), want, what + " kernel C")
            same_bits(op.apply_sb(dxp, packed=True, cf_out=enc, **kw).to_host(), want, what + " kernel C SB_PACKED")
            kept = op.apply_sb(dxt, keep_batch_fastest=True, cf_out=enc, **kw)
            assert kept.layout == "sb" and kept.shape == (op.n_dst, batch) and kept.dtype == np.dtype(raw)
            same_bits(kept.to_host(), np.ascontiguousarray(want.T), what + " kernel C Y_SB")
            with _lib.tuning(sb_packed_y_rows=16):                   # the other tile height of kernel C
                same_bits(op.apply(dxt, cf_out=enc, **kw).to_host(), want, what + " kernel C, 16-row tiles")
                same_bits(op.apply_sb(dxt, keep_batch_fastest=True, cf_out=enc, **kw).to_host(),
                          np.ascontiguousarray(want.T), what + " kernel C Y_SB, 16-row tiles")


@pytest.mark.parametrize("raw,kind", [(np.int16, "pf32"), (np.uint16, "f64")])
def test_tiny_odd_and_ragged_batches(hip, raw, kind):
    """Kernel C's element-wise walk (one batch entry), odd and ragged batches, and a destination grid that is no
    multiple of any tile height (648 rows)."""
    op, frac, imask, shape, _ = operator("odd")
    assert op.n_dst % 16 and op.n_dst % 64
    rng = np.random.default_rng(5)
    enc = enc_rule(raw)
    for batch in (1, 2, 3, 127, 129):
        q = raw_field(rng, raw, batch, shape, op.max_row_nnz)
        x, cf = x_of(q, kind)
        for skipna in (False, True):
            kw = dict(masked=True, skipna=skipna, cf=cf)
            want = enc.encode(op.apply(to_device(x), **kw).to_host())
            assert (want == enc.fill_value).any() and (want != enc.fill_value).any()
            same_bits(op.apply(to_device(x), cf_out=enc, **kw).to_host(), want, f"A B={batch}")
            xt = to_device(np.ascontiguousarray(x.T))
            for rows in (0, 16):
                with _lib.tuning(sb_packed_y_rows=rows):
                    same_bits(op.apply_sb(xt, cf_out=enc, **kw).to_host(), want, f"C B={batch} rows={rows}")
                    same_bits(op.apply_sb(xt, keep_batch_fastest=True, cf_out=enc, **kw).to_host(),
                              np.ascontiguousarray(want.T), f"C Y_SB B={batch} rows={rows}")


@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_padded_pitch_keeps_its_sentinel_and_y_needs_two_byte_alignment_only(hip, raw):
    """ldy beyond a row of Y, a Y base that is only 2-byte aligned: the raw entries write the results and nothing else."""
    op, frac, imask, shape, _ = operator("odd")
    lib = _lib.load()
    rng = np.random.default_rng(13)
    enc, B, D, pad = enc_rule(raw), 67, op.n_dst, 3
    q = raw_field(rng, raw, B, shape, op.max_row_nnz)
    cf = dec_rule(raw, np.float32)
    want = enc.encode(op.apply(to_device(q), masked=True, cf=cf).to_host())
    sentinel = np.dtype(raw).type(12345)
    assert not (want == sentinel).all()
    st, est = cf._struct(q.dtype), enc._struct()
    code = _lib.SMM_I16 if raw == np.int16 else _lib.SMM_U16
    dq, dqt = to_device(q), to_device(np.ascontiguousarray(q.T))
    for entry, x, ldx, ldy, rows, flags in (("smm_apply_pk", dq, op.n_src, D + pad, B, 0),
                                            ("smm_apply_sb_pk", dqt, B, D + pad, B, 0),
                                            ("smm_apply_sb_pk", dqt, B, B + pad, D, _lib.APPLY_SB_Y_SB)):
        for rows_knob in (0, 16):
            buf = to_device(np.full(1 + rows * ldy, sentinel, raw))
            with _lib.tuning(sb_packed_y_rows=rows_knob):
                rc = getattr(lib, entry)(op.handle, ctypes.c_void_p(x.ptr), code, ldx, ctypes.c_void_p(buf.ptr + 2), code, ldy,
                                         B, 0.0, _lib.APPLY_MASKED | flags, None, ctypes.byref(st), ctypes.byref(est))
            assert rc == _lib.SMM_OK, lib.smm_last_error()
            host = buf.to_host()
            assert host[0] == sentinel
            got = host[1:].reshape(rows, ldy)
            same_bits(got[:, :ldy - pad], want.T if flags else want, f"{entry} flags={flags} rows={rows_knob}")
            assert (got[:, ldy - pad:] == sentinel).all(), f"{entry}: the padding of Y was written"
    # an odd Y address is refused
    buf = to_device(np.zeros(2 + B * D, raw))
    rc = lib.smm_apply_pk(op.handle, ctypes.c_void_p(dq.ptr), code, op.n_src, ctypes.c_void_p(buf.ptr + 1), code, D, B, 0.0,
                          0, None, ctypes.byref(st), ctypes.byref(est))
    assert rc == _lib.SMM_ERR_INVALID
    # a packed field produces results of its own raw type only
    other = _lib.SMM_U16 if raw == np.int16 else _lib.SMM_I16
    est2 = CFEncode(1.0, 0.0, 1, np.uint16 if raw == np.int16 else np.int16)._struct()
    rc = lib.smm_apply_pk(op.handle, ctypes.c_void_p(dq.ptr), code, op.n_src, ctypes.c_void_p(buf.ptr), other, D, B, 0.0,
                          0, None, ctypes.byref(st), ctypes.byref(est2))
    assert rc == _lib.SMM_ERR_UNSUPPORTED, lib.smm_last_error()


def test_lowered_grid_limit_splits_the_launches(hip):
    op, frac, imask, shape, _ = operator("odd")
    rng = np.random.default_rng(19)
    raw, B = np.int16, 300
    enc = enc_rule(raw)
    q = raw_field(rng, raw, B, shape, op.max_row_nnz)
    x, cf = x_of(q, "pf64")
    want = enc.encode(op.apply(to_device(x), masked=True, cf=cf).to_host())
    dx, dxt = to_device(x), to_device(np.ascontiguousarray(x.T))
    try:
        for limit in (11, 40):                # kernel C: 11 destination tiles of 64 rows, so one / three batch tiles a launch
            _lib.call("smm_debug_set_grid_limit", limit)
            same_bits(op.apply(dx, masked=True, cf=cf, cf_out=enc).to_host(), want, f"A limit {limit}")
            same_bits(op.apply_sb(dxt, masked=True, cf=cf, cf_out=enc).to_host(), want, f"C limit {limit}")
            same_bits(op.apply_sb(dxt, masked=True, cf=cf, cf_out=enc, keep_batch_fastest=True).to_host(),
                      np.ascontiguousarray(want.T), f"C Y_SB limit {limit}")
        _lib.call("smm_debug_set_grid_limit", 41)
        with _lib.tuning(sb_packed_y_rows=16):    # 41 destination tiles of 16 rows
            same_bits(op.apply_sb(dxt, masked=True, cf=cf, cf_out=enc).to_host(), want, "C 16-row tiles, limit 41")
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)


@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_chain_of_two_regrids_stays_packed(hip, raw):
    """apply_sb with SB_Y_SB and cf_out gives the int16 / uint16 batch-fastest field a second apply_sb(cf=) consumes."""
    op1, _, _, shape, _ = operator("odd")
    op2, frac2 = _op_of(gridgen.bilinear_weights("r36x18", "r18x9"))
    rng = np.random.default_rng(43)
    B = 130
    enc = enc_rule(raw)
    q = raw_field(rng, raw, B, shape, op1.max_row_nnz)
    cf1 = dec_rule(raw, np.float32)
    cf2 = CFDecode.from_attrs(enc.attrs(), dtype=np.float64, raw_dtype=raw)
    # the host statement of the chain
    y1 = enc.encode(op1.apply(to_device(cf1.decode(q)), masked=True).to_host())
    assert (y1 == enc.fill_value).any()
    want = op2.apply(to_device(cf2.decode(y1))).to_host()
    assert np.isnan(want).any() and np.isfinite(want).any()
    mid = op1.apply_sb(to_device(np.ascontiguousarray(q.T)), masked=True, keep_batch_fastest=True, cf=cf1, cf_out=enc)
    assert mid.dtype == np.dtype(raw) and mid.layout == "sb" and mid.shape == (op1.n_dst, B)
    got = op2.apply_sb(mid, cf=cf2).to_host()
    assert got.dtype == np.float64
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.array_equal(got[~np.isnan(got)], want[~np.isnan(want)])
    # ... and packed again at the end of the chain
    same_bits(op2.apply_sb(mid, cf=cf2, cf_out=enc).to_host(), enc.encode(want), "second hop packed")


# ---------------------------------------------------------------- host pipeline

@pytest.mark.parametrize("kind", ["pf32", "f64"])
@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_apply_host_brings_two_bytes_per_cell_back(hip, raw, kind):
    op, frac, imask, shape, B = operator("odd")
    assert op.n_used_src * 5 <= op.n_src * 4
    rng = np.random.default_rng(17)
    enc, D = enc_rule(raw), op.n_dst
    q = raw_field(rng, raw, B, shape, op.max_row_nnz)
    x, cf = x_of(q, kind)
    for skipna in (False, True):
        kw = dict(masked=True, skipna=skipna, cf=cf)
        y64 = op.apply_host(x, **kw)
        check_expectation(y64, enc, f"host {kind} skipna={skipna}")
        want = enc.encode(y64)
        for label, extra in (("packed", {}), ("packed chunk 48", {"chunk_rows": 48}),
                             ("whole rows", {"flags": _lib.APPLY_HOST_NO_PACK}),
                             ("whole rows chunk 50", {"flags": _lib.APPLY_HOST_NO_PACK, "chunk_rows": 50}),
                             ("forced SELL", {"flags": _lib.APPLY_KERNEL_SELL})):
            for pinned in (False, True):
                out = pinned_empty((B, D), raw) if pinned else np.empty((B, D), raw)
                out[...] = 12345
                _lib.host_stats(reset=True)
                got = op.apply_host(x, out=out, cf_out=enc, **kw, **extra)
                st = _lib.host_stats(reset=True)
                assert got is out
                same_bits(got, want, f"{label} pinned={pinned} skipna={skipna}")
                assert st["d2h_bytes"] == B * D * 2, (label, st)
                if "chunk_rows" in extra:
                    assert st["chunks"] == -(-B // extra["chunk_rows"]), (label, st)
        got = op.apply_host(x, cf_out=enc, **kw)                    # the library's own result buffer
        assert got.dtype == np.dtype(raw)
        same_bits(got, want, "own buffer")
        _lib.host_stats(reset=True)
        op.apply_host(x, **kw)
        assert _lib.host_stats(reset=True)["d2h_bytes"] == B * D * 8   # the float64 result: four times the bytes


@pytest.mark.parametrize("pinned", [False, True])
def test_apply_host_injected_chunk_failure_drains(hip, pinned):
    op, frac, imask, shape, B = operator("odd")
    rng = np.random.default_rng(23)
    raw, D, chunk, fail_at = np.int16, op.n_dst, 32, 3
    enc, cf = enc_rule(raw), dec_rule(raw, np.float64)
    q = raw_field(rng, raw, B, shape, op.max_row_nnz)
    want = enc.encode(op.apply_host(q, cf=cf))
    out = pinned_empty((B, D), raw) if pinned else np.empty((B, D), raw)
    out[...] = 12345
    _lib.call("smm_debug_fail_at_chunk", fail_at)
    try:
        with pytest.raises(_lib.SmmError) as e:
            op.apply_host(q, out=out, chunk_rows=chunk, cf=cf, cf_out=enc)
        assert "injected failure" in str(e.value)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    # what was enqueued before the failure has landed (direct DMA: chunks 0..c-1; staged copies: 0..c-2), the rest is
    # untouched
    done = fail_at * chunk if pinned else (fail_at - 1) * chunk
    got = np.array(out)
    same_bits(got[:done], want[:done], "delivered chunks")
    assert (got[fail_at * chunk:] == 12345).all()
    same_bits(op.apply_host(q, out=out, chunk_rows=chunk, cf=cf, cf_out=enc), want, "the next call works")


# ---------------------------------------------------------------- Regridder

def _packed_da(rng, raw=np.int16, nt=6, name="t2m", fill_attr=True):
    src = gridgen.parse_grid("r180x90")
    enc_off, dec_off, _, fills = RULES[np.dtype(raw)]
    q = raw_field(rng, raw, nt, (90, 180), 4).reshape(nt, 90, 180)
    # the variable's own rule does both jobs here: decode with it, encode with it
    attrs = {"scale_factor": ENC_SCALE, "add_offset": enc_off, "units": "K", "long_name": "2 metre temperature"}
    if fill_attr:
        attrs.update({"_FillValue": np.dtype(raw).type(fills[0]), "missing_value": np.dtype(raw).type(fills[1])})
    coords = {"time": np.arange(nt), "lat": src.lat, "lon": src.lon}
    return DataArray(q, dims=("time", "lat", "lon"), coords=coords, name=name, attrs=attrs)


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("raw", [np.int16, np.uint16], ids=["i16", "u16"])
def test_regridder_packed_out_equals_encode_after_regrid(hip, raw, skipna):
    rng = np.random.default_rng(29)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da = _packed_da(rng, raw)
    enc = CFEncode.from_attrs(da.attrs, raw)
    f64 = Regridder(weights=w, skipna=skipna, packed=True).regrid(da)            # today's path: float64
    assert f64.values.dtype == np.float64 and np.isnan(f64.values).any()
    want = enc.encode(f64.values)
    assert (want != enc.fill_value).any()
    rg = Regridder(weights=w, skipna=skipna, packed=True, packed_out=True)
    got = rg.regrid(da)
    assert got.values.dtype == np.dtype(raw) and got.dims == f64.dims
    same_bits(got.values, want, "Regridder")
    assert {k: got.attrs[k] for k in PACKING} == {k: da.attrs[k] for k in PACKING}
    assert got.attrs == da.attrs
    # it reads back through CFDecode: NaN where the float64 result is NaN, within half a step elsewhere
    back = CFDecode.from_attrs(got.attrs, dtype=np.float64, raw_dtype=raw).decode(got.values)
    ok = want != enc.fill_value
    assert np.isnan(back[~ok]).all() and (np.abs(back[ok] - f64.values[ok]) <= 0.5 * ENC_SCALE + 1e-9).all()
    for k in got.coords:
        assert np.array_equal(got.coords[k].values, f64.coords[k].values)
    # device-resident fields, both layouts
    dev = DataArray(to_device(da.data), dims=da.dims, coords=da.coords, name=da.name, attrs=da.attrs)
    out = rg.regrid(dev)
    assert out.data.dtype == np.dtype(raw)
    same_bits(out.values, want, "device field")
    sb = DataArray(to_device(np.ascontiguousarray(da.data.transpose(1, 2, 0)), layout="sb"), dims=("lat", "lon", "time"),
                   coords=da.coords, name=da.name, attrs=da.attrs)
    same_bits(rg.regrid(sb).values, want, "batch-fastest device field")
    kept = Regridder(weights=w, skipna=skipna, packed=True, packed_out=True, keep_batch_fastest=True).regrid(sb)
    assert kept.data.layout == "sb" and kept.data.dtype == np.dtype(raw)
    same_bits(kept.values, np.ascontiguousarray(want.transpose(1, 2, 0)), "kept batch-fastest")
    # lazy: deferred as before, the dtype is the raw dtype
    lazy = Regridder(weights=w, skipna=skipna, packed=True, packed_out=True, lazy=True).regrid(da)
    assert isinstance(lazy.data, LazyArray) and lazy.data.dtype == np.dtype(raw) and not lazy.data.computed
    same_bits(np.asarray(lazy.values), want, "lazy")


def test_regridder_dataset_mixing_packed_and_float(hip, caplog):
    rng = np.random.default_rng(31)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da = _packed_da(rng)
    nofill = _packed_da(rng, name="skt", fill_attr=False)          # packed, but no fill attribute: float64 as today
    other = DataArray(250.0 + rng.standard_normal((6, 90, 180)), dims=da.dims, coords=da.coords, name="tas",
                      attrs={"units": "K"})
    ds = Dataset({"t2m": da, "skt": nofill, "tas": other}, coords=dict(da.coords))
    today = Regridder(weights=w, packed=True).regrid(ds)
    with caplog.at_level("WARNING"):
        out = Regridder(weights=w, packed=True, packed_out=True).regrid(ds)
    assert sum("comes back as float64" in r.getMessage() for r in caplog.records) == 1
    enc = CFEncode.from_attrs(da.attrs, np.int16)
    assert out["t2m"].values.dtype == np.int16
    same_bits(out["t2m"].values, enc.encode(today["t2m"].values), "packed variable")
    assert out["t2m"].attrs == da.attrs
    for name in ("skt", "tas"):
        assert out[name].values.dtype == np.float64
        assert np.array_equal(out[name].values.view(np.uint64), today[name].values.view(np.uint64)), name
        assert out[name].attrs == today[name].attrs
    assert not set(PACKING) & set(out["skt"].attrs) and out["tas"].attrs == {"units": "K"}


def test_regridder_packed_out_false_is_today(hip):
    rng = np.random.default_rng(37)
    w = gridgen.bilinear_weights("r180x90", "r90x45")
    da = _packed_da(rng)
    a = Regridder(weights=w, packed=True).regrid(da)
    b = Regridder(weights=w, packed=True, packed_out=False).regrid(da)
    dec = DataArray(CFDecode.from_attrs(da.attrs, raw_dtype=np.int16).decode(da.data), dims=da.dims, coords=da.coords,
                    name=da.name, attrs={k: v for k, v in da.attrs.items() if k not in PACKING})
    ref = Regridder(weights=w).regrid(dec)
    for out in (a, b):
        assert out.values.dtype == np.float64
        assert np.array_equal(out.values.view(np.uint64), ref.values.view(np.uint64))
        assert out.attrs == ref.attrs == {"units": "K", "long_name": "2 metre temperature"}


@pytest.mark.parametrize("packed_levels", [False, True])
def test_regridder_levels_encode_on_the_host(hip, caplog, packed_levels):
    """3-D (masked-level) weights: the regrid runs as before, a host result is encoded on the host -- one INFO line, the
    same bits; a device-resident result stays float64 with a WARNING; lazy defers with the raw dtype."""
    rng = np.random.default_rng(41)
    g = gridgen.parse_grid("r72x36")
    levels, nt = (5.0, 50.0, 500.0, 2000.0), 3
    masks = gridgen.synthetic_ocean_masks(72, 36, len(levels), top=0.95, bottom=0.6)
    q = rng.integers(-32767, 32768, size=(nt, len(levels), 36, 72)).astype(np.int16)
    for l in range(len(levels)):
        q[:, l].reshape(nt, -1)[:, masks[l] == 0] = -32768
    coords = {"time": np.arange(nt), "lev": np.asarray(levels), "lat": g.lat, "lon": g.lon}
    attrs = {"scale_factor": 1.0e-3, "add_offset": 20.0, "_FillValue": np.int16(-32768), "units": "psu"}
    da = DataArray(q, dims=("time", "lev", "lat", "lon"), coords=coords, name="so", attrs=attrs)
    cf = CFDecode.from_attrs(attrs, raw_dtype=np.int16)
    dec = DataArray(cf.decode(q), dims=da.dims, coords=coords, name="so", attrs={"units": "psu"})
    w3 = CdoGenerate(dec, "r24x12").weights(method="con", mask_dim="lev")
    kw = dict(weights=w3, packed=True, packed_levels=packed_levels)
    f64 = Regridder(**kw).regrid(da)
    enc = CFEncode.from_attrs(attrs, np.int16)
    want = enc.encode(f64.values)
    assert (want == -32768).any() and (want != -32768).any()
    with caplog.at_level("INFO"):
        got = Regridder(loglevel="INFO", packed_out=True, **kw).regrid(da)
    assert sum("encoded on the host" in r.getMessage() for r in caplog.records) == 1
    assert got.values.dtype == np.int16 and got.dims == f64.dims
    same_bits(got.values, want, "levels")
    assert got.attrs == attrs
    lazy = Regridder(packed_out=True, lazy=True, **kw).regrid(da)
    assert isinstance(lazy.data, LazyArray) and lazy.data.dtype == np.int16 and not lazy.data.computed
    same_bits(np.asarray(lazy.values), want, "levels lazy")
    caplog.clear()
    dev = DataArray(to_device(q), dims=da.dims, coords=coords, name="so", attrs=attrs)
    with caplog.at_level("WARNING"):
        out = Regridder(packed_out=True, **kw).regrid(dev)
    assert sum("stays float64" in r.getMessage() for r in caplog.records) == 1
    assert out.values.dtype == np.float64 and not set(PACKING) & set(out.attrs)
    assert np.array_equal(out.values.view(np.uint64), f64.values.view(np.uint64))
