"""The in-kernel CF encode (`cf_out=`, the `_pk` entries) on NON-DYADIC rules and adversarial values.

tests/test_gpu_packed_out.py builds its fields in the arithmetic of a dyadic rule, where (y - offset) / scale is exact:
a kernel that multiplies by 1 / scale, re-associates, contracts to an fma or keeps a float32 intermediate gives the
same bits there.  Here the rules are of the kind real files carry and the values (tests/cf_cases.py) are the ones on
which such kernels differ from `CFEncode.encode` (tests/test_cf_encode_reference.py shows that each does).

The vehicle is a selection operator: one link of weight exactly 1.0 per destination row computes 0.0 + 1.0 * x, which
is x bit for bit (-0.0 comes back as +0.0); the plain epilogue turns non-finite x and x > 1e19 into NaN.  So any chosen
double stands in front of the encode on every path that stores packed results.  The expectation is `CFEncode.encode`
of that host-side model, never of a GPU result.  Every comparison is bit equality."""
import numpy as np
import pytest

from smmregrid_amd import CFDecode, SparseOperator, _lib, gridgen, to_device
from tests import cf_cases as C
from tests import helpers

pytestmark = pytest.mark.gpu
N = 1031                                    # prime: no multiple of 16 or 64 (ragged last tile of kernels A and C)
RULE_RAW = [(s, o, raw) for s, o in C.RULES for raw in C.RAWS]
IDS = [C.rule_id(*r) for r in RULE_RAW]
EPILOGUES = [(m, na) for m in (False, True) for na in (False, True)]


def same_bits(got, want, y, what):
    """got == want element for element; on a mismatch: the rule and path (`what`), the first three offending values of
    the float64 result y the encode saw, as float.hex(), and got against want."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, want.shape, got.dtype, want.dtype)
    bad = np.argwhere(got != want)
    if bad.size:
        first = [(float(y[tuple(i)]).hex(), f"got {int(got[tuple(i)])}", f"want {int(want[tuple(i)])}") for i in bad[:3]]
        raise AssertionError(f"{what}: {len(bad)} of {got.size} elements differ, first {first}")


def same_f64(got, want, what):
    """float64 results bit for bit (any NaN equals any NaN: the kernels make their own)."""
    assert got.dtype == np.float64 and got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    assert np.array_equal(gn, wn), f"{what}: NaN pattern differs at {np.argwhere(gn != wn)[:3].tolist()}"
    bad = np.flatnonzero(got[~gn].view(np.uint64) != want[~wn].view(np.uint64))
    assert bad.size == 0, f"{what}: {bad.size} values differ, first {[(float(got[~gn][i]).hex(), float(want[~wn][i]).hex()) for i in bad[:3]]}"


# ---------------------------------------------------------------- the selection operator

_SEL = []


def selection():
    """(operator, perm, dst_imask): destination row d reads source cell perm[d] with weight 1.0; ~10 % masked rows,
    no dst_frac.  Built once per session."""
    if not _SEL:
        rng = np.random.default_rng(20261017)
        perm = rng.permutation(N)
        order = rng.permutation(N)                                   # the link list is not sorted
        op = SparseOperator(N, N, (perm + 1)[order].astype(np.int32), (np.arange(N) + 1)[order].astype(np.int32),
                            np.ones(N), device=0)
        imask = (rng.random(N) > 0.1).astype(np.int32)
        assert 0 < (imask == 0).sum() < N // 5
        op.set_epilogue(imask, None)
        assert op.max_row_nnz == 1 and op.n_used_src == N
        _SEL.append((op, perm, imask))
    return _SEL[0]


def selected(x, perm, imask, masked):
    """What the selection operator makes of a float64 field x (B, N), stated on the host."""
    v = x[:, perm]
    with np.errstate(invalid="ignore"):
        out = np.where(np.isfinite(v) & (v <= 1e19), v + 0.0, np.nan)    # 0.0 + 1.0 * x: -0.0 -> +0.0
    if masked:
        out[:, imask == 0] = np.nan
    return out


def as_field(values):
    """(B, N), padded with repeats of the values."""
    rows = -(-values.size // N)
    return np.resize(values, rows * N).reshape(rows, N)


class Paths:
    """Every path that stores packed results, on one field: x (B, S) float64, or raw int16 / uint16 with cf."""

    def __init__(self, op, x, cf=None):
        self.op, self.cf = op, cf
        xt = np.ascontiguousarray(x.T)
        self.dx, self.dxt = to_device(x), to_device(xt, layout="sb")
        self.dxp = to_device(np.ascontiguousarray(xt[op.used_sources()]))

    def f64(self, **kw):
        return self.op.apply(self.dx, cf=self.cf, **kw).to_host()

    def a_and_c(self, enc, **kw):
        yield "kernel A", self.op.apply(self.dx, cf=self.cf, cf_out=enc, **kw).to_host()
        yield "kernel C", self.op.apply(self.dxt, cf=self.cf, cf_out=enc, **kw).to_host()

    def all(self, enc, **kw):
        yield from self.a_and_c(enc, **kw)
        op, kw = self.op, dict(kw, cf=self.cf, cf_out=enc)
        yield "forced SELL", op.apply(self.dx, flags=_lib.APPLY_KERNEL_SELL, **kw).to_host()
        yield "kernel C SB_PACKED", op.apply_sb(self.dxp, packed=True, **kw).to_host()
        kept = op.apply_sb(self.dxt, keep_batch_fastest=True, **kw)
        assert kept.layout == "sb" and kept.shape == (op.n_dst, self.dx.shape[0])
        yield "kernel C Y_SB", np.ascontiguousarray(kept.to_host().T)
        with _lib.tuning(sb_packed_y_rows=16):                           # the other tile height of kernel C
            yield "kernel C, 16-row tiles", op.apply(self.dxt, **kw).to_host()
            yield "kernel C Y_SB, 16-row tiles", np.ascontiguousarray(
                op.apply_sb(self.dxt, keep_batch_fastest=True, **kw).to_host().T)


# ---------------------------------------------------------------- adversarial values through every path

@pytest.mark.parametrize("scale,offset,raw", RULE_RAW, ids=IDS)
def test_adversarial_values_encode_as_the_rule_says_on_every_path(hip, scale, offset, raw):
    op, perm, imask = selection()
    enc = C.encoder(scale, offset, raw)
    x = as_field(C.cases(scale, offset, raw))
    assert x.shape[0] <= 59 and x.dtype == np.float64
    paths = Paths(op, x)
    seen = set()
    for masked, skipna in EPILOGUES:
        what = f"rule {C.rule_id(scale, offset, raw)} masked={masked} skipna={skipna}"
        kw = dict(masked=masked, skipna=skipna)
        y = selected(x, perm, imask, masked)
        want = enc.encode(y)
        # the vehicle: the float64 result is the host-side model bit for bit, so `want` owes nothing to the GPU
        y64 = paths.f64(**kw)
        same_f64(y64, y, what + " float64 result")
        same_bits(enc.encode(y64), want, y, what + " encode of the float64 result")
        assert (want == enc.fill_value).any() and (want != enc.fill_value).sum() > x.size // 2
        for path, got in paths.all(enc, **kw):
            assert got.dtype == raw
            same_bits(got, want, y, f"{what} {path}")
            seen.add(path)
    assert len(seen) == 7
    # the host pipeline, once per rule
    y = selected(x, perm, imask, True)
    want = enc.encode(y)
    for label, flags in (("packed", 0), ("whole rows", _lib.APPLY_HOST_NO_PACK)):
        got = op.apply_host(x, masked=True, cf_out=enc, flags=flags)
        same_bits(got, want, y, f"rule {C.rule_id(scale, offset, raw)} apply_host {label}")


# ---------------------------------------------------------------- decode -> encode inside one launch

DECODES = [(s, o, raw, dt) for s, o, raw in RULE_RAW for dt in (np.float32, np.float64)]


@pytest.mark.parametrize("scale,offset,raw,dtype", DECODES,
                         ids=[f"{C.rule_id(s, o, raw)}-{np.dtype(dt).name}" for s, o, raw, dt in DECODES])
def test_every_raw_value_decodes_exactly_and_encodes_back(hip, scale, offset, raw, dtype):
    """All 65 536 raw values through the in-kernel decode (exhaustive: the float64 result is `CFDecode.decode` bit for
    bit) and, in the same launch, through the in-kernel encode of the same rule: `encode(decode(q))`, which is q itself
    off the fill value (tests/test_cf_encode_reference.py; the one rule that float32 cannot carry keeps the host
    composition as its expectation)."""
    op, perm, imask = selection()
    info, fill = np.iinfo(raw), C.FILLS[np.dtype(raw)]
    q = as_field(np.arange(info.min, info.max + 1).astype(raw))
    assert q.shape == (64, N) and q.dtype == raw and np.unique(q).size == 65536
    cf, enc = CFDecode(scale, offset, (fill,), dtype), C.encoder(scale, offset, raw)
    decoded = cf.decode(q).astype(np.float64)
    paths = Paths(op, q, cf=cf)
    for masked, skipna in EPILOGUES:
        what = f"rule {C.rule_id(scale, offset, raw)} decode {np.dtype(dtype).name} masked={masked} skipna={skipna}"
        kw = dict(masked=masked, skipna=skipna)
        y = selected(decoded, perm, imask, masked)
        same_f64(paths.f64(**kw), y, what + " kernel A float64")
        same_f64(op.apply(paths.dxt, cf=cf, **kw).to_host(), y, what + " kernel C float64")
        want = enc.encode(y)
        if not (dtype == np.float32 and (scale, offset) in C.NO_F32_ROUND_TRIP):
            qs = q[:, perm]
            alive = ~np.isnan(y)
            assert np.array_equal(want[alive], qs[alive]) and (want[~alive] == fill).all()
        for path, got in paths.a_and_c(enc, **kw):
            same_bits(got, want, y, f"{what} {path}")


# ---------------------------------------------------------------- realistic stencils

_OPS = {}


def stencil(name):
    """(operator, dst_frac or None, batch): the conservative and the bilinear operator of test_gpu_packed_out.py, with
    10 % masked rows."""
    if name not in _OPS:
        if name == "con":           # 9 links per row, with dst_frac
            w, batch = gridgen.conservative_weights("r144x72", "r48x24"), 37
        else:                       # n_dst = 648: no multiple of 16 or 64 rows
            w, batch = gridgen.bilinear_weights("r143x71", "r36x18"), 203
        op = SparseOperator(w.sizes["src_grid_size"], w.sizes["dst_grid_size"], w["src_address"].values,
                            w["dst_address"].values, w["remap_matrix"].values, device=0)
        frac = w["dst_grid_frac"].values if "dst_grid_frac" in w else None
        imask = (np.random.default_rng(20261018).random(op.n_dst) > 0.1).astype(np.int32)
        op.set_epilogue(imask, frac)
        _OPS[name] = (op, frac, batch)
    return _OPS[name]


@pytest.mark.parametrize("raw", C.RAWS, ids=["i16", "u16"])
@pytest.mark.parametrize("name", ["con", "odd"])
def test_realistic_stencils_on_a_non_dyadic_rule(hip, name, raw):
    """Sums of several products in front of the encode: every path against `CFEncode.encode` of the float64 result of
    the existing entry (which the other GPU tests pin to the CPU oracle)."""
    scale, offset = 1.9e-3, 2.7e2
    op, frac, batch = stencil(name)
    enc = C.encoder(scale, offset, raw)
    info = np.iinfo(raw)
    rng = np.random.default_rng(47 + batch)
    # helpers.field is 250 +- 30; moved to the middle of the rule's range, whose half width is 62
    x = helpers.field(rng, batch, op.n_src, nan_frac=0.02) + (offset + scale * 0.5 * (info.min + info.max) - 250.0)
    paths = Paths(op, x)
    for skipna in (False, True):
        kw = dict(masked=True, skipna=skipna, remap_area_min=0.5 if frac is not None else 0.0)
        what = f"rule {C.rule_id(scale, offset, raw)} {name} skipna={skipna}"
        y64 = paths.f64(**kw)
        want = enc.encode(y64)
        fills = float((want == enc.fill_value).mean())
        print(f"{what}: fill share {fills:.3f}, NaN share {float(np.isnan(y64).mean()):.3f}")
        assert (want != enc.fill_value).any() and 0.0 < fills < 0.6, (what, fills)
        for path, got in paths.all(enc, **kw):
            same_bits(got, want, y64, f"{what} {path}")
        for label, flags in (("packed", 0), ("whole rows", _lib.APPLY_HOST_NO_PACK)):
            same_bits(op.apply_host(x, cf_out=enc, flags=flags, **kw), want, y64, f"{what} apply_host {label}")
