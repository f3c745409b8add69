"""Every instantiation `launch_tile` can pick (tests/cell_cases.py: REACHABLE, CASES) is launched, identified through
`launch_info` and compared bit for bit with the oracle -- through the tile kernel and, on the same input, through the
SELL kernel -- and the SELL kernel's batch tiling (BT = 1 / 2 / 4 / 8) is walked over every batch tail."""
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import CFDecode, CFEncode, SparseOperator, _lib, to_device
from tests import cell_cases as cc
from tests.helpers import bits_equal, field, skipna_ref

pytestmark = pytest.mark.gpu
T, S_ = _lib.APPLY_KERNEL_TILE, _lib.APPLY_KERNEL_SELL


@functools.lru_cache(maxsize=None)
def _operator(op_args):
    """(operator with its epilogue set, the oracle's CSR of the links, imask, frac, sentinel columns): once per module."""
    L = cc.banded_links(*op_args)
    op = SparseOperator(L["n_src"], L["n_dst"], L["src"], L["dst"], L["w"], device=0)
    rng = np.random.default_rng([cc.SEED, 1] + [int(v) for v in op_args])
    imask = (rng.random(op.n_dst) > 0.1).astype(np.int32)
    frac = rng.random(op.n_dst)
    op.set_epilogue(imask, frac)
    csr = oracle.coo_to_csr(L["n_src"], L["n_dst"], L["src"], L["dst"], L["w"])
    for got, want in zip(op.export_csr(), csr):
        assert np.array_equal(got, want)
    return op, csr, imask, frac, L["sentinels"]


def _reference(csr, x, case_or_flags, imask, frac, ydt):
    masked, area_min, skipna = case_or_flags
    if skipna:
        return skipna_ref(csr, x, masked, imask, frac, area_min, ydt)
    return oracle.apply_c(csr, x, masked, imask, frac, area_min).astype(ydt)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_cell_matches_oracle(hip, rng, case):
    op, csr, imask, frac, sentinels = _operator(case.op)
    knobs = dict(case.knobs)
    xdt, ydt = cc.XDT[case.xt], cc.XDT[case.yt]
    flags = T | (_lib.APPLY_MASKED if case.masked else 0) | (_lib.APPLY_SKIPNA if case.skipna else 0)
    with _lib.tuning(**knobs):
        info = op.launch_info(case.batch, xdt, flags=flags)
    cell, np_needed = cc.structural_cell(int(np.diff(csr[0]).max()), info, knobs)
    assert (cell, np_needed) == (case.cell, case.np_needed), info
    assert info["j_per_block"] == min(case.batch, knobs["tile_walk"])
    x = field(rng, case.batch, op.n_src, xdt, nan_frac=0.03, inf_frac=0.005)
    x[0, list(sentinels)] = (-123456.75, 654321.5)          # distinctive, exact in float32
    x[-1, list(sentinels)] = np.nan if case.batch > 1 else (777.25, -3.0e5)
    dx = to_device(x)
    kw = dict(masked=case.masked, remap_area_min=case.area_min, out_dtype=ydt, skipna=case.skipna)
    ref = _reference(csr, x, (case.masked, case.area_min, case.skipna), imask, frac, ydt)
    with _lib.tuning(**knobs):
        y = op.apply(dx, flags=T, **kw).to_host()
    bits_equal(y, ref)
    bits_equal(op.apply(dx, flags=S_, **kw).to_host(), ref)


# ---------------------------------------------------------------- the SELL kernel's batch tiling

SELL_X = ("f32", "f64", "i16->f32", "u16->f64")
SELL_Y = ("f64", "f32", "i16")
# a packed field decodes into float64 results or packed ones (smm_apply_cf / smm_apply_pk)
SELL_XY = [(x, y) for x in SELL_X for y in SELL_Y if not ("->" in x and y == "f32")]
B_MAX = max(b for _, bs in cc.SELL_BT.values() for b in bs)
_FILL = {np.dtype(np.int16): -32768, np.dtype(np.uint16): 65535}


@functools.lru_cache(maxsize=None)
def _sell_operator():
    n_src, n_dst, src, dst, w = cc.ragged_sell_links()
    op = SparseOperator(n_src, n_dst, src, dst, w, device=0)
    rng = np.random.default_rng(cc.SEED + 2)
    imask, frac = (rng.random(n_dst) > 0.1).astype(np.int32), rng.random(n_dst)
    op.set_epilogue(imask, frac)
    csr = oracle.coo_to_csr(n_src, n_dst, src, dst, w)
    assert n_dst % 64 and np.diff(csr[0]).min() == 0 and 30 <= np.diff(csr[0]).max() <= 40
    return op, csr, imask, frac


@functools.lru_cache(maxsize=None)
def _sell_field(xkind):
    """(what the kernel reads, its CFDecode or None, the values it stands for): B_MAX rows, made once and left unchanged."""
    rng = np.random.default_rng([cc.SEED, 3, SELL_X.index(xkind)])
    n_src = _sell_operator()[0].n_src
    if "->" not in xkind:
        x = field(rng, B_MAX, n_src, cc.XDT[xkind], nan_frac=0.03, inf_frac=0.005)
        x.setflags(write=False)
        return x, None, x
    raw = np.dtype(np.int16 if xkind[0] == "i" else np.uint16)
    info = np.iinfo(raw)
    q = rng.integers(info.min, info.max + 1, size=(B_MAX, n_src)).astype(raw)
    q[rng.random(q.shape) < 0.03] = _FILL[raw]
    cf = CFDecode(0.125, 20.0 if raw == np.int16 else -4000.0, (_FILL[raw],), cc.XDT[xkind[-3:]])
    x = cf.decode(q)
    for a in (q, x):
        a.setflags(write=False)
    return q, cf, x


@functools.lru_cache(maxsize=None)
def _sell_reference(xkind, ykind, skipna):
    op, csr, imask, frac = _sell_operator()
    x = _sell_field(xkind)[2]
    y = _reference(csr, x, (True, 0.37, skipna), imask, frac, np.float32 if ykind == "f32" else np.float64)
    if ykind == "i16":
        y = _encoder(xkind).encode(y)
    y.setflags(write=False)
    return y


def _encoder(xkind):
    """The packed result form: int16, or the field's own raw type (a packed field packs into that one only)."""
    if xkind.startswith("u16"):
        return CFEncode(0.25, -8000.125, 65535, np.uint16)
    return CFEncode(0.25, -1024.125, -32768, np.int16)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("xkind,ykind", SELL_XY, ids=lambda v: v)
@pytest.mark.parametrize("bt", sorted(cc.SELL_BT))
def test_sell_batch_tiles_and_tails(hip, bt, xkind, ykind, skipna):
    op, csr, imask, frac = _sell_operator()
    xin, cf, _ = _sell_field(xkind)
    ref = _sell_reference(xkind, ykind, skipna)
    knob, batches = cc.SELL_BT[bt]
    kw = dict(masked=True, remap_area_min=0.37, skipna=skipna, flags=S_)
    if cf is not None:
        kw["cf"] = cf
    if ykind == "i16":
        kw["cf_out"] = _encoder(xkind)
    else:
        kw["out_dtype"] = cc.XDT[ykind]
    reached = set()
    with _lib.tuning(sell_batch_rows=knob):
        for b in batches:
            info = op.launch_info(b, xin.dtype, flags=S_)
            assert info["kernel"] == "sell" and info["rows_per_step"] == cc.sell_batch_rows(b, knob)
            reached.add(info["rows_per_step"])
            y = op.apply(to_device(np.ascontiguousarray(xin[:b])), **kw).to_host()
            if ykind == "i16":
                assert y.dtype == ref.dtype and np.array_equal(y, ref[:b]), f"B={b}: {np.argwhere(y != ref[:b])[:5].tolist()}"
            else:
                try:
                    bits_equal(y, ref[:b])
                except AssertionError as e:
                    raise AssertionError(f"B={b}: {e}") from None
    assert bt in reached
