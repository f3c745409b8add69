"""The device entries at offsets past 2^31 and 2^32 elements (and past 2^32 bytes), in two files.  This one: smm_apply
(tile and SELL kernels, every field and result type), smm_apply_sb, smm_group_apply, smm_group_apply_sb, smm_apply_grib,
smm_apply_grib_bm, smm_fill_random, and the host pipelines smm_apply_host, smm_apply_host_cf, smm_group_apply_host and
smm_apply_host_grib.  tests/test_gpu_grib_far_offsets.py: the GRIB entries that came later -- smm_apply_grib_na,
smm_group_apply_grib, smm_group_apply_grib_na, smm_grib_pack and the four transcoders smm_grib_cpx_unpack,
smm_grib_aec_unpack, smm_grib_cpx_pack, smm_grib_aec_pack -- with the buffers, the fixture and the memory rule below.

Here: a handful of batch rows on a huge pitch, so the arithmetic stays tiny and only the addresses are large
(tests/far_cases.py; tests/test_far_cases.py shows that the checks catch an offset narrowed in any of four ways).

The pattern of every case: X is one flat buffer filled with decoys -- `fill_random` values of another mean for
float32 / float64, which is all `smm_fill_random` builds; the byte 0x44 for 2-byte elements (785.0 as bfloat16, 4.27 as
float16, 17476 as int16) -- into which the true rows are copied; Y is one flat buffer of the byte 0x42.  The raw entry
is called through `_lib.call` with the far strides, the true rows and the windows are copied back: the rows must hold
the bits of the CPU reference on the host copies, every window byte must still be 0x42.  X far and Y far are separate
cases, so that one case holds at most about 40 GiB; the buffers are freed explicitly.  A case skips only when
`mem_info()` reports less free memory than it needs plus 2 GiB.

SMM_FAR_REPORT=<path> writes per case the peak device bytes and the wall time as JSON lines."""
import ctypes
import functools
import json
import os
import time

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CFDecode, CFEncode, OperatorGroup,
                           SparseOperator, _lib, bfloat16)
from smmregrid_amd.device import DeviceArray, mem_info
from tests import cell_cases as cc
from tests import far_cases as fc
from tests import grib_cases
from tests import half_cases as hc
from tests.helpers import field, random_links, skipna_ref

pytestmark = pytest.mark.gpu

SEED = 20261019
GIB = 1 << 30
T, SELL = _lib.APPLY_KERNEL_TILE, _lib.APPLY_KERNEL_SELL
F32, F64, U16, I16, U8 = (np.dtype(t) for t in (np.float32, np.float64, np.uint16, np.int16, np.uint8))
CODE = {"f32": _lib.SMM_F32, "f64": _lib.SMM_F64, "f16": _lib.SMM_F16, "bf16": _lib.SMM_BF16, "i16": _lib.SMM_I16,
        "u16": _lib.SMM_U16}
NP = {"f32": F32, "f64": F64, "f16": U16, "bf16": U16, "i16": I16, "u16": U16}      # what the buffers hold (halves: bits)
LAUNCH_DTYPE = dict(NP, f16=np.float16, bf16=bfloat16)                              # what launch_info is asked about
AREA_MIN = 0.37
_vp = ctypes.c_void_p


# ------------------------------------------------------------------ buffers

class Buf:
    """A flat device buffer with the true rows of a Layout in it."""

    def __init__(self, arr, layout):
        self.arr, self.lay, self.isz = arr, layout, arr.dtype.itemsize

    @property
    def ptr(self):
        """Where row 0 starts: what the entry receives."""
        return _vp(self.arr.ptr + self.lay.offsets[0] * self.isz)

    def at(self, start, n):
        assert 0 <= start and start + n <= self.lay.size
        return DeviceArray((int(n),), self.arr.dtype, ptr=self.arr.ptr + int(start) * self.isz, base=self.arr)

    def put_rows(self, rows):
        rows = np.asarray(rows)
        assert rows.shape == (len(self.lay.offsets), self.lay.row_len), (rows.shape, self.lay.row_len)
        for o, r in zip(self.lay.offsets, rows):
            self.at(o, self.lay.row_len).copy_from_host(r)
        return self

    def rows(self):
        return np.stack([self.at(o, self.lay.row_len).to_host() for o in self.lay.offsets])

    def read(self, start, stop):
        return self.at(start, stop - start).to_host()

    def check(self, want, what):
        fc.check_rows(self.rows(), want, what)
        fc.check_windows(self.read, self.lay, self.isz, what)


class Far:
    """The buffers of one case: allocated against the memory rule, freed at the end, peak bytes and wall time kept."""

    def __init__(self, name):
        self.name, self.live, self.bytes, self.peak, self.t0 = name, [], 0, 0, time.perf_counter()

    def alloc(self, n, dtype):
        nbytes = int(n) * np.dtype(dtype).itemsize
        free = mem_info()[0]
        if free < nbytes + 2 * GIB:
            pytest.skip(f"{free / GIB:.1f} GiB of device memory free, the case needs {nbytes / GIB:.1f} GiB + 2 GiB")
        arr = DeviceArray((int(n),), dtype)
        self.live.append(arr)
        self.bytes += nbytes
        self.peak = max(self.peak, self.bytes)
        return arr

    def x(self, layout, dtype, rows, seed=1):
        """X: decoys everywhere, then the true rows."""
        arr = self.alloc(layout.size, dtype)
        if arr.dtype in (F32, F64):
            arr.fill_random(seed=seed, mean=1000.0, sigma=50.0)
        else:
            arr.fill_bytes(0x44)
        buf = Buf(arr, layout).put_rows(rows)
        if layout.guard:                                     # the decoys are there, up to the far end of the buffer
            d = buf.at(layout.offsets[-1] + layout.row_len, 16).to_host()
            assert (np.abs(d - 1000.0) < 400.0).all() if d.dtype in (F32, F64) else (d.view(U8) == 0x44).all(), d
        return buf

    def y(self, layout, dtype):
        return Buf(self.alloc(layout.size, dtype).fill_bytes(fc.SENTINEL), layout)

    def close(self):
        for a in self.live:
            a.free()
        self.live = []
        return {"case": self.name, "peak_bytes": self.peak, "seconds": round(time.perf_counter() - self.t0, 3)}


@pytest.fixture
def far(hip, request):
    f = Far(request.node.name)
    yield f
    rec = f.close()
    path = os.environ.get("SMM_FAR_REPORT")
    if path:
        with open(path, "a") as fh:
            fh.write(json.dumps(rec) + "\n")


def layouts(side, n_rows, xlen, ylen, **kw):
    """(X layout, ldx, Y layout, ldy) of a row-major case: the far side on the far pitch, the other contiguous."""
    lx, ldx = fc.rows_layout(n_rows, xlen, **kw) if side == "x" else (fc.near_layout(n_rows, xlen), xlen)
    ly, ldy = fc.rows_layout(n_rows, ylen, **kw) if side == "y" else (fc.near_layout(n_rows, ylen), ylen)
    return lx, ldx, ly, ldy


def reference(csr, x, imask, frac, skipna=False, masked=True, area_min=AREA_MIN):
    if skipna:
        return skipna_ref(csr, x, masked, imask, frac, area_min, np.float64)
    return oracle.apply_c(csr, x, masked, imask, frac, area_min).astype(np.float64)


def bad_field(rng, n, n_src, dtype):
    return field(rng, n, n_src, dtype, nan_frac=0.03, inf_frac=0.005)


# ------------------------------------------------------------------ smm_apply, tile kernel

TILE_FORMS = {
    "reg": (lambda c: c.shape == 256 and c.staging == "reg" and c.r == 1, 3),
    "dma": (lambda c: c.shape == 256 and c.staging == "dma" and c.r == 1, 3),
    "reg-r2": (lambda c: c.shape == 256 and c.staging == "reg" and c.r == 2, 3),
    # a walk of 3 rows would halve four rows per step: the walk of 4 steps across 2^31, its tail row lies past 2^32
    "reg-r4": (lambda c: c.shape == 256 and c.staging == "reg" and c.r == 4, 4),
    "wave": (lambda c: c.shape == 64 and c.staging == "reg" and not c.split and c.maxk == 32, 3),
    "split": (lambda c: c.split, 3),
}


@functools.lru_cache(maxsize=None)
def tile_operator(op_args):
    L = cc.banded_links(*op_args)
    op = SparseOperator(L["n_src"], L["n_dst"], L["src"], L["dst"], L["w"], device=0)
    rng = np.random.default_rng([SEED, 1] + [int(v) for v in op_args])
    imask, frac = (rng.random(op.n_dst) > 0.1).astype(np.int32), rng.random(op.n_dst)
    op.set_epilogue(imask, frac)
    return op, oracle.coo_to_csr(L["n_src"], L["n_dst"], L["src"], L["dst"], L["w"]), imask, frac


@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("xt", cc.XTS)
@pytest.mark.parametrize("form", TILE_FORMS)
def test_apply_tile_kernel(far, form, xt, side):
    """B = 5 on a pitch of 2^30 + K: one workgroup's walk of 3 rows steps across 2^31, the tail walk across 2^32."""
    pick, walk = TILE_FORMS[form]
    B = 5
    case = next(c for c in cc.CASES if c.xt == xt and pick(c.cell) and c.batch >= dict(c.knobs)["tile_walk"] >= walk)
    op, csr, imask, frac = tile_operator(case.op)
    knobs = dict(case.knobs, tile_walk=walk)
    if case.cell.shape == 256:
        knobs["tile_rows_per_step"] = case.cell.r
    xdt = cc.XDT[xt]
    flags = T | _lib.APPLY_MASKED
    with _lib.tuning(**knobs):
        info = op.launch_info(B, xdt, flags=flags)
    cell, _ = cc.structural_cell(int(np.diff(csr[0]).max()), info, knobs)
    assert cell == case.cell and info["j_per_block"] == walk, (info, cell, case.cell)
    x = bad_field(np.random.default_rng([SEED, 2, B]), B, op.n_src, xdt)
    lx, ldx, ly, ldy = layouts(side, B, op.n_src, op.n_dst)
    X, Y = far.x(lx, xdt, x), far.y(ly, F64)
    with _lib.tuning(**knobs):
        _lib.call("smm_apply", op.handle, X.ptr, CODE[xt], ldx, Y.ptr, _lib.SMM_F64, ldy, B, AREA_MIN, flags, None)
    Y.check(reference(csr, x, imask, frac), f"tile {form} {xt} far {side}")


# ------------------------------------------------------------------ smm_apply, SELL kernel

@functools.lru_cache(maxsize=None)
def sell_operator():
    n_src, n_dst, src, dst, w = cc.ragged_sell_links()
    op = SparseOperator(n_src, n_dst, src, dst, w, device=0)
    rng = np.random.default_rng(SEED + 2)
    imask, frac = (rng.random(n_dst) > 0.1).astype(np.int32), rng.random(n_dst)
    op.set_epilogue(imask, frac)
    return op, oracle.coo_to_csr(n_src, n_dst, src, dst, w), imask, frac


CF = CFDecode(0.125, 20.0, (-32768,), np.float32)
ENC = CFEncode(0.25, -8000.125, 65535, np.uint16)


def typed_field(xk, n, n_src, seed):
    """(what the device holds, the values it stands for) for a field of kind xk."""
    rng = np.random.default_rng([SEED, 3, seed])
    if xk in ("f32", "f64"):
        x = bad_field(rng, n, n_src, NP[xk])
        return x, x
    if xk == "i16":
        q = rng.integers(-32768, 32768, size=(n, n_src)).astype(np.int16)
        q[rng.random(q.shape) < 0.03] = -32768
        return q, CF.decode(q)
    bits = hc.half_field(xk, (n, n_src), seed)
    return bits, hc.widen(bits, xk)


def typed_result(y64, yk):
    """The float64 reference as what a Y of kind yk must hold."""
    if yk == "f64":
        return y64
    if yk == "f32":
        return y64.astype(np.float32)
    if yk == "u16":
        return ENC.encode(y64)
    return hc.round_bits(y64, yk).astype(np.uint16)


def apply_raw(entry, handle, X, xk, mid, Y, yk, rest):
    """entry, entry_cf for an int16 X, entry_pk for a uint16 Y: the rule structs go last."""
    rules = []
    if yk == "u16":
        entry, rules = entry + "_pk", [None, ctypes.byref(ENC._struct())]
    elif xk == "i16":
        entry, rules = entry + "_cf", [ctypes.byref(CF._struct(I16))]
    _lib.call(entry, handle, X.ptr, CODE[xk], *mid, Y.ptr, CODE[yk], *rest, *rules)


# (field, result, SKIPNA)
SELL_KINDS = {"f32": ("f32", "f64", False), "f64": ("f64", "f64", False), "f64-skipna": ("f64", "f64", True),
              "i16-cf": ("i16", "f64", False), "f16": ("f16", "f16", False), "bf16": ("bf16", "bf16", False),
              "f32-pk": ("f32", "u16", False)}


@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("kind", SELL_KINDS)
def test_apply_sell_kernel(far, kind, side):
    """9 rows on a pitch of 2^29 + K (row 4 past 2^31 elements, row 8 past 2^32) through 2, 4 and 8 batch rows per
    thread: 8 rows per thread need a batch of 8, and the 2-byte types cross at their full element count."""
    xk, yk, skipna = SELL_KINDS[kind]
    op, csr, imask, frac = sell_operator()
    B = 9
    x, values = typed_field(xk, B, op.n_src, 1)
    want = typed_result(reference(csr, values, imask, frac, skipna), yk)
    lx, ldx, ly, ldy = layouts(side, B, op.n_src, op.n_dst)
    X, Y = far.x(lx, NP[xk], x), far.y(ly, NP[yk])
    flags = SELL | _lib.APPLY_MASKED | (_lib.APPLY_SKIPNA if skipna else 0)
    for knob in (2, 4, 8):
        Y.arr.fill_bytes(fc.SENTINEL)
        with _lib.tuning(sell_batch_rows=knob):
            info = op.launch_info(B, LAUNCH_DTYPE[xk], flags=SELL)
            assert info["kernel"] == "sell" and info["rows_per_step"] == knob == cc.sell_batch_rows(B, knob), info
            apply_raw("smm_apply", op.handle, X, xk, (ldx,), Y, yk, (ldy, B, AREA_MIN, flags, None))
        Y.check(want, f"SELL {kind} far {side}, {knob} rows per thread")


# ------------------------------------------------------------------ smm_apply_sb

S_SB = D_SB = 36            # c * ldx crosses 2^31 at cell 16 and 2^32 at cell 32 on a pitch of 2^27 + K


@functools.lru_cache(maxsize=None)
def sb_operator(seed=0):
    rng = np.random.default_rng([SEED, 4, seed])
    src, dst, w = random_links(rng, S_SB, D_SB, 220)
    src[:S_SB] = np.arange(1, S_SB + 1)                      # every source cell carries a link: the packed X has S rows
    op = SparseOperator(S_SB, D_SB, src, dst, w, device=0)
    imask, frac = (rng.random(D_SB) > 0.1).astype(np.int32), rng.random(D_SB)
    op.set_epilogue(imask, frac)
    assert op.n_used_src == S_SB
    return op, oracle.coo_to_csr(S_SB, D_SB, src, dst, w), imask, frac


# id: (field, result, far side, extra flags); "ysb" = the result kept batch-fastest, d * ldy crosses
SB_CASES = {
    "x-f32": ("f32", "f64", "x", 0),
    "x-i16-cf": ("i16", "f64", "x", 0),
    "x-f32-packed": ("f32", "f64", "x", _lib.APPLY_SB_PACKED),
    "y-f32": ("f32", None, "y", 0),
    "ysb-f64": ("f64", "f64", "ysb", _lib.APPLY_SB_Y_SB),
    "ysb-f32-pk": ("f32", "u16", "ysb", _lib.APPLY_SB_Y_SB),
}


@pytest.mark.parametrize("B", [3, 131])
@pytest.mark.parametrize("case", SB_CASES)
def test_apply_sb(far, case, B):
    """Odd batches: 3 (the lane that shifts one entry) and 131 (a second batch tile).  The plain far Y has B rows:
    3 rows on a pitch of 2^31 + K hold float32 results, 131 rows on 2^25 + K float64 ones."""
    xk, yk, side, extra = SB_CASES[case]
    if yk is None:
        yk = "f32" if B == 3 else "f64"
    op, csr, imask, frac = sb_operator()
    x, values = typed_field(xk, B, S_SB, 10 + B)
    want = typed_result(reference(csr, values, imask, frac), yk)
    if side == "x":
        (lx, ldx), (ly, ldy) = fc.rows_layout(S_SB, B), (fc.near_layout(B, D_SB), D_SB)
    elif side == "y":
        (lx, ldx), (ly, ldy) = (fc.near_layout(S_SB, B), B), fc.rows_layout(B, D_SB)
    else:
        (lx, ldx), (ly, ldy) = (fc.near_layout(S_SB, B), B), fc.rows_layout(D_SB, B)
        want = np.ascontiguousarray(want.T)
    X, Y = far.x(lx, NP[xk], np.ascontiguousarray(x.T)), far.y(ly, NP[yk])
    apply_raw("smm_apply_sb", op.handle, X, xk, (ldx,), Y, yk, (ldy, B, AREA_MIN, _lib.APPLY_MASKED | extra, None))
    Y.check(want, f"smm_apply_sb {case} B={B}")


# ------------------------------------------------------------------ smm_group_apply: 3 levels over 2 operators

LEVEL_INDEX = np.array([1, 0, 1], np.int32)
MASKED_LEVELS = np.array([1, 0], np.uint8)


@functools.lru_cache(maxsize=None)
def tile_group():
    """Two operators of the 4-wave tile shape on the same grids, grouped."""
    args = next(c.op for c in cc.CASES if c.xt == "f32" and c.cell.shape == 256 and c.cell.r == 1)
    members = [tile_operator(args), tile_operator(args + (cc.N_DST, SEED))]          # the same bands, other links
    assert members[0][0].n_src == members[1][0].n_src and members[0][0].n_dst == members[1][0].n_dst
    grp = OperatorGroup([m[0] for m in members])
    assert grp.plan_info()["tile_plan"]
    return grp, members


def level_reference(members, x):
    """x (n_lev, rows per level, S): every row through the member its level names."""
    out = []
    for lev, rows in enumerate(x):
        _, csr, imask, frac = members[LEVEL_INDEX[lev]]
        out.append(reference(csr, rows, imask, frac, masked=bool(MASKED_LEVELS[LEVEL_INDEX[lev]])))
    return np.stack(out)


@pytest.mark.parametrize("kernel", ["tile", "sell"])
@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("which", ["lev", "outer"])
def test_group_apply(far, which, side, kernel):
    """lev: (2 outer, 3 levels, 2 inner) with the level stride far and the outer and inner strides near.
    outer: (3 outer, 3 levels, 1 inner) with the outer stride far.  float32 fields and results: 3 x 2^31 elements."""
    grp, members = tile_group()
    S, D = grp.n_src, grp.n_dst
    n_outer, n_lev, n_inner = (2, 3, 2) if which == "lev" else (3, 3, 1)
    near = n_outer * n_inner if which == "lev" else n_lev              # near rows under one far step
    x = bad_field(np.random.default_rng([SEED, 5]), 3 * near, S, F32).reshape(3, near, S)   # [far step, near row]
    if which == "lev":
        want = level_reference(members, x)
    else:
        want = level_reference(members, x.transpose(1, 0, 2)).transpose(1, 0, 2)
    want = want.astype(np.float32).reshape(3 * near, D)

    def strides(far_side, n):
        if far_side:
            lay, ld = fc.rows_layout(3, n, inner=near)
            s1 = lay.offsets[1] - lay.offsets[0]
        else:
            lay, ld, s1 = fc.near_layout(3 * near, n), near * n, n
        # (outer, lev, inner) strides
        return lay, ((n_inner * s1, ld, s1) if which == "lev" else (ld, s1, s1))

    lx, xs = strides(side == "x", S)
    ly, ys = strides(side == "y", D)
    X, Y = far.x(lx, F32, x.reshape(3 * near, S)), far.y(ly, F32)
    flags = (T if kernel == "tile" else SELL) | _lib.APPLY_MASKED
    with _lib.tuning(tile_walk=3):
        info = grp.launch_info(n_outer, n_lev, n_inner, F32, flags=flags)
        assert info["kernel"] in (("tile", "tile-dma") if kernel == "tile" else ("sell",)), info
        _lib.call("smm_group_apply", grp.handle, X.ptr, _lib.SMM_F32, *xs, Y.ptr, _lib.SMM_F32, *ys, n_outer, n_lev,
                  n_inner, LEVEL_INDEX.ctypes.data_as(_vp), MASKED_LEVELS.ctypes.data_as(_vp), AREA_MIN, flags, None)
    Y.check(want, f"smm_group_apply {which} stride far in {side}, {kernel}")


# ------------------------------------------------------------------ smm_group_apply_sb

@pytest.mark.parametrize("level_launches", [0, 1], ids=["grouped", "per-level"])
@pytest.mark.parametrize("side", ["x", "y"])
def test_group_apply_sb(far, side, level_launches):
    """Three per-level (S, ldx) slabs 2^31 + K elements apart / three per-level (B, D) results that far apart."""
    members = [sb_operator(0), sb_operator(1)]
    grp = OperatorGroup([m[0] for m in members])
    B = 7
    x = bad_field(np.random.default_rng([SEED, 6]), 3 * B, S_SB, F32).reshape(3, B, S_SB)
    want = level_reference(members, x).astype(np.float32).reshape(3 * B, D_SB)
    if side == "x":
        ldx = fc._round4(B + 9)
        lx, xs_lev = fc.rows_layout(3, B, inner=S_SB, inner_stride=ldx)
        ly, ys_lev, ys_b = fc.near_layout(3 * B, D_SB), B * D_SB, D_SB
    else:
        ldx = B
        lx, xs_lev = fc.near_layout(3 * S_SB, B), S_SB * B
        ly, ys_lev = fc.rows_layout(3, D_SB, inner=B)
        ys_b = ly.offsets[1] - ly.offsets[0]
    X = far.x(lx, F32, np.ascontiguousarray(x.transpose(0, 2, 1)).reshape(3 * S_SB, B))
    Y = far.y(ly, F32)
    with _lib.tuning(sb_level_launches=level_launches):
        _lib.call("smm_group_apply_sb", grp.handle, X.ptr, _lib.SMM_F32, xs_lev, ldx, Y.ptr, _lib.SMM_F32, ys_lev, ys_b,
                  B, 3, LEVEL_INDEX.ctypes.data_as(_vp), MASKED_LEVELS.ctypes.data_as(_vp), AREA_MIN, _lib.APPLY_MASKED,
                  None)
    Y.check(want, f"smm_group_apply_sb far {side}")
    grp.close()


# ------------------------------------------------------------------ smm_apply_grib, smm_apply_grib_bm

def grib_case(S=None, n_rows=5):
    """One buffer of just over 2^34 bytes.  Row 0: 16 bits at a byte offset just over 2^32.  Row 1: 12 bits at an odd
    byte offset just over 2^34 (a word index past 2^32).  Row 2: a bitmap that lies far and a stream that lies near.
    Row 3: a stream that lies far and a bitmap that lies near.  Row 4: plain and near.  With n_rows = 6 (the grouped
    entries of tests/test_gpu_grib_far_offsets.py: records (outer, level) of 3 x 2) row 4 lies past 2^34 instead and
    row 5 past 2^32, so each of the two levels has a record past either.  S: the source cells (default: the SELL
    operator's).  Returns (x_bytes, pieces [(byte offset, bytes)], rows, bitmaps, decoded float32 field)."""
    S = sell_operator()[0].n_src if S is None else int(S)
    rng = np.random.default_rng([SEED, 7])
    nbits = (16, 12, 16, 12, 16, 12)[:n_rows]
    specs = [dict(q=grib_cases.random_q(rng, S, nb), nbits=nb, E=int(rng.integers(-6, 3)), D=int(b == 1),
                  ref=float(np.float32(rng.normal(0.0, 300.0)))) for b, nb in enumerate(nbits)]
    masks = {2: rng.random(S) < 0.6, 3: rng.random(S) < 0.3}
    data_off = {0: (1 << 32) + 8, 1: (1 << 34) + 4097, 2: 4099, 3: (1 << 32) + (1 << 31) + 6, 4: 40002}
    if n_rows == 6:
        data_off.update({4: (1 << 34) + 40002, 5: (1 << 32) + 90003})
    bm_off = {2: (1 << 33) + 5, 3: 80001}
    rows = np.zeros(n_rows, GRIB_ROW_DTYPE)
    bitmaps = np.zeros(n_rows, GRIB_BITMAP_DTYPE)
    bitmaps["bitmap_off"] = GRIB_NO_BITMAP
    pieces = []
    fld = np.stack([grib_cases.decode_ref(s["q"], s["ref"], s["E"], s["D"]) for s in specs])
    for b, s in enumerate(specs):
        q = np.asarray(s["q"], np.uint64)
        m = masks.get(b)
        pieces.append((data_off[b], grib_cases.pack_bits(q if m is None else q[m], s["nbits"])))
        rows[b] = (data_off[b], s["ref"], 2.0 ** s["E"], 10.0 ** s["D"], s["nbits"], 0)
        bitmaps["n_values"][b] = S if m is None else int(m.sum())
        if m is not None:
            packed = np.packbits(m.astype(np.uint8))
            if S % 8:
                packed[-1] |= 0xFF >> (S % 8)
            pieces.append((bm_off[b], packed.tobytes()))
            bitmaps["bitmap_off"][b] = bm_off[b]
            fld[b, ~m] = np.float32(np.nan)
    x_bytes = max(o + len(d) for o, d in pieces) + 3
    spans = sorted((o, o + len(d)) for o, d in pieces)
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])) and (1 << 34) < x_bytes < (1 << 34) + (1 << 20)
    return x_bytes, pieces, rows, bitmaps, fld


@pytest.mark.parametrize("entry", ["smm_apply_grib", "smm_apply_grib_bm"])
def test_apply_grib(far, entry):
    op, csr, imask, frac = sell_operator()
    x_bytes, pieces, rows, bitmaps, fld = grib_case()
    sel = [0, 1, 4] if entry == "smm_apply_grib" else [0, 1, 2, 3, 4]
    n_alloc = (x_bytes + 3) // 4 * 4
    xa = far.alloc(n_alloc // 4, F32).fill_random(seed=9, mean=1000.0, sigma=50.0)       # decoy bytes everywhere
    for off, data in pieces:
        DeviceArray((len(data),), U8, ptr=xa.ptr + off, base=xa).copy_from_host(np.frombuffer(data, U8))
    # today's expectation: smm_apply on the decoded field, itself tied to the oracle
    x = np.ascontiguousarray(fld[sel])
    ref = reference(csr, x, imask, frac)
    lx = fc.near_layout(len(sel), op.n_src)
    ly = fc.near_layout(len(sel), op.n_dst)
    Xd, Yd = far.x(lx, F32, x), far.y(ly, F64)
    _lib.call("smm_apply", op.handle, Xd.ptr, _lib.SMM_F32, op.n_src, Yd.ptr, _lib.SMM_F64, op.n_dst, len(sel), AREA_MIN,
              SELL | _lib.APPLY_MASKED, None)
    want = Yd.rows()
    fc.check_rows(want, ref, "smm_apply on the decoded field")
    Y = far.y(ly, F64)
    r = np.ascontiguousarray(rows[sel])
    rp = ctypes.cast(r.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))
    if entry == "smm_apply_grib":
        _lib.call(entry, op.handle, _vp(xa.ptr), x_bytes, rp, Y.ptr, _lib.SMM_F64, op.n_dst, len(sel), AREA_MIN,
                  _lib.APPLY_MASKED, None)
    else:
        bm = np.ascontiguousarray(bitmaps[sel])
        _lib.call(entry, op.handle, _vp(xa.ptr), x_bytes, rp, ctypes.cast(bm.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)),
                  Y.ptr, _lib.SMM_F64, op.n_dst, len(sel), AREA_MIN, _lib.APPLY_MASKED, None)
    got = Y.rows()
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), np.argwhere(got.view(np.uint64) != want.view(np.uint64))[:3]


# ------------------------------------------------------------------ smm_fill_random

def test_fill_random_past_2_32_elements(far):
    n, W = (1 << 32) + 4096 + 37, 4096
    a = far.alloc(n + W, F32)
    view = lambda s, m: DeviceArray((m,), F32, ptr=a.ptr + 4 * s, base=a)       # noqa: E731
    view(n - W, 2 * W).fill_bytes(fc.SENTINEL)
    _lib.call("smm_fill_random", _vp(a.ptr), _lib.SMM_F32, n, ctypes.c_uint64(77), 1000.0, 50.0, None)
    w0, w1, w2 = (view(s, W).to_host().view(np.uint32) for s in (0, 1 << 31, 1 << 32))
    for p, q in ((w0, w1), (w0, w2), (w1, w2)):
        assert (p != q).mean() > 0.99                      # a wrapped index would repeat a window
    tail = view(n - W, 2 * W).to_host().view(np.uint32)
    assert (tail[:W] != 0x42424242).all() and (tail[W:] == 0x42424242).all()     # the last element, and not one more
    small = far.alloc(W, F32).fill_random(seed=77, mean=1000.0, sigma=50.0).to_host().view(np.uint32)
    assert np.array_equal(w0, small)                       # element i depends only on (seed, i)
    for w in (w0, w1, w2, tail[:W]):
        v = w.view(np.float32)
        assert np.isfinite(v).all() and 600.0 < v.min() and v.max() < 1400.0 and 990.0 < v.mean() < 1010.0


# ------------------------------------------------------------------ host pipelines: pageable, virtual host arrays

class HostBuf:
    """A pageable host array from np.empty: virtual, so only what a case touches -- the true rows, and in a Y the
    windows, which get their sentinel bytes -- ever becomes resident.  Never pinned."""

    def __init__(self, layout, dtype, sentinel=False):
        self.lay, self.arr = layout, np.empty(layout.size, dtype)
        self.isz = self.arr.dtype.itemsize
        if sentinel:
            for o in layout.offsets:
                self.arr[o:o + layout.row_len].view(U8)[:] = fc.SENTINEL
            for s, e in fc.windows(layout, self.isz):
                self.arr[s:e].view(U8)[:] = fc.SENTINEL

    @property
    def ptr(self):
        return _vp(self.arr.ctypes.data + self.lay.offsets[0] * self.isz)

    def put_rows(self, rows):
        for o, r in zip(self.lay.offsets, rows):
            self.arr[o:o + self.lay.row_len] = r
        return self

    def check(self, want, what):
        fc.check_rows(np.stack([self.arr[o:o + self.lay.row_len] for o in self.lay.offsets]), want, what)
        fc.check_windows(lambda s, e: self.arr[s:e], self.lay, self.isz, what)


def host_layouts(side, n_rows, xlen, ylen):
    lx, ldx = fc.host_rows_layout(n_rows, xlen) if side == "x" else (fc.near_layout(n_rows, xlen), xlen)
    ly, ldy = fc.host_rows_layout(n_rows, ylen) if side == "y" else (fc.near_layout(n_rows, ylen), ylen)
    return lx, ldx, ly, ldy


@pytest.mark.parametrize("chunk_rows", [1, 2])
@pytest.mark.parametrize("xk,side", [("f32", "x"), ("f32", "y"), ("i16", "x")])
def test_apply_host(hip, xk, side, chunk_rows):
    """smm_apply_host (float32 X, float32 Y) and smm_apply_host_cf (int16 X): 5 rows on a pitch of 2^29 + K cross
    2^32 bytes and 2^31 elements in a mapping of under 9 GB.  smm_apply_host_cf stores float64 only, which would double
    the mapping: its Y goes through the code of smm_apply_host's, which the float32 case walks."""
    op, csr, imask, frac = sell_operator()
    B = 5
    yk = "f32" if xk == "f32" else "f64"
    x, values = typed_field(xk, B, op.n_src, 20)
    want = typed_result(reference(csr, values, imask, frac), yk)
    lx, ldx, ly, ldy = host_layouts(side, B, op.n_src, op.n_dst)
    X, Y = HostBuf(lx, NP[xk]).put_rows(x), HostBuf(ly, NP[yk], sentinel=True)
    _lib.host_stats(reset=True)
    apply_raw("smm_apply_host", op.handle, X, xk, (ldx,), Y, yk, (ldy, B, AREA_MIN, _lib.APPLY_MASKED, chunk_rows))
    st = _lib.host_stats(reset=True)
    assert st["chunks"] == -(-B // chunk_rows) and st["h2d_bytes"] == B * op.n_src * X.isz, st
    Y.check(want, f"smm_apply_host {xk} far {side}, {chunk_rows} rows per chunk")


@functools.lru_cache(maxsize=None)
def wide_group():
    """Two operators on 2^26 + 16 source cells whose few links touch early and late cells, and the same links on the
    used cells alone for the oracle (the map is monotone: the order of every sum is kept)."""
    S, D = (1 << 26) + 16, 3
    members = []
    for m in range(2):
        src = np.array([5 + m, S - 3, 0, S - 1 - m, 7], np.int64)
        dst = np.array([0, 0, 1, 2, 2], np.int64)
        w = np.random.default_rng([SEED, 8, m]).uniform(0.1, 1.0, size=src.size)
        op = SparseOperator(S, D, (src + 1).astype(np.int32), (dst + 1).astype(np.int32), w, device=0)
        imask, frac = np.array([1, m, 1], np.int32), np.array([0.9, 0.8, 0.2 + 0.7 * m])
        op.set_epilogue(imask, frac)
        used = np.unique(src)
        csr = oracle.coo_to_csr(used.size, D, np.searchsorted(used, src) + 1, dst + 1, w)
        members.append((op, csr, imask, frac, used))
    return OperatorGroup([m[0] for m in members]), members, S, D


@pytest.mark.parametrize("chunk_outer", [1, 2, 0], ids=["1", "2", "packed"])
def test_group_apply_host(hip, chunk_outer):
    """smm_group_apply_host takes no strides: the dense (9, 2, 1, S) float32 field itself is 4.8 GB, its last outer
    step starts past 2^32 bytes.  chunk_outer 1 / 2: whole rows travel; 0: the used cells, packed per level."""
    grp, members, S, D = wide_group()
    n_outer, n_lev, n_inner = 9, 2, 1
    lev = np.array([1, 0], np.int32)
    assert n_outer * n_lev * S * 4 > (1 << 32) and (n_outer - 1) * n_lev * S * 4 > (1 << 32)
    x = np.empty((n_outer, n_lev, n_inner, S), F32)                     # virtual: only the used cells are written
    rng = np.random.default_rng([SEED, 9])
    want = np.empty((n_outer, n_inner, n_lev, D), F64)
    for l in range(n_lev):
        _, csr, imask, frac, used = members[lev[l]]
        vals = bad_field(rng, n_outer, used.size, F32)
        x[:, l, 0, used] = vals
        want[:, 0, l] = reference(csr, vals, imask, frac, masked=bool(MASKED_LEVELS[lev[l]]))
    y = np.frombuffer(bytes([fc.SENTINEL]) * want.nbytes, F64).reshape(want.shape).copy()
    _lib.host_stats(reset=True)
    _lib.call("smm_group_apply_host", grp.handle, _vp(x.ctypes.data), _lib.SMM_F32, _vp(y.ctypes.data), _lib.SMM_F64,
              n_outer, n_lev, n_inner, 1, lev.ctypes.data_as(_vp), MASKED_LEVELS.ctypes.data_as(_vp), AREA_MIN,
              _lib.APPLY_MASKED, chunk_outer)
    st = _lib.host_stats(reset=True)
    if chunk_outer:
        assert st["chunks"] == -(-n_outer // chunk_outer) and st["h2d_bytes"] >= n_outer * n_lev * S * 4, st
    else:
        assert st["chunks"] >= 1 and st["h2d_bytes"] == sum(members[m][4].size for m in lev) * n_outer * 4, st
    fc.check_rows(y, want, f"smm_group_apply_host chunk_outer={chunk_outer}")


@pytest.mark.parametrize("chunk_rows", [1, 2])
def test_apply_host_grib(far, chunk_rows):
    """A row whose byte_off lies past 2^32 in an x_bytes over 2^32 (16 bits, and 12 bits at an odd offset)."""
    op, csr, imask, frac = sell_operator()
    S = op.n_src
    rng = np.random.default_rng([SEED, 10])
    nbits, offs = (16, 16, 12), (4098, (1 << 32) + 4097, (1 << 32) + 20001)
    specs = [dict(q=grib_cases.random_q(rng, S, nb), nbits=nb, E=int(rng.integers(-6, 3)), D=int(b == 2),
                  ref=float(np.float32(rng.normal(0.0, 300.0)))) for b, nb in enumerate(nbits)]
    x_bytes = offs[2] + (S * 12 + 7) // 8 + 5
    buf = np.empty(x_bytes, U8)                                         # virtual
    rows = np.zeros(3, GRIB_ROW_DTYPE)
    for b, s in enumerate(specs):
        data = np.frombuffer(grib_cases.pack_bits(s["q"], s["nbits"]), U8)
        buf[offs[b]:offs[b] + data.size] = data
        rows[b] = (offs[b], s["ref"], 2.0 ** s["E"], 10.0 ** s["D"], s["nbits"], 0)
    fld = np.stack([grib_cases.decode_ref(s["q"], s["ref"], s["E"], s["D"]) for s in specs])
    Xd, Yd = far.x(fc.near_layout(3, S), F32, fld), far.y(fc.near_layout(3, op.n_dst), F64)
    _lib.call("smm_apply", op.handle, Xd.ptr, _lib.SMM_F32, S, Yd.ptr, _lib.SMM_F64, op.n_dst, 3, AREA_MIN,
              SELL | _lib.APPLY_MASKED, None)
    want = Yd.rows()
    fc.check_rows(want, reference(csr, fld, imask, frac), "smm_apply on the decoded field")
    y = np.frombuffer(bytes([fc.SENTINEL]) * want.nbytes, F64).reshape(want.shape).copy()
    _lib.host_stats(reset=True)
    _lib.call("smm_apply_host_grib", op.handle, _vp(buf.ctypes.data), x_bytes,
              ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)), _vp(y.ctypes.data), _lib.SMM_F64,
              op.n_dst, 3, AREA_MIN, _lib.APPLY_MASKED, chunk_rows)
    assert _lib.host_stats(reset=True)["chunks"] == -(-3 // chunk_rows)
    assert np.array_equal(y.view(np.uint64), want.view(np.uint64)), np.argwhere(y.view(np.uint64) != want.view(np.uint64))[:3]
