"""smm_gradients and smm_apply_cols at offsets past 2^31 and 2^32 elements: the entries that came after
tests/test_gpu_far_offsets.py and tests/test_gpu_grib_far_offsets.py, with the buffers, the fixture and the memory rule of
the first (a case skips only when `mem_info()` reports less than its need + 2 GiB; at most about 40 GiB a case).

Both kernels form `b * ldx`, `b * ld_row`, `p * ld_plane`, `j * ldy` and `j * g_ld_row`, and both entries form `r0 * ldx`,
`r0 * ld_row` and `r0 * ldy` on the host when the batch is cut into rounds: every case runs in one launch and cut.  The grid
is 257 x 33 -- two tiles, two bands -- on stretched axes (tests/grad_cases.py).  X holds decoys, G and Y the byte 0x42; the
true rows must hold the reference's bits and the windows at every alias of every true row their 0x42
(tests/far_cases.py; tests/test_far_cases.py shows that a narrowed `ld_row` and a narrowed `ld_plane` are caught)."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import SparseOperator, _lib
from tests import far_cases as fc
from tests import grad_cases as gc
from tests.helpers import random_links
from tests.test_gpu_far_offsets import F32, F64, Buf, Far, far, layouts      # noqa: F401  (far: the fixture)
from tests.test_gpu_gradients import stacked_links

pytestmark = pytest.mark.gpu

NX, NY = 257, 33
S = NX * NY
GRID_BLOCKS = 4                  # workgroups one batch row of the stencil takes: a launch limit of 4 is one row a launch
AREA_MIN = 0.37
DT = {"f32": (F32, _lib.SMM_F32), "f64": (F64, _lib.SMM_F64)}
KINDS = {"sphere": 3, "index": 4}
_vp = ctypes.c_void_p


@functools.lru_cache(maxsize=None)
def rule_of(kind):
    return gc.stretched_rule(NX, NY, True, KINDS[kind])


def gradients(rule, X, code, ldx, G, ld_plane, ld_row, n_batch, limit):
    _lib.call("smm_debug_set_grid_limit", limit)
    try:
        _lib.call("smm_gradients", rule.plan(0), X.ptr, code, ldx, G.ptr, ld_plane, ld_row, n_batch, None)
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)


# ------------------------------------------------------------------ smm_gradients

@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("kind", KINDS)
def test_gradients_x_far(far, kind, dt):
    """5 rows on a pitch of 2^30 + K: `b * ldx` in the kernel, `r0 * ldx` on the host with one row a launch."""
    rule, (dtype, code), B = rule_of(kind), DT[dt], 5
    x = gc.seam_batch(NX, NY, B, dtype)
    lx, ldx = fc.rows_layout(B, S)
    assert ldx > 1 << 30 and lx.crossed() == (3, 1)
    X = far.x(lx, dtype, x)
    G = far.y(fc.near_layout(B * rule.n_planes, S), F64)
    want = rule.gradients_rows(x).reshape(B * rule.n_planes, S)
    for limit in (0, GRID_BLOCKS):
        G.arr.fill_bytes(fc.SENTINEL)
        gradients(rule, X, code, ldx, G, S, rule.n_planes * S, B, limit)
        G.check(want, f"smm_gradients {kind} {dt} X far, grid limit {limit}")


@pytest.mark.parametrize("kind", KINDS)
def test_gradients_g_far_by_row(far, kind):
    """3 rows of planes on `ld_row` = 2^31 + K, the planes of a row near each other."""
    rule, B = rule_of(kind), 3
    x = gc.seam_batch(NX, NY, B, np.float32)
    lg, ld_row = fc.rows_layout(B, S, inner=rule.n_planes)
    ld_plane = lg.offsets[1] - lg.offsets[0]
    assert ld_row > 1 << 31 and ld_row >= (rule.n_planes - 1) * ld_plane + S
    X = far.x(fc.near_layout(B, S), F32, x)
    G = far.y(lg, F64)
    want = rule.gradients_rows(x).reshape(B * rule.n_planes, S)
    for limit in (0, GRID_BLOCKS):
        G.arr.fill_bytes(fc.SENTINEL)
        gradients(rule, X, _lib.SMM_F32, S, G, ld_plane, ld_row, B, limit)
        G.check(want, f"smm_gradients {kind} G far by row, grid limit {limit}")


def test_gradients_g_far_by_plane(far):
    """One row, its three planes on `ld_plane` = 2^31 + K."""
    rule = rule_of("index")
    x = gc.seam_batch(NX, NY, 1, np.float64)
    lg, ld_plane = fc.rows_layout(3, S)
    assert ld_plane > 1 << 31 and lg.crossed() == (2, 1)
    X = far.x(fc.near_layout(1, S), F64, x)
    G = far.y(lg, F64)
    gradients(rule, X, _lib.SMM_F64, S, G, ld_plane, 3 * ld_plane, 1, 0)
    G.check(rule.gradients_rows(x).reshape(3, S), "smm_gradients G far by plane")


# ------------------------------------------------------------------ smm_apply_cols

D_COLS = 300


@functools.lru_cache(maxsize=None)
def cols_operator():
    """A K = 4 operator on the grid, its epilogue, and the CSR of the stacked statement."""
    rng = np.random.default_rng([gc.SEED, 80])
    src, dst, _ = random_links(rng, S, D_COLS, 2400, dup_frac=0.1)
    w = rng.uniform(-0.5, 1.5, size=(src.size, 4))
    op = SparseOperator(S, D_COLS, src, dst, w, device=0, columns=True)
    imask, frac = (rng.random(D_COLS) > 0.1).astype(np.int32), rng.random(D_COLS)
    op.set_epilogue(imask, frac)
    return op, oracle.coo_to_csr_c(S * 4, D_COLS, *stacked_links(src, dst, w)), imask, frac


@pytest.mark.parametrize("case", ["x-f32", "x-f64", "y-f64"])
def test_apply_cols(far, case):
    """5 rows on a pitch of 2^30 + K.  With scratch for all 5 the gather blocks 4 batch rows a thread and `j * ldx` (or
    `j * ldy`) crosses 2^32 inside the kernel; with scratch for 2 the rounds start at rows 0, 2 and 4 on the host."""
    side, dt = case.split("-")
    (dtype, code), B = DT[dt], 5
    rule = rule_of("index")
    op, csr, imask, frac = cols_operator()
    x = gc.seam_batch(NX, NY, B, dtype)
    want = oracle.apply_c(csr, rule.stacked(x), masked=True, dst_imask=imask, dst_frac=frac, area_min=AREA_MIN)
    assert np.isnan(want).any() and np.isfinite(want).any()
    lx, ldx, ly, ldy = layouts(side, B, S, D_COLS)
    X, Y = far.x(lx, dtype, x), far.y(ly, F64)
    for rows in (5, 2):
        nbytes = rows * rule.n_planes * S * 8
        scratch = far.alloc(nbytes, np.uint8)
        Y.arr.fill_bytes(fc.SENTINEL)
        _lib.call("smm_apply_cols", op.handle, rule.plan(0), X.ptr, code, ldx, Y.ptr, _lib.SMM_F64, ldy, B, AREA_MIN,
                  _lib.APPLY_MASKED, _vp(scratch.ptr), nbytes, None)
        Y.check(want, f"smm_apply_cols {dt} far {side}, scratch for {rows} rows")
