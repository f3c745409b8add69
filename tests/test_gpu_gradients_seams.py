"""smm_gradients on its tile and band seams and smm_apply_cols in every instantiation, on the inputs of
tests/grad_cases.py (tests/test_grad_cases.py shows on the CPU what those inputs catch).

The stencil: grids just around one and two tiles of 256 columns and bands of 32 rows, periodic and regional, on stretched
axes -- every column and row with a table entry of its own -- against `GradientRule` and, for the index kind, against the
closed-form planes of a bilinear field.  The gather: K = 2 (one plane: `OnePlaneRule`), 3 and 4 with float32 and float64
fields in batches of 1, 2-3 and 4 and more rows, against the stacked statement through the C oracle.  Everything is bit
equality."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import DeviceArray, SparseOperator, _lib, to_device
from smmregrid_amd.gradients import GRAD_I, GRAD_IJ, GRAD_J
from tests import grad_cases as gc
from tests.helpers import bits_equal, field, ragged_links, random_links
from tests.test_gpu_gradients import Case

pytestmark = pytest.mark.gpu
DT = {"f32": np.float32, "f64": np.float64}
SENTINEL = 0x42
_vp = ctypes.c_void_p


def dummy_operator(S):
    """`SparseOperator.gradients` lives on an operator: any one of S source cells."""
    return SparseOperator(S, 1, np.array([1], np.int32), np.array([1], np.int32), np.array([1.0]), device=0)


def padded(x, pad, value=7.0):
    """x (B, S) as rows of pitch S + pad: the pad is never read into a plane."""
    xp = np.full((x.shape[0], x.shape[1] + pad), value, dtype=x.dtype)
    xp[:, :x.shape[1]] = x
    return xp


class limited:
    """smm_debug_set_grid_limit for a block."""

    def __init__(self, n):
        self.n = n

    def __enter__(self):
        _lib.call("smm_debug_set_grid_limit", self.n)

    def __exit__(self, *exc):
        _lib.call("smm_debug_set_grid_limit", 0)


# ------------------------------------------------------------------ the stencil on the seam grids

@pytest.mark.parametrize("dt", DT)
@pytest.mark.parametrize("num_wgts", [3, 4])
@pytest.mark.parametrize("periodic", [True, False], ids=["periodic", "regional"])
@pytest.mark.parametrize("grid", gc.SEAM_GRIDS, ids=lambda g: f"{g[0]}x{g[1]}")
def test_gradients_on_tile_and_band_seams(hip, grid, periodic, num_wgts, dt):
    """B = 3 on 513x33 (3 x 2 blocks a row) and on 257x65 (2 x 3) tells the three-way split of the block index apart."""
    nx, ny = grid
    S = nx * ny
    op = dummy_operator(S)
    for descending in (False, True):
        rule = gc.stretched_rule(nx, ny, periodic, num_wgts, descending)
        for n_batch in (1, 2, 3):
            x = gc.seam_batch(nx, ny, n_batch, DT[dt])
            got = op.gradients(to_device(padded(x, 5)), rule).to_host()
            assert got.shape == (n_batch, rule.n_planes, S)
            bits_equal(got, rule.gradients_rows(x))
        if rule.kind == "index":
            coeffs = ((3, 5, 2), (1, 1, 1))
            x = np.stack([gc.known_field(nx, ny, *abc, DT[dt]).ravel() for abc in coeffs])
            got = op.gradients(to_device(padded(x, 5)), rule).to_host()
            want = np.stack([gc.known_answer(nx, ny, periodic, descending, *abc).reshape(3, S) for abc in coeffs])
            bits_equal(got, want)


@pytest.mark.parametrize("num_wgts", [3, 4])
@pytest.mark.parametrize("kind", [GRAD_I, GRAD_J], ids=["g_i", "g_j"])
def test_one_plane_alone(hip, kind, num_wgts):
    nx, ny = 257, 33
    full = gc.stretched_rule(nx, ny, True, num_wgts)
    one = gc.OnePlaneRule(full, kind)
    op = dummy_operator(nx * ny)
    x = gc.seam_batch(nx, ny, 3, np.float32)
    got = op.gradients(to_device(padded(x, 5)), one).to_host()
    assert got.shape == (3, 1, nx * ny)
    bits_equal(got, one.gradients_rows(x))
    bits_equal(got[:, 0], full.gradients_rows(x)[:, full.plane_kind.index(kind)])


def test_a_cross_plane_alone_is_refused(hip):
    rule = gc.stretched_rule(257, 33, True, 4)
    with pytest.raises(_lib.SmmError) as err:
        gc.create_plan(rule.tables(), (GRAD_IJ,), 0)
    assert err.value.code == _lib.SMM_ERR_INVALID and "J plane" in str(err.value)


@pytest.mark.parametrize("limit", [6, 7])
def test_the_batch_is_cut_on_a_grid_of_six_blocks_a_row(hip, limit):
    nx, ny = 513, 33
    rule = gc.stretched_rule(nx, ny, True, 4)
    op = dummy_operator(nx * ny)
    x = gc.seam_batch(nx, ny, 4, np.float64)
    with limited(limit):                       # one row a launch either way: 7 // 6 == 1
        got = op.gradients(to_device(padded(x, 5)), rule).to_host()
    bits_equal(got, rule.gradients_rows(x))
    with limited(5):
        with pytest.raises(_lib.SmmError) as err:
            op.gradients(to_device(x), rule)
    assert err.value.code == _lib.SMM_ERR_INVALID and "one batch row alone" in str(err.value)


# ------------------------------------------------------------------ the gather fuzz

def fuzz_case(p):
    """(Case, x, rule) of the draw p (tests/grad_cases.py)."""
    rng = np.random.default_rng([gc.SEED, 78, p["seed"]])
    nx, ny = p["grid"]
    full = gc.stretched_rule(nx, ny, p["periodic"], p["num_wgts"], descending=bool(p["seed"] % 2))
    rule = gc.OnePlaneRule(full, p["plane"]) if p["K"] == 2 else full
    S, D, K = rule.size, p["D"], p["K"]
    if p["links"] == "random":
        src, dst, _ = random_links(rng, S, D, max(1, D * int(rng.integers(2, 9))), dup_frac=0.1)
        if D > 2:
            dst[dst == 2] = 1                                      # a row without links
    else:
        src, dst, _ = ragged_links(rng, S, D, max_len=200)         # rows of up to 200 links, 15 % of them empty
    if src.size == 0:
        src, dst = np.array([S], np.int32), np.array([D], np.int32)
    n = src.size
    w = rng.uniform(-0.5, 1.5, size=(n, K))
    w[rng.random(n) < 0.1] = 0.0                                   # links whose columns are all zero
    w[rng.random(n) < 0.1, 0] = 0.0                                # ... and whose column 0 alone is
    imask, frac = (rng.random(D) > 0.2).astype(np.int32), rng.random(D)
    x = field(rng, p["B"], S, DT[p["dtype"]], nan_frac=0.03, inf_frac=0.01)
    return Case(src, dst, w, rule, D, imask, frac), x, rule


@pytest.mark.parametrize("seed", gc.FUZZ_SEEDS)
def test_apply_cols_fuzz(hip, seed):
    p = gc.fuzz_draw(seed)
    c, x, rule = fuzz_case(p)
    assert c.op.n_cols == p["K"] == rule.n_planes + 1
    got = c.op.apply(to_device(x), masked=p["masked"], remap_area_min=p["area_min"], gradients=rule,
                     scratch_rows=p["scratch_rows"]).to_host()
    bits_equal(got, c.ref(x, p["masked"], p["area_min"]))
    assert not np.isfinite(x).all()


def test_the_fuzz_runs_all_18_instantiations():
    """Every K with every field type at 1, 2 and 4 batch rows per thread."""
    ran = set().union(*(gc.fuzz_instantiations(gc.fuzz_draw(s)) for s in gc.FUZZ_SEEDS))
    assert ran == set(gc.INSTANTIATIONS) and len(ran) == 18


# ------------------------------------------------------------------ side cases of smm_apply_cols

@pytest.fixture(scope="module")
def side(hip):
    """K = 4 on 12x7, D = 600: three blocks of destination rows."""
    rng = np.random.default_rng([gc.SEED, 79])
    rule = gc.stretched_rule(12, 7, True, 4)
    D = 600
    src, dst, _ = random_links(rng, rule.size, D, 3000, dup_frac=0.1)
    w = rng.uniform(-0.5, 1.5, size=(src.size, 4))
    c = Case(src, dst, w, rule, D, (rng.random(D) > 0.2).astype(np.int32), rng.random(D))
    return c, field(rng, 7, rule.size, np.float64, nan_frac=0.03, inf_frac=0.01)


def raw_apply_cols(c, x_dev, ldx, y_dev, ldy, n_batch, scratch_rows, flags=0, area_min=0.0):
    """smm_apply_cols itself; the status, not an exception."""
    nbytes = max(scratch_rows, 1) * c.rule.n_planes * c.S * 8
    scratch = DeviceArray((nbytes,), np.uint8)
    rc = _lib.load().smm_apply_cols(c.op.handle, c.rule.plan(0), _vp(x_dev.ptr), _lib.SMM_F64, ldx, _vp(y_dev.ptr),
                                    _lib.SMM_F64, ldy, n_batch, area_min, flags, _vp(scratch.ptr), nbytes, None)
    _lib.call("smm_device_sync")
    return rc, (_lib.load().smm_last_error() or b"").decode()


def test_padded_rows_keep_their_pad(side):
    c, x = side
    B, S, D = x.shape[0], c.S, c.D
    ldx, ldy = S + 3, D + 7
    y = DeviceArray((B, ldy), np.float64).fill_bytes(SENTINEL)
    rc, msg = raw_apply_cols(c, to_device(padded(x, 3)), ldx, y, ldy, B, B, flags=_lib.APPLY_MASKED, area_min=0.25)
    assert rc == _lib.SMM_OK, msg
    got = y.to_host()
    bits_equal(np.ascontiguousarray(got[:, :D]), c.ref(x, True, 0.25))
    assert (np.ascontiguousarray(got[:, D:]).view(np.uint8) == SENTINEL).all()


def test_no_fill_gathers_the_raw_field(side):
    """The case that found the padded slots: a row ending in an inf cell, shorter than its slice, gave NaN (+0.0 * inf
    from the slots that repeat its last column) where its own links give -inf."""
    c, x = side
    X = c.rule.stacked(x).reshape(x.shape[0], c.S, c.K)
    X[:, :, 0] = x                                                 # slot 0 raw: NaN and inf as they are
    ref = oracle.apply_c(c.csr, X.reshape(x.shape[0], -1), masked=True, dst_imask=c.imask, dst_frac=c.frac, area_min=0.25,
                         fill=False)
    got = c.op.apply(to_device(x), masked=True, remap_area_min=0.25, gradients=c.rule, flags=_lib.APPLY_NO_FILL).to_host()
    bits_equal(got, ref)
    filled = c.op.apply(to_device(x), masked=True, remap_area_min=0.25, gradients=c.rule).to_host()
    bits_equal(filled, c.ref(x, True, 0.25))
    assert np.isnan(x).any() and np.isinf(x).any() and not np.array_equal(got, filled, equal_nan=True)


def test_an_empty_batch_and_an_empty_destination_touch_nothing(side):
    c, x = side
    y = DeviceArray((64,), np.float64).fill_bytes(SENTINEL)
    rc, msg = raw_apply_cols(c, to_device(x), c.S, y, c.D, 0, 1)
    assert rc == _lib.SMM_OK, msg
    none = np.zeros(0, np.int32)
    c0 = SparseOperator(c.S, 0, none, none, np.zeros((0, 4)), device=0, columns=True)
    assert (c0.n_dst, c0.n_cols) == (0, 4)
    empty = type("Empty", (), {"op": c0, "rule": c.rule, "S": c.S})
    rc, msg = raw_apply_cols(empty, to_device(x), c.S, y, 0, x.shape[0], x.shape[0])
    assert rc == _lib.SMM_OK, msg
    assert (y.to_host().view(np.uint8) == SENTINEL).all()


def test_apply_cols_under_the_grid_limit(side):
    """D = 600 is three blocks a j-tile.  At a limit of 3 a round of 4 rows fits (one j-tile), but 7 rows cut into 4 + 3
    would not: 3 rows are two j-tiles, 6 blocks.  The rounds are chosen so that the last one fits as well."""
    c, x = side
    assert x.shape[0] == 7
    whole = c.op.apply(to_device(x), gradients=c.rule, scratch_rows=7).to_host()
    bits_equal(whole, c.ref(x))
    with limited(3):
        got = c.op.apply(to_device(x), gradients=c.rule, scratch_rows=7).to_host()
    bits_equal(got, whole)
    y = DeviceArray((7, c.D), np.float64)
    with limited(2):
        rc, msg = raw_apply_cols(c, to_device(x), c.S, y, c.D, 7, 7)
    assert rc == _lib.SMM_ERR_INVALID and "one batch row alone" in msg
