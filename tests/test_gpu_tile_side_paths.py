"""Side paths of the LDS tile kernel that the dispatch-cell cases (tests/cell_cases.py) do not reach: their operators
have source rows of a multiple of 16 elements, links in every full block, long source rows and contiguous batches.
Each case here is launched through a named walk of the 4-wave shape (register staging with 1 / 2 / 4 batch rows per
step, LDS-DMA with 1 / 2 / 4), identified through `launch_info`, and compared bit for bit with the CPU oracle, for
f32 and f64 fields, plain and SKIPNA.

  row-end piece      n_src = 1029 (f32) / 1027 (f64): the last 16-B staging piece of a source row is loaded early
                     and realigned; the last destination block links to the last source cells.  Register staging
                     only: LDS-DMA refuses rows that are no multiple of 16 B.
  block, no links    a full block of 256 destination rows without a link between two blocks that have links.
  tiny source row    n_src = 3 (f32) / 1 (f64): shorter than one 16-B piece, gathered straight from the field.
  batch end, strides (n_outer, 2 levels, n_inner) fields of 7 x 1 and 5 x 2 batch rows walked 3 rows per workgroup:
                     the row walker wraps inside a step and inside a walk tail, outer and inner strides differ.

Operators of at most 805 destination rows and 8 links per row.  The single-wave forms (rows of 17 or more links:
SPLIT and streamed rows among them) are outside these sizes: the block shape follows the operator's own plan, and
rows of at most 16 links get the 4-wave shape.  What the existing files reach for those forms, by reading:
tests/test_gpu_dispatch_cells.py runs every single-wave cell (register and DMA staging, SPLIT, streamed) with batches
that are no multiple of the walk, on contiguous fields whose rows are a multiple of 16 elements and whose full
blocks all have links; tests/test_gpu_long_rows.py runs SPLIT and streamed rows on contiguous fields of odd
row lengths (n_src = n_dst * stride + max_len + 7: the row-end piece exists, in the last block only if a row there
links the last cells) and one (3, 2 levels, 2) strided group through the split form.  So for the single-wave forms
the strided batch end is reached once, the row-end piece by chance of the drawn links, and a block without links
and the tiny source row by no pinned case."""
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import OperatorGroup, SparseOperator, _lib, to_device
from tests.helpers import bits_equal, field, skipna_ref

pytestmark = pytest.mark.gpu
T = _lib.APPLY_KERNEL_TILE
SEED = 20261018
XDT = {"f32": np.float32, "f64": np.float64}
REG = [("reg", r) for r in (1, 2, 4)]
DMA = [("dma", r) for r in (1, 2, 4)]
AREA_MIN = 0.37


def _knobs(staging, r, walk):
    return dict(tile_staging=_lib.STAGING_DMA if staging == "dma" else 1, tile_rows_per_step=r, tile_walk=walk)


@functools.lru_cache(maxsize=None)
def _operator(n_src, n_dst, empty_block):
    """Banded rows of 0 .. 8 links whose windows move from the first to the last source cell; the last row links the
    last source cells.  empty_block: rows 256 .. 511 have no link."""
    rng = np.random.default_rng([SEED, n_src, n_dst, int(empty_block)])
    src, dst = [], []
    span = min(24, n_src)
    for d in range(n_dst):
        if empty_block and 256 <= d < 512:
            continue
        ln = min(int(rng.integers(0, 9)), span)
        base = d * (n_src - span) // max(n_dst - 1, 1)
        cols = base + rng.choice(span, size=ln, replace=False)
        if d == n_dst - 1:
            cols = np.union1d(cols, [n_src - 1, max(n_src - 3, 0)])
        cols = np.unique(cols)
        src.append(cols)
        dst.append(np.full(cols.size, d))
    src, dst = np.concatenate(src), np.concatenate(dst)
    w = rng.uniform(-0.2, 1.0, size=src.size)
    perm = rng.permutation(src.size)
    src, dst, w = (src[perm] + 1).astype(np.int32), (dst[perm] + 1).astype(np.int32), w[perm]
    op = SparseOperator(n_src, n_dst, src, dst, w, device=0)
    imask = (rng.random(n_dst) > 0.1).astype(np.int32)
    frac = rng.random(n_dst)
    op.set_epilogue(imask, frac)
    csr = oracle.coo_to_csr(n_src, n_dst, src, dst, w)
    lens = np.diff(csr[0])
    assert lens.max() <= 16 and csr[1][-1] == n_src - 1
    if empty_block:
        assert lens[256:512].max() == 0 and lens[:256].max() > 0 and lens[512:].max() > 0
    return op, csr, imask, frac


def _reference(csr, x, imask, frac, skipna):
    if skipna:
        return skipna_ref(csr, x, True, imask, frac, AREA_MIN, np.float64)
    return oracle.apply_c(csr, x, True, imask, frac, AREA_MIN).astype(np.float64)


def _check(rng, n_src, n_dst, empty_block, xt, staging, r, skipna, batch=7, walk=5):
    op, csr, imask, frac = _operator(n_src, n_dst, empty_block)
    knobs = _knobs(staging, r, walk)
    with _lib.tuning(**knobs):
        info = op.launch_info(batch, XDT[xt], flags=T | (_lib.APPLY_SKIPNA if skipna else 0))
    assert info["kernel"] == ("tile-dma" if staging == "dma" else "tile"), info
    assert (info["rows_per_block"], info["rows_per_step"], info["j_per_block"]) == (256, r, walk), info
    x = field(rng, batch, n_src, XDT[xt], nan_frac=0.03, inf_frac=0.005)
    x[0, n_src - 1], x[-1, n_src - 1] = -123456.75, np.nan
    ref = _reference(csr, x, imask, frac, skipna)
    with _lib.tuning(**knobs):
        y = op.apply(to_device(x), masked=True, remap_area_min=AREA_MIN, skipna=skipna, flags=T).to_host()
    bits_equal(y, ref)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("staging,r", REG, ids=lambda v: str(v))
@pytest.mark.parametrize("xt", ["f32", "f64"])
def test_row_end_piece(hip, rng, xt, staging, r, skipna):
    _check(rng, 1029 if xt == "f32" else 1027, 3 * 256 + 37, False, xt, staging, r, skipna)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("staging,r", REG + DMA, ids=lambda v: str(v))
@pytest.mark.parametrize("xt", ["f32", "f64"])
def test_block_without_links(hip, rng, xt, staging, r, skipna):
    _check(rng, 1040, 3 * 256 + 37, True, xt, staging, r, skipna)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("staging,r", REG, ids=lambda v: str(v))
@pytest.mark.parametrize("xt", ["f32", "f64"])
def test_tiny_source_row(hip, rng, xt, staging, r, skipna):
    _check(rng, 3 if xt == "f32" else 1, 2 * 256 + 37, False, xt, staging, r, skipna)


@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("n_outer,n_inner", [(7, 1), (5, 2)])
@pytest.mark.parametrize("staging,r,walk", [("reg", 1, 3), ("reg", 2, 3), ("dma", 1, 3), ("dma", 2, 3),
                                            ("reg", 4, 6), ("dma", 4, 6)], ids=lambda v: str(v))
@pytest.mark.parametrize("xt", ["f32", "f64"])
def test_batch_end_with_strides(hip, rng, xt, staging, r, walk, n_outer, n_inner, skipna):
    """Two data levels of one operator: the outer stride is 2 n_inner rows, the inner stride one row, and the results
    go out transposed.  7 and 10 batch rows are no multiple of the 3-row walk nor of R = 2.  Steps of four rows need
    a walk of at least four (shorter walks halve R): a 6-row walk, of which 7 and 10 are no multiple either, and
    whose 6-row walks and 1- / 4-row tails are no multiple of R = 4."""
    n_src, n_dst, n_lev = 1040, 3 * 256 + 37, 2
    op, csr, imask, frac = _operator(n_src, n_dst, False)
    grp = OperatorGroup([op])
    knobs = _knobs(staging, r, walk)
    flags = T | (_lib.APPLY_SKIPNA if skipna else 0)
    with _lib.tuning(**knobs):
        info = grp.launch_info(n_outer, n_lev, n_inner, XDT[xt], flags=flags)
    assert info["kernel"] == ("tile-dma" if staging == "dma" else "tile"), info
    assert (info["rows_per_step"], info["j_per_block"]) == (r, walk), info
    x = field(rng, n_outer * n_lev * n_inner, n_src, XDT[xt], nan_frac=0.03, inf_frac=0.005)
    ref = _reference(csr, x, imask, frac, skipna).reshape(n_outer, n_lev, n_inner, n_dst).transpose(0, 2, 1, 3)
    lev = np.zeros(n_lev, np.int32)
    with _lib.tuning(**knobs):
        y = grp.apply(to_device(x.reshape(n_outer, n_lev, n_inner, n_src)), lev, np.ones(1, np.uint8), masked=True,
                      remap_area_min=AREA_MIN, transpose=True, skipna=skipna, flags=T).to_host()
    bits_equal(y, np.ascontiguousarray(ref))
