"""smm_group_apply_host on a group whose levels are thin or empty and whose target is larger than its source
(S = 288 = r24x12, D = 648 = r36x18): a level of U used cells adds U * batch * xsz bytes of X to a level-major chunk but
a full slab of batch * D * ysz bytes of Y, so the chunk plan (smm::plan_group_chunks) bounds X + Y.  A data level with
no used cell at all puts a slab of zero rows into the packed chunk (the next level's slab starts at the same address),
packs an empty list of cells, and -- alone in a chunk -- ships an H2D copy of 0 bytes.  Every result is bit-equal to the
oracle and to the whole-row pipeline; the copies' byte counts are exact."""
import ctypes
import functools

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import OperatorGroup, SparseOperator, _lib, pinned_empty
from tests.helpers import assert_same, skipna_ref

pytestmark = pytest.mark.gpu

S, D, N_OUTER = 288, 648, 40
USED = (130, 1, 2, 3, 0, 1)            # n_used_src of the six members: 45 % of the cells, three thin ones, none, one
MASKED_LEVELS = np.array([1, 0, 1, 0, 1, 1], np.uint8)
AREA_MIN = 0.5
ORDERS = {
    "wide, thin, empty": np.array([0, 1, 2, 3, 5, 4], np.int32),
    "empty first and last, repeated": np.array([4, 0, 1, 4, 4, 2, 4], np.int32),
    "a subset in reverse": np.array([5, 4, 2, 0], np.int32),
}
# SMM_TUNE_HOST_CHUNK_KB: 0 = the default rule; 1024 = level-major chunks of several thin levels; 256 per inner index =
# level-major chunks that the Y bound ends after one level each (the inequalities: _budget_facts)
KB_SEVERAL, KB_Y_BOUND = 1024, {1: 256, 2: 512}


def _links(rng):
    """The six link lists (1-based), exact in their used source cells."""
    cells = np.sort(rng.permutation(S)[:USED[0]])
    src, dst = [], []
    for d in range(D):                                     # rows of 1 to 9 links; the first 130 rows cover every used cell
        n = int(rng.integers(1, 9 if d < cells.size else 10))
        cols = set(rng.choice(cells, size=n, replace=False).tolist())
        if d < cells.size:
            cols.add(int(cells[d]))
        src += sorted(cols)
        dst += [d] * len(cols)
    wide = (np.array(src) + 1, np.array(dst) + 1)
    thin = [([17, 17, 17], [0, 5, 647]),                                   # one used cell, three rows
            ([3, 287, 287, 3], [1, 300, 301, 301]),                        # two
            ([0, 100, 200, 100], [10, 11, 640, 640])]                      # three
    out = [wide] + [(np.array(s) + 1, np.array(d) + 1) for s, d in thin]
    out.append((np.zeros(0, np.int64), np.zeros(0, np.int64)))             # no links at all
    out.append((np.array([S]), np.array([D])))                             # a single link into the last destination cell
    return [(s.astype(np.int32), d.astype(np.int32), rng.uniform(0.1, 1.0, size=s.size)) for s, d in out]


@pytest.fixture(scope="module")
def thin(hip, rng):
    links = _links(rng)
    imask = (rng.random((len(links), D)) < 0.9).astype(np.int32)
    frac = rng.random((len(links), D))
    ops = []
    for (src, dst, w), im, fr in zip(links, imask, frac):
        op = SparseOperator(S, D, src, dst, w, device=0)
        op.set_epilogue(im, fr)
        ops.append(op)
    assert tuple(op.n_used_src for op in ops) == USED
    grp = OperatorGroup(ops)
    csrs = [oracle.coo_to_csr_c(S, D, *lk) for lk in links]

    @functools.lru_cache(maxsize=None)
    def case(order, n_inner, dtype):
        """(x, oracle result in concat order (n_lev, n_outer, n_inner, D)), made once per walk and left unchanged"""
        lev = ORDERS[order]
        x = (10.0 + 5.0 * rng.standard_normal((N_OUTER, lev.size, n_inner, S))).astype(dtype)
        x[rng.random(x.shape) < 0.02] = np.nan
        ref = oracle.apply_levels(csrs, x, 1, lev, MASKED_LEVELS.astype(bool), imask, frac, AREA_MIN, transpose=False)
        x.setflags(write=False)
        ref.setflags(write=False)
        return x, ref

    yield dict(grp=grp, csrs=csrs, imask=imask, frac=frac, case=case)
    grp.close()


def _budget_facts(lev, n_inner, xsz, ysz):
    """The byte counts of a call, and the inequalities that make KB_SEVERAL and KB_Y_BOUND what their names say."""
    used = [USED[w] for w in lev]
    batch = N_OUTER * n_inner                               # batch entries per level
    assert 0 < sum(used) * 5 <= lev.size * S * 4            # the packing variant applies
    x_all, y_level = sum(used) * batch * xsz, batch * D * ysz
    for kb in (KB_SEVERAL, KB_Y_BOUND[n_inner]):
        # level-major needs all 40 outer indices of the widest level within four budgets (else: whole rows)
        assert 4 * (kb << 10) // (max(used) * n_inner * xsz) >= N_OUTER
    # the default rule: twice the 40 outer indices of all levels stay below the 32 MiB that a chunk keeps (a block of at
    # least 64 outer indices, whole multiples of 32): one packed block
    assert 2 * (x_all + lev.size * y_level) <= 32 << 20
    # several levels per chunk: all of X and any two levels' Y fit one budget, so every chunk but the last holds two
    # or more
    assert x_all + 2 * y_level <= KB_SEVERAL << 10
    # the Y bound ends every chunk: all of X fits one budget (X alone would make one chunk) and so does one level's Y,
    # two levels' Y do not
    assert max(x_all, y_level) <= (KB_Y_BOUND[n_inner] << 10) < 2 * y_level
    return dict(h2d=x_all, d2h=lev.size * y_level, y_level=y_level, x_all=x_all)


def _check_chunks(kb, chunks, n_lev, facts, y_bound):
    if kb == 0:
        assert chunks == 1
        return
    target = kb << 10
    assert chunks >= -(-facts["d2h"] // target)             # no chunk's Y beyond the budget (X alone: one chunk)
    if y_bound:
        assert chunks == n_lev                              # one level each
    else:
        assert chunks <= (n_lev + 1) // 2                   # every chunk but the last holds several levels


@pytest.mark.parametrize("order", list(ORDERS))
@pytest.mark.parametrize("transpose", [True, False])
@pytest.mark.parametrize("n_inner,dtype", [(1, np.float64), (2, np.float32)])
def test_thin_and_empty_levels_through_every_chunk_plan(thin, n_inner, dtype, transpose, order):
    grp, lev = thin["grp"], ORDERS[order]
    x, ref = thin["case"](order, n_inner, dtype)
    if transpose:
        ref = np.moveaxis(ref, 0, -2)
    kw = dict(masked=True, remap_area_min=AREA_MIN, transpose=transpose)
    facts = _budget_facts(lev, n_inner, x.itemsize, 8)
    whole = grp.apply_host(x, lev, MASKED_LEVELS, flags=_lib.APPLY_HOST_NO_PACK, **kw)
    assert_same(whole, ref, exact=True)
    for kb in (0, KB_SEVERAL, KB_Y_BOUND[n_inner]):
        with _lib.tuning(host_chunk_kb=kb):
            _lib.host_stats(reset=True)
            y = grp.apply_host(x, lev, MASKED_LEVELS, **kw)
            st = _lib.host_stats(reset=True)
        print(f"{order}, n_inner={n_inner}, host_chunk_kb={kb}: chunks {st['chunks']}, h2d_bytes {st['h2d_bytes']}, "
              f"d2h_bytes {st['d2h_bytes']}")
        assert_same(y, ref, exact=True)
        assert_same(y, whole, exact=True)
        assert st["h2d_bytes"] == facts["h2d"]              # sum_l U_l * batch * xsz: the used cells and nothing else
        assert st["d2h_bytes"] == facts["d2h"]              # Y comes back once
        _check_chunks(kb, st["chunks"], lev.size, facts, kb == KB_Y_BOUND[n_inner])


def test_skipna_on_thin_and_empty_levels(thin):
    """SMM_APPLY_SKIPNA through the level-major chunks, against the rule restated per level (helpers.skipna_ref)."""
    order = "empty first and last, repeated"
    grp, lev = thin["grp"], ORDERS[order]
    x = thin["case"](order, 1, np.float64)[0]
    ref = np.stack([skipna_ref(thin["csrs"][w], x[:, l, 0], masked=bool(MASKED_LEVELS[w]), imask=thin["imask"][w],
                               frac=thin["frac"][w], area_min=AREA_MIN) for l, w in enumerate(lev)], axis=1)[:, None]
    kw = dict(masked=True, remap_area_min=AREA_MIN, skipna=True)
    whole = grp.apply_host(x, lev, MASKED_LEVELS, flags=_lib.APPLY_HOST_NO_PACK, **kw)
    assert_same(whole, ref, exact=True)
    for kb in (0, KB_SEVERAL, KB_Y_BOUND[1]):
        with _lib.tuning(host_chunk_kb=kb):
            assert_same(grp.apply_host(x, lev, MASKED_LEVELS, **kw), ref, exact=True)


def test_two_byte_result_on_thin_and_empty_levels(thin):
    """float16 field and result (half=True): ysz = 2 reaches the plan, the slabs and the level-range copies.  The
    expectation as tests/test_gpu_half.py builds it: the oracle on the field widened to float32, narrowed by one
    rounding, NaN the canonical quiet NaN.  A level is 80 * 648 * 2 = 103 680 B of Y and all of X 21 920 B: under 128 KiB
    the Y bound ends every chunk after one level, under 1 MiB several levels share a chunk."""
    order, n_inner = "wide, thin, empty", 2
    grp, lev = thin["grp"], ORDERS[order]
    x16 = thin["case"](order, n_inner, np.float32)[0].astype(np.float16)
    ref = oracle.apply_levels(thin["csrs"], x16.astype(np.float32), 1, lev, MASKED_LEVELS.astype(bool), thin["imask"],
                              thin["frac"], AREA_MIN, transpose=True)
    with np.errstate(over="ignore"):
        want = np.where(np.isnan(ref), np.uint16(0x7E00), ref.astype(np.float16).view(np.uint16))
    batch = N_OUTER * n_inner
    x_all, y_level = sum(USED) * batch * 2, batch * D * 2
    assert x_all <= (128 << 10) < 2 * y_level and 4 * (128 << 10) // (max(USED) * n_inner * 2) >= N_OUTER
    kw = dict(masked=True, remap_area_min=AREA_MIN, out_dtype=np.float16, half=True)
    for kb, flags in ((0, _lib.APPLY_HOST_NO_PACK), (0, 0), (1024, 0), (128, 0)):
        with _lib.tuning(host_chunk_kb=kb):
            _lib.host_stats(reset=True)
            y = grp.apply_host(x16, lev, MASKED_LEVELS, flags=flags, **kw)
            st = _lib.host_stats(reset=True)
        assert y.dtype == np.float16
        bad = np.argwhere(y.view(np.uint16) != want)
        assert bad.size == 0, f"host_chunk_kb={kb} flags={flags}: {len(bad)} cells differ, first {bad[:3].tolist()}"
        assert st["d2h_bytes"] == lev.size * y_level
        assert st["h2d_bytes"] == (lev.size * S * batch * 2 if flags else x_all)
        if kb == 128:
            assert st["chunks"] == lev.size


@pytest.mark.parametrize("transpose", [True, False])
def test_pinned_result_on_thin_and_empty_levels(thin, transpose):
    """A page-locked Y goes back by the pitched D2H copy of each chunk's level range, straight from the device."""
    order = "empty first and last, repeated"
    grp, lev = thin["grp"], ORDERS[order]
    x, ref = thin["case"](order, 1, np.float64)
    if transpose:
        ref = np.moveaxis(ref, 0, -2)
    out = pinned_empty(ref.shape, np.float64)
    levp, ml = grp._level_args(lev, MASKED_LEVELS, lev.size)
    for kb in (KB_SEVERAL, KB_Y_BOUND[1]):
        out[...] = -12345.678
        with _lib.tuning(host_chunk_kb=kb):
            _lib.call("smm_group_apply_host", grp.handle, x.ctypes.data_as(ctypes.c_void_p), 1,
                      out.ctypes.data_as(ctypes.c_void_p), 1, N_OUTER, lev.size, 1, int(transpose),
                      levp.ctypes.data_as(ctypes.c_void_p), ml.ctypes.data_as(ctypes.c_void_p), AREA_MIN,
                      _lib.APPLY_MASKED, 0)
        assert_same(np.array(out), ref, exact=True)
