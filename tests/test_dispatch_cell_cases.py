"""The dispatch table of the LDS tile kernel (tests/cell_cases.py) against its own cases, without a GPU: the cases
cover exactly the reachable cells, the other template axes meet every class, and every builder's operator has the
row length, the per-block footprint and the sentinel links its case declares."""
import functools

import numpy as np
import pytest

from oracle import oracle
from tests import cell_cases as cc


@functools.lru_cache(maxsize=None)
def _csr(op):
    L = cc.banded_links(*op)
    return oracle.coo_to_csr(L["n_src"], L["n_dst"], L["src"], L["dst"], L["w"])


@pytest.mark.parametrize("xt", cc.XTS)
def test_cases_cover_exactly_the_reachable_cells(xt):
    got = {c.cell for c in cc.CASES if c.xt == xt}
    assert got == cc.REACHABLE[xt], (sorted(cc.REACHABLE[xt] - got), sorted(got - cc.REACHABLE[xt]))
    assert len({c.id for c in cc.CASES}) == len(cc.CASES)


def test_reachable_counts():
    """The figures DESIGN.md quotes."""
    assert {xt: len(cc.REACHABLE[xt]) for xt in cc.XTS} == {"f64": 85, "f32": 61}
    assert cc.REACHABLE["f32"] <= cc.REACHABLE["f64"]


def test_every_cell_runs_its_batches():
    """Per cell: a walk tail (B = 2 j_per_block + 1) and a multiple of j_per_block that is no multiple of R; B = 1
    and B = R - 1 land in the cell the dispatcher steps down to, and are declared there."""
    for xt in cc.XTS:
        for cell in cc.REACHABLE[xt]:
            mine = [(dict(c.knobs)["tile_walk"], c.batch) for c in cc.CASES if c.xt == xt and c.cell == cell]
            assert any(b == 2 * w + 1 for w, b in mine), cell
            assert any(b % w == 0 and (cell.r == 1 or b % cell.r) for w, b in mine), cell
            if cell.r == 1:
                assert any(b == 1 for w, b in mine), cell
    assert max(c.batch for c in cc.CASES) <= 40
    for r in (2, 4):
        assert any(b == r - 1 for _, b in cc._WALK_BATCH[r])


def test_rotation_meets_every_class():
    """YT, NT (tile_x_loads), the epilogue and SKIPNA (where the form has a variant) meet every MAXK class, every
    NP class and both staging forms."""
    axes = {"yt": lambda c: c.yt, "nt": lambda c: dict(c.knobs)["tile_x_loads"],
            "epilogue": lambda c: (c.masked, c.area_min), "skipna": lambda c: c.skipna}
    values = {"yt": set(cc.XTS), "nt": {1, 2}, "epilogue": {(False, 0.0), (True, 0.0), (True, 0.37), (False, 0.37)},
              "skipna": {False, True}}
    classes = {"maxk": lambda c: c.cell.maxk, "np": lambda c: c.cell.np, "staging": lambda c: c.cell.staging}
    for aname, aval in axes.items():
        for cname, cval in classes.items():
            for cls in {cval(c) for c in cc.CASES}:
                seen = {aval(c) for c in cc.CASES if cval(c) == cls}
                want = values[aname]
                if aname == "skipna" and cname == "maxk" and cls == 0:
                    want = {False}                      # streamed links have no skipna variant
                assert seen == want, (aname, cname, cls, seen)
    for c in cc.CASES:
        if c.skipna:
            assert c.cell.shape == 256 or (not c.cell.split and c.cell.maxk in (32, 48)), c.id


@pytest.mark.parametrize("op", sorted({c.op for c in cc.CASES}), ids=lambda o: "-".join(str(int(v)) for v in o))
def test_builder_invariants(op):
    shape, k, chunks, steered = op
    L = cc.banded_links(*op)
    rowptr, col, val = _csr(op)
    lens = np.diff(rowptr)
    n_dst = L["n_dst"]
    assert n_dst % 64 and n_dst % 256 and n_dst <= 1500 and L["n_src"] <= 300000 and L["n_src"] % 16 == 0
    assert lens.max() == k and (lens == 0).any() and (lens == 1).any()
    assert (val == 0.0).any() and val.min() >= -0.2 and val.max() < 1.0
    d, s = L["dst"].astype(np.int64), L["src"].astype(np.int64)
    assert not np.all(np.diff(d * L["n_src"] + s) >= 0), "links are shuffled"
    # per-block chunk footprint of the declared rows: every full block stages exactly `chunks`
    foot = [np.unique(col[rowptr[b]:rowptr[min(b + shape, n_dst)]] // cc.CHUNK).size for b in range(0, n_dst, shape)]
    assert foot[:-1] == [chunks] * (len(foot) - 1) and foot[-1] <= chunks, foot
    # sentinels: a link on the first element of block 0's first staged chunk and on the last element of its last
    blk = col[:rowptr[shape]]
    first, last = L["sentinels"]
    assert first == blk.min() and first % cc.CHUNK == 0 and last == blk.max() and last % cc.CHUNK == cc.CHUNK - 1
    for c_ in (first, last):
        assert (val[:rowptr[shape]][blk == c_] != 0.0).all()
    # the planner restated picks the declared shape and footprint
    got_shape, st = cc.native_plan(rowptr, col)
    assert got_shape == shape and st["valid"] and st["max_chunks"] == chunks, (got_shape, st)


@pytest.mark.parametrize("case", cc.CASES, ids=lambda c: c.id)
def test_case_is_predicted_to_land_in_its_cell(case):
    shape, k, chunks, steered = case.op
    knobs = dict(case.knobs)
    info = cc.model_launch_info(shape, chunks, k, case.batch, case.xt, knobs)
    cell, np_needed = cc.structural_cell(k, info, knobs)
    assert cell == case.cell and np_needed == case.np_needed
    assert info["lds_bytes"] <= 65536


def test_largest_legal_tiles_are_cases():
    """np_needed == 16: a 64 KiB f64 tile on the 4-wave shape (LDS byte offset 65528 in use) and 16 KiB on one wave."""
    assert any(c.xt == "f64" and c.op[0] == 256 and c.op[2] == 2048 for c in cc.CASES)
    assert any(c.xt == "f64" and c.op[0] == 64 and c.op[2] == 512 for c in cc.CASES)
    assert any(c.xt == "f32" and c.op[0] == 256 and c.op[2] == 2048 for c in cc.CASES)
    np_seen = {(c.xt, c.cell.shape == 256, c.np_needed) for c in cc.CASES}
    for n in (1, 2, 3, 4, 5, 8, 9, 16):
        assert ("f64", True, n) in np_seen
    for n in (1, 2, 3, 4, 5, 8):
        assert ("f32", True, n) in np_seen
    k_seen = {c.op[1] for c in cc.CASES}
    assert {4, 5, 8, 9, 16, 17, 32, 33, 48, 49, 64, 65, 128, 129, 256, 257} <= k_seen
