"""tests/sb_cases.py checked on a machine without a GPU: the header's rows all map to a call, the cell list is what
`launch_sb_any` can pick and the GPU file covers it once, the restated tile order is a bijection, the operators hold
every kind of tile, and the references can tell a wrong kernel from a right one."""
import itertools

import numpy as np
import pytest

from tests import sb_cases as sc


def test_header_rows_map_to_calls():
    rows = sc.built_rows()
    assert len(rows) == 24 and len(set(rows)) == 24
    by_kind = {"float": 0, "packed-x": 0, "packed-y": 0, "half": 0}
    for row in rows:
        call = sc.call_of(row)
        assert call["x_dtype"] == sc.NP_OF[row.x]
        assert (call["cf"] is not None) == (row.x in ("i16", "u16")) == (row.dd is not None)
        assert (call["cf_out"] is not None) == (row.y in ("i16", "u16"))
        if call["cf"] is not None:
            assert call["cf"].dtype == sc.NP_OF[row.dd] and sc.call_of(row, fill=False)["cf"].fill_values == ()
        if call["cf_out"] is not None:
            assert call["cf_out"].raw_dtype == sc.NP_OF[row.y] and call["out_dtype"] == np.float64
        else:
            assert call["out_dtype"] == sc.NP_OF[row.y]
        half = {"f16", "bf16"} & {row.x, row.y}
        by_kind["half" if half else ("packed-y" if call["cf_out"] else ("packed-x" if call["cf"] else "float"))] += 1
    assert by_kind == {"float": 4, "packed-x": 4, "packed-y": 8, "half": 8}


def test_a_changed_header_is_noticed():
    with open(sc.HEADER) as f:
        text = f.read()
    lines = text.splitlines()
    at = [i for i, ln in enumerate(lines) if ln.lstrip().startswith("M(SMM_")]
    assert len(at) == 24
    fewer = lines[:at[3]] + lines[at[3] + 1:]
    assert len(sc.parse_built("\n".join(fewer))) == 23                     # the count test above would fail
    more = lines[:at[3]] + ["  M(SMM_F16, kAnyDecode, XF16, SMM_F32, float, 0)     \\"] + lines[at[3]:]
    assert len(sc.parse_built("\n".join(more))) == 25                      # a row of known types: the counts fail
    for extra in ("  M(SMM_F32, kAnyDecode, float, SMM_I8, YI8, 0)       \\",        # a type no call is known for
                  "  M(SMM_F32, kAnyDecode, float, SMM_F32, float, 1)   \\",         # a row twice
                  "  N(SMM_F32, kAnyDecode, float, SMM_F32, float, 1)   \\"):        # not a row at all
        with pytest.raises(ValueError):
            sc.parse_built("\n".join(lines[:at[3]] + [extra] + lines[at[3]:]))


def test_cells_are_what_the_launcher_can_pick():
    cells = sc.cells()
    assert len(set(cells)) == len(cells) == sc.expected_cell_count() == 24 * (10 + 2 * 14) == 912
    for c in cells:
        assert c.fill or not c.skipna                                       # NO_FILL is refused with skipna
        assert c.td in sc.TDS_OF_SIZE[sc.Y_SIZE[c.row.y]] and c.u in (4, 8) and c.kind in sc.KINDS
        knobs, flags, keep = sc.launch_of(c)
        assert knobs["sb_loads"] == c.u and keep == c.ysb and bool(flags) == (not c.fill)
        assert (knobs["sb_packed_y_rows"] == 16) == (sc.Y_SIZE[c.row.y] == 2 and c.td == 16)
    for row in sc.ROWS:
        assert {c.td for c in cells if c.row == row} == ({16} if sc.Y_SIZE[row.y] == 8 else
                                                         ({32} if sc.Y_SIZE[row.y] == 4 else {16, 64}))


def test_the_gpu_file_covers_every_cell_once():
    assert len(sc.TESTS) == 24 * 2 * 2 and len(set(sc.TESTS)) == len(sc.TESTS)
    walked = [c for t in sc.TESTS for c in sc.cells_of_test(*t)]
    assert len(walked) == len(set(walked)) and set(walked) == set(sc.cells())
    assert all(sc.cells_of_test(*t) for t in sc.TESTS)
    assert sc.launches() == sum(len(sc.BATCHES) * (3 if c.kind == "single" else (2 if c.ysb else 4)) for c in walked)


def _is_bijection(n_dtiles, n_btiles, strip, run):
    seen = {sc.tile_of(b, n_dtiles, n_btiles, strip, run) for b in range(n_dtiles * n_btiles)}
    return seen == set(itertools.product(range(n_dtiles), range(n_btiles)))


def test_tile_order_is_a_bijection():
    for td in (16, 32, 64):
        grid = sc.order_grid(td)
        strip, run = sc.choose_order(*grid)
        for knobs in ({}, dict(sb_strip=strip, xcd_run=run), dict(sb_strip=-1), dict(xcd_run=-1)):
            assert _is_bijection(*grid, *sc.order_args(**knobs)), (grid, knobs)
    for n_dtiles, n_btiles, strip, run in itertools.product(range(1, 14), range(1, 5), range(0, 6), range(0, 7)):
        assert _is_bijection(n_dtiles, n_btiles, strip, run), (n_dtiles, n_btiles, strip, run)
    # the restatement against two orders worked out by hand: 3 x 2 tiles, strips of 2, no remap; 17 blocks, runs of 1
    assert [sc.tile_of(b, 3, 2, 2, 0) for b in range(6)] == [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (2, 1)]
    assert [sc.xcd_remap_block(b, 2, 35) for b in (0, 1, 2, 8, 9, 16, 31, 32, 34)] == [0, 2, 4, 1, 3, 16, 31, 32, 34]
    assert sc.order_args() == (2, 32) and sc.order_args(-1, -1) == (0, 0) and sc.order_args(5, 4) == (5, 4)


def test_chosen_orders_take_both_branches_and_end_on_a_short_strip():
    for td in (16, 32, 64):
        n_dtiles, n_btiles = sc.order_grid(td)
        assert n_dtiles == sc.N_FULL + 1 and n_btiles == 3
        strip, run = sc.choose_order(n_dtiles, n_btiles)
        n = n_dtiles * n_btiles
        assert 0 < sc.remapped_blocks(n, run) < n            # remapped and identity blocks in one launch
        assert n_dtiles % strip != 0 and 1 < strip < n_dtiles
        assert (strip, run) != sc.order_args() and strip != 2 and run != 32
        moved = sum(sc.xcd_remap_block(b, run, n) != b for b in range(n))
        assert moved > 0


@pytest.mark.parametrize("td", [16, 32, 64])
def test_operators_hold_every_kind_of_tile(td):
    for r in (1, 2, 3, td - 1, td):
        for member in range(3 if r == sc.R_CELLS else 1):
            op = sc.operator(td, r, member)
            rowptr, col, val = op["csr"]
            assert op["n_dst"] == sc.N_FULL * td + r and rowptr.size == op["n_dst"] + 1
            per_tile = sc.tile_links(op, td)[:sc.N_FULL]
            lens = np.diff(rowptr)
            assert (per_tile == 0).any()                                                # a tile without links
            for u in (4, 8):
                for n in (1, u - 1, u, u + 1, 2 * u, 2 * u + 1):
                    assert (per_tile == n).sum() == 1, (td, r, member, n)
            assert (lens > 32).sum() == 1 and lens.max() == sc.LONG                     # one row alone beyond 4 U
            tiles = [lens[t * td:(t + 1) * td] for t in range(sc.N_FULL)]
            assert any(t.sum() and not t[:3].any() for t in tiles)                      # starts with empty rows
            assert any(t.sum() and not t[-3:].any() for t in tiles)                     # ends with them
            assert lens[sc.N_FULL * td:].sum() > 0
            assert (val < 0).any() and (val == 0.0).any()
            assert len(op["src"]) > col.size                                            # duplicate (dst, src) links
            assert all((np.diff(col[rowptr[d]:rowptr[d + 1]]) > 0).all() for d in range(op["n_dst"]))
            assert 0.03 < (op["imask"] == 0).mean() < 0.2
            assert (np.diff(op["imask"]) != 0).any()                                    # neighbours differ: a shifted mask bit shows
            assert sc.rows_without_valid_link(op)
            assert (col == sc.BIG_COL).any()


def test_fields_hold_the_special_values():
    for row in {(r.x, r.dd) for r in sc.ROWS}:
        for level in range(len(sc.LEVEL_INDEX)):
            raw, val = sc.field(*row, True, level)
            assert raw.shape == val.shape == (sc.B_MAX, sc.N_SRC) and raw.dtype == sc.NP_OF[row[0]]
            assert val.dtype == (np.float64 if "f64" in row else np.float32)
            assert 0.02 < np.isnan(val).mean() < 0.06 and np.isnan(val[0, :sc.LOW]).all()
            if row[0] in ("f32", "f64", "f16", "bf16"):
                assert 0.002 < np.isinf(val).mean() < 0.01 and (val == np.inf).any() and (val == -np.inf).any()
            if row[0] in ("f32", "f64", "bf16"):
                assert 0.99e20 < val[0, sc.BIG_COL] < 1.01e20
            if row[1]:
                assert np.isfinite(sc.field(*row, False, level)[1]).all()               # NO_FILL: no fill values


def _cases():
    for row, skipna, kind in sc.TESTS:
        done = set()
        for c in sc.cells_of_test(row, skipna, kind):
            for ep in sc.epilogues_of(kind):
                if (c.td, c.fill, ep) not in done:
                    done.add((c.td, c.fill, ep))
                    yield c, ep


def test_references_are_not_vacuous():
    """On the references alone: finite cells everywhere; NaN / fill cells, but not mostly, where the case can make
    them; and for an odd B the last entry's row differs from the row before it (a kernel that took the wrong element
    of the last pair would show)."""
    n = 0
    for c, ep in _cases():
        ref = sc.reference(c.row, c.skipna, c.fill, c.kind, c.td, sc.R_CELLS, ep)
        per_b = ref if c.kind == "single" else np.moveaxis(ref, 1, 0)                   # batch entry first
        assert per_b.shape[0] == sc.B_MAX
        # a packed field under NO_FILL takes no fill value (the library refuses the pair): its values are all finite
        # and only the epilogue can make a cell missing
        epilogue_only = not c.fill and c.row.x in ("i16", "u16")
        must_miss = ep[0] or ep[1] > 0 or c.skipna or (not c.fill and not epilogue_only)
        for b in sc.BATCHES:
            part = per_b[:b]
            assert sc.finite(part, c.row).any(), (c, ep, b)
            share = sc.missing(part, c.row).mean()
            assert share <= 0.5 and (share > 0 or not must_miss), (c, ep, b, share)
            if b % 2 and b > 1:
                assert (per_b[b - 1].view(f"u{per_b.itemsize}") != per_b[b - 2].view(f"u{per_b.itemsize}")).any()
        n += 1
    assert n == sum(len({(c.td, c.fill) for c in sc.cells_of_test(*t)}) * len(sc.epilogues_of(t[2])) for t in sc.TESTS)


def test_batches_and_tails_are_the_edges():
    assert sc.BATCHES == (1, 2, 3, 127, 128, 129, 257) and sc.TAIL_BATCHES == (1, 3, 129)
    assert sc.N_SRC % 2 == 1 and sc.R_CELLS % 2 == 1
    assert sc.LEVEL_INDEX == (2, 0, 1, 2) and sc.MASKED_LEVELS == (1, 0, 1)
    assert {(s, td) for s, tds in sc.TDS_OF_SIZE.items() for td in tds} == set(sc.SIZE_TD)
    for size, _ in sc.SIZE_TD:                       # the rotations reach every row, both U and both skipna settings
        got = [sc.rotated(size, i) for i in range(4 * len(sc.rows_of_size(size)))]
        assert {g[0] for g in got} == set(sc.rows_of_size(size)) and {g[1:] for g in got} == set(
            itertools.product((False, True), sc.US))
