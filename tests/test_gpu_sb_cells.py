"""Every instantiation of the batch-fastest kernel that `launch_sb_any` can pick (tests/sb_cases.py: `cells`) is
launched on operators that hold every kind of tile, at every batch edge, and compared bit for bit with the CPU oracles
narrowed by the row's own rule -- the single-operator kernel and the level-group kernel, every built (X, Y, decode) row,
plain, NO_FILL and skipna, U = 8 and 4, both tile heights of a 2-byte Y, (B, D) and batch-fastest results.  Y is handed
in on a padded pitch, pre-filled with a sentinel byte (a tile the kernel never wrote would otherwise still hold the
previous, identical result of a recycled buffer); X sits on an odd pitch with invalid values in its pad.  The tile
orders other than the default, and the tails of the destination grid, have tests of their own below.

`apply_sb(y=...)` takes a Y of the result's own shape only, so the padded pitch goes through `_apply_call`, the one
call path underneath `SparseOperator.apply_sb` and `OperatorGroup.apply_sb` (it picks the plain, `_cf` or `_pk` entry
from the rules exactly as they do)."""
import functools

import numpy as np
import pytest

from smmregrid_amd import DeviceArray, OperatorGroup, SparseOperator, _lib, to_device
from smmregrid_amd.device import result_dtype
from smmregrid_amd.operator import _apply_call
from tests import sb_cases as sc
from tests.helpers import bits_equal

pytestmark = pytest.mark.gpu
N_LEV = len(sc.LEVEL_INDEX)


@functools.lru_cache(maxsize=None)
def _single(td, r, has_frac=True):
    case = sc.operator(td, r)
    op = SparseOperator(sc.N_SRC, case["n_dst"], case["src"], case["dst"], case["w"], device=0)
    op.set_epilogue(case["imask"], case["frac"] if has_frac else None)
    for got, want in zip(op.export_csr(), case["csr"]):
        assert np.array_equal(got, want)
    return op


@functools.lru_cache(maxsize=None)
def _group(td, r):
    ops = []
    for member in range(len(sc.MASKED_LEVELS)):
        case = sc.operator(td, r, member)
        op = SparseOperator(sc.N_SRC, case["n_dst"], case["src"], case["dst"], case["w"], device=0)
        op.set_epilogue(case["imask"], case["frac"])
        for got, want in zip(op.export_csr(), case["csr"]):
            assert np.array_equal(got, want)
        ops.append(op)
    return OperatorGroup(ops)


def _pad_of(raw):
    """An invalid element for the pad of X: NaN, or the fill value of a packed field."""
    if raw.dtype.kind in "iu":
        return np.iinfo(raw.dtype).min if raw.dtype.kind == "i" else np.iinfo(raw.dtype).max
    return raw.dtype.type(np.nan) if raw.dtype.kind == "f" else np.array(0x7FC0, np.uint16).view(raw.dtype)


def _x_on_device(row, fill, kind, batch):
    """The first `batch` entries of the field, batch-fastest on the odd pitch B + 1: (S, B + 1), or (L, S, B + 1)."""
    ffill = fill if row.x in ("i16", "u16") else True
    raws = [sc.field(row.x, row.dd, ffill, level)[0] for level in range(N_LEV if kind == "group" else 1)]
    x = np.empty((len(raws), sc.N_SRC, batch + 1), raws[0].dtype)
    x[:, :, batch] = _pad_of(raws[0])
    for l, raw in enumerate(raws):
        x[l, :, :batch] = raw[:batch].T
    return to_device(x if kind == "group" else x[0], layout="sb")


def _launch(cell, r, dx, batch, epilogue, transpose=True, knobs=None):
    """One launch of the cell's kernel into a sentinel-filled Y on a padded pitch.  Returns (the results (B, D) --
    (L, B, D) of a group -- as Y's own dtype, the pad)."""
    masked, area_min, has_frac = epilogue
    tune, flags, keep = sc.launch_of(cell)
    call = sc.call_of(cell.row, cell.fill)
    y_res = result_dtype(call["out_dtype"], call["cf_out"])
    fl = flags | (_lib.APPLY_MASKED if masked else 0) | (_lib.APPLY_SKIPNA if cell.skipna else 0) \
        | (_lib.APPLY_SB_Y_SB if keep else 0)
    n_dst = sc.n_dst_of(cell.td, r)
    width, ldy = (batch, batch + 3) if keep else (n_dst, n_dst + 5)
    lead = n_dst if keep else batch
    with _lib.tuning(**dict(tune, **(knobs or {}))):
        if cell.kind == "single":
            y = DeviceArray((lead, ldy), y_res[0]).fill_bytes(sc.SENTINEL)
            _apply_call("smm_apply_sb", _single(cell.td, r, has_frac).handle, dx, (batch + 1,), y,
                        (ldy, batch, area_min, fl, None), y_res, call["cf"], call["cf_out"])
            host = y.to_host()
            out = host[:, :width]
            return (out.T if keep else out), host[:, width:]
        # level l's results start ys_lev elements into Y, batch entry b's (a destination cell's, kept batch-fastest)
        # ys_b further on
        if keep:
            shape, ys_lev, ys_b = (N_LEV, n_dst, ldy), n_dst * ldy, ldy
        elif transpose:
            shape, ys_lev, ys_b = (batch, N_LEV, ldy), ldy, N_LEV * ldy
        else:
            shape, ys_lev, ys_b = (N_LEV, batch, ldy), batch * ldy, ldy
        y = DeviceArray(shape, y_res[0]).fill_bytes(sc.SENTINEL)
        lev, ml = np.array(sc.LEVEL_INDEX, np.int32), np.array(sc.MASKED_LEVELS, np.uint8)
        _apply_call("smm_group_apply_sb", _group(cell.td, r).handle, dx, (sc.N_SRC * (batch + 1), batch + 1), y,
                    (ys_lev, ys_b, batch, N_LEV, lev.ctypes.data_as(_lib._p), ml.ctypes.data_as(_lib._p), area_min,
                     fl, None), y_res, call["cf"], call["cf_out"])
        host = y.to_host()
        out = host[..., :width]
        return (out.transpose(0, 2, 1) if keep else (out.transpose(1, 0, 2) if transpose else out)), host[..., width:]


def _check(cell, r, dx, batch, epilogue, what, **kw):
    ref = sc.reference(cell.row, cell.skipna, cell.fill, cell.kind, cell.td, r, epilogue)
    want = ref[:batch] if cell.kind == "single" else ref[:, :batch]
    got, pad = _launch(cell, r, dx, batch, epilogue, **kw)
    what = f"{sc.row_id(cell.row)} {cell} r={r} B={batch} epilogue={epilogue} {what}"
    assert (np.ascontiguousarray(pad).view(np.uint8) == sc.SENTINEL).all(), f"{what}: the pad of Y was written"
    if want.dtype.kind == "f":
        try:
            bits_equal(np.ascontiguousarray(got), want)
        except AssertionError as e:
            raise AssertionError(f"{what}: {e}") from None
    else:
        got = np.ascontiguousarray(got).view(want.dtype)
        assert got.shape == want.shape, what
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{what}: {len(bad)} of {got.size} differ, first at {bad[:5].tolist()}"


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("skipna", [False, True], ids=["plain", "skipna"])
@pytest.mark.parametrize("row", sc.ROWS, ids=sc.row_id)
def test_cells_match_the_oracle(hip, row, skipna, kind):
    cells = sc.cells_of_test(row, skipna, kind)
    for batch in sc.BATCHES:
        dx = {fill: _x_on_device(row, fill, kind, batch) for fill in {c.fill for c in cells}}
        for cell in cells:
            for epilogue in sc.epilogues_of(kind):
                for transpose in ((True, False) if kind == "group" and not cell.ysb else (True,)):
                    _check(cell, sc.R_CELLS, dx[cell.fill], batch, epilogue, f"transpose={transpose}",
                           transpose=transpose)


def test_area_min_without_dst_frac_is_refused(hip):
    """Why the epilogue without dst_frac runs at remap_area_min = 0."""
    cell = sc.Cell(sc.ROWS[0], True, 16, 8, True, False, "single")
    with pytest.raises(_lib.SmmError, match="no dst_frac"):
        _launch(cell, sc.R_CELLS, _x_on_device(cell.row, True, "single", 3), 3, (True, 0.37, False))


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("size,td", sc.SIZE_TD, ids=[f"y{s}B-td{t}" for s, t in sc.SIZE_TD])
def test_tile_orders(hip, size, td, kind):
    """B = 257 on the largest grid of the height: a (strip, run) pair that remaps a part of the grid and ends on a short
    strip, destination-tile-fastest order over the whole grid, and dispatcher order -- the group kernel remaps every
    level with its own blocks_per_level."""
    grid = sc.order_grid(td)
    strip, run = sc.choose_order(*grid)
    assert 0 < sc.remapped_blocks(grid[0] * grid[1], run) < grid[0] * grid[1] and grid[0] % strip
    orders = (dict(sb_strip=strip, xcd_run=run), dict(sb_strip=-1), dict(xcd_run=-1))
    i = sc.SIZE_TD.index((size, td)) + 2 * sc.KINDS.index(kind)
    for ysb in (False, True):
        for knobs in orders:
            row, skipna, u = sc.rotated(size, i)
            i += 1
            cell = sc.Cell(row, skipna, td, u, True, ysb, kind)
            dx = _x_on_device(row, True, kind, sc.B_MAX)
            _check(cell, td, dx, sc.B_MAX, (True, 0.37, True), f"order={knobs}", knobs=knobs)


@pytest.mark.parametrize("kind", sc.KINDS)
@pytest.mark.parametrize("ysb", [False, True], ids=["bd", "ysb"])
@pytest.mark.parametrize("size,td", sc.SIZE_TD, ids=[f"y{s}B-td{t}" for s, t in sc.SIZE_TD])
def test_tails_of_the_destination_grid(hip, size, td, ysb, kind):
    """Last tiles of 1, 2, td - 1 and td rows: the one-row-ahead row pointer of a one-row tile, the single-element
    store of an odd n_dst, dst_frac read from lane td - 1."""
    i = sc.SIZE_TD.index((size, td)) + 2 * sc.KINDS.index(kind) + int(ysb)
    for r in (1, 2, td - 1, td):
        for batch in sc.TAIL_BATCHES:
            for skipna in (False, True):
                for u in sc.US:
                    row = sc.rotated(size, i)[0]
                    i += 1
                    cell = sc.Cell(row, skipna, td, u, True, ysb, kind)
                    _check(cell, r, _x_on_device(row, True, kind, batch), batch, (True, 0.37, True), "tail")
