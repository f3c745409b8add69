"""The chunk plan of the host GRIB calls whose rows are decoded or coded on the device (`_grib.plan_chunks`:
`apply_host_grib(ccsds=)`, `apply_host_grib(cpx=)`, `apply_host_grib(grib_out=GribEncode(..., ccsds=...))`).  No device:
the plan is numpy and the library's host-only layout entries.  The calls are the 8-row ones of
tests/test_gpu_grib_ccsds.py and tests/test_gpu_grib_complex.py, which run the plan on the GPU."""
import numpy as np
import pytest

from smmregrid_amd import GRIB_AEC_DTYPE, GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, _grib, _lib
from tests import ccsds_cases as cc
from tests import complex_cases as xc

S, D = cc.NI * cc.NJ, 333
BM_LEN = (S + 7) // 8
HUGE = 1 << 40
_CALLS = {}


def a4(v):
    return (v + 3) // 4 * 4


def call(name):
    """(kind, buf, rows, records, bitmaps, extra_cost) of a call: "ccsds-mixed", "cpx-bitmaps", ...; "simple": the
    simple-packed twin of the CCSDS "mixed" call with no coded description and a cost per row beside it -- the input of
    the CCSDS-output road."""
    if name not in _CALLS:
        if name == "simple":
            _, (buf, rows, _, bms) = cc.build(**cc.CALLS["mixed"])
            _CALLS[name] = (None, buf, rows, None, bms, 1000 * np.arange(8, dtype=np.int64) + 77)
        else:
            kind, case = name.split("-")
            mod = cc if kind == "ccsds" else xc
            (buf, rows, recs, bms), _ = mod.build(**mod.CALLS[case])
            _CALLS[name] = (_grib.CCSDS if kind == "ccsds" else _grib.CPX, buf, rows, recs, bms, 0)
    return _CALLS[name]


CALLS = ["ccsds-bitmaps", "ccsds-mixed", "cpx-bitmaps", "cpx-mixed", "simple"]


def plan(name, chunk_rows, target=HUGE):
    kind, buf, rows, recs, bms, extra = call(name)
    return list(_grib.plan_chunks(buf.size, rows, bms, coded_of(kind, rows, recs), S, D, chunk_rows, target, extra))


def coded_of(kind, rows, recs):
    return None if kind is None else _grib.CodedRows.of(rows.size, **{kind.name: recs})


def is_coded(kind, rows, recs, i):
    if kind is _grib.CCSDS:
        return int(recs["block_size"][i]) != 0 and int(rows["nbits"][i]) != 0
    return kind is _grib.CPX and int(recs["order"][i]) != _lib.GRIB_CPX_SIMPLE


def stream(kind, rows, recs, bms, i):
    """(offset, length, values) of row i's stream in the caller's buffer."""
    has_bm = bms is not None and int(bms["bitmap_off"][i]) != GRIB_NO_BITMAP
    n_val = int(bms["n_values"][i]) if has_bm else S
    if is_coded(kind, rows, recs, i):
        return int(recs["byte_off"][i]), int(recs["byte_len"][i]), n_val
    return int(rows["byte_off"][i]), (n_val * int(rows["nbits"][i]) + 7) // 8, n_val


def costs(name):
    """The bytes each row counts against the target, from the documented formula: the staged stream and bitmap, each
    rounded up to 4; for a CCSDS row its simple-packed stream rounded up to 4 and 4 B per value, for a complex-packed row
    12 B per value, 16 B per group and 256 B; 8 B per destination cell; what the caller puts beside them."""
    kind, buf, rows, recs, bms, extra = call(name)
    out = []
    for i in range(rows.size):
        _, length, n_val = stream(kind, rows, recs, bms, i)
        cost = a4(length) + D * 8 + int(np.broadcast_to(extra, rows.shape)[i])
        if is_coded(kind, rows, recs, i):
            cost += a4((n_val * int(rows["nbits"][i]) + 7) // 8) + 4 * n_val if kind is _grib.CCSDS else \
                12 * n_val + 16 * int(recs["n_groups"][i]) + 256
        if bms is not None and int(bms["bitmap_off"][i]) != GRIB_NO_BITMAP:
            cost += a4(BM_LEN)
        out.append(cost)
    return out


def bounds(chunks):
    return [(c.r0, c.r1) for c in chunks]


def covers(chunks, n):
    assert chunks[0].r0 == 0 and chunks[-1].r1 == n and all(c.r0 < c.r1 for c in chunks)
    assert all(a.r1 == b.r0 for a, b in zip(chunks, chunks[1:]))


# ------------------------------------------------------------------------------------------------ partition and budget
@pytest.mark.parametrize("name", CALLS)
def test_the_chunks_cover_the_rows_in_order(name):
    assert bounds(plan(name, 3)) == [(0, 3), (3, 6), (6, 8)]
    assert bounds(plan(name, 0)) == [(0, 8)]
    assert bounds(plan(name, 1)) == [(i, i + 1) for i in range(8)]
    assert bounds(plan(name, 3, target=1)) == [(0, 3), (3, 6), (6, 8)]        # chunk_rows fixes the rows whatever the target
    for target in (1, min(costs(name)), max(costs(name)), sum(costs(name)) // 3, sum(costs(name)) - 1, sum(costs(name))):
        covers(plan(name, 0, target), 8)


@pytest.mark.parametrize("name", CALLS)
def test_the_budget_cuts_the_chunks(name):
    cost = costs(name)
    assert all(c > D * 8 for c in cost)
    # exactly three rows fit: the fourth would pass the target by its whole cost
    assert plan(name, 0, sum(cost[:3]))[0].r1 == 3
    assert plan(name, 0, sum(cost[:3]) - 1)[0].r1 < 3 and plan(name, 0, sum(cost[:4]))[0].r1 >= 4
    assert bounds(plan(name, 0, sum(cost))) == [(0, 8)] and len(plan(name, 0, sum(cost) - 1)) == 2
    for target in (max(cost), sum(cost[:3]), sum(cost) // 2):
        chunks = plan(name, 0, target)
        assert len(chunks) > 1
        for c in chunks:
            used = sum(cost[c.r0:c.r1])
            assert used <= target or c.r1 - c.r0 == 1, (target, c.r0, c.r1, used)
            assert c.r1 == 8 or used + cost[c.r1] > target, (target, c.r0, c.r1)      # and no chunk stops early
    # a target below every row's cost: a chunk still takes one row
    assert bounds(plan(name, 0, min(cost) - 1)) == [(i, i + 1) for i in range(8)]


# ------------------------------------------------------------------------------------------------ staging
@pytest.mark.parametrize("chunk_rows", [0, 1, 3])
@pytest.mark.parametrize("name", CALLS)
def test_the_staged_pieces_hold_every_rows_bytes(name, chunk_rows):
    kind, buf, rows, recs, bms, _ = call(name)
    before = (rows.copy(), None if recs is None else recs.copy(), bms.copy())
    for c in plan(name, chunk_rows):
        assert all(a % 4 == 0 for a, _, _ in c.pieces) and c.staged_bytes % 4 == 0
        ends = [a + n for a, _, n in c.pieces]
        assert all(e <= a for e, (a, _, _) in zip(ends, c.pieces[1:])) and ends[-1] <= c.staged_bytes      # no overlap
        staged = np.full(c.staged_bytes, 0xEE, dtype=np.uint8)
        for a, off, n in c.pieces:
            staged[a:a + n] = buf[off:off + n]
        assert (c.recs is None) == (kind is None) and c.rows.size == c.bitmaps.size == c.r1 - c.r0
        want_idx = [i - c.r0 for i in range(c.r0, c.r1) if is_coded(kind, rows, recs, i)]
        assert c.coded_idx.tolist() == want_idx
        if kind is _grib.CPX:
            assert c.coded_bytes == 4 * sum(stream(kind, rows, recs, bms, c.r0 + k)[2] for k in want_idx)
        elif kind is _grib.CCSDS:
            assert c.coded_bytes == sum(a4((stream(kind, rows, recs, bms, c.r0 + k)[2] * int(rows["nbits"][c.r0 + k]) + 7) // 8)
                                        for k in want_idx)
        else:
            assert c.coded_bytes == 0
        bitmap_at = {}
        for i in range(c.r0, c.r1):
            off, length, _ = stream(kind, rows, recs, bms, i)
            coded = is_coded(kind, rows, recs, i)
            at = int((c.recs if coded else c.rows)["byte_off"][i - c.r0])
            assert at % 4 == 0 and (at, off, length) in c.pieces
            assert np.array_equal(staged[at:at + length], buf[off:off + length]), (i, at, off, length)
            if coded:                              # the row record of a coded row is the unpack step's to rewrite
                assert c.rows[i - c.r0].tobytes() == rows[i].tobytes()
            bm_off = int(bms["bitmap_off"][i])
            if bm_off == GRIB_NO_BITMAP:
                assert int(c.bitmaps["bitmap_off"][i - c.r0]) == GRIB_NO_BITMAP
                continue
            at = int(c.bitmaps["bitmap_off"][i - c.r0])
            assert bitmap_at.setdefault(bm_off, at) == at                      # every sharer points at the one copy
            assert [p for p in c.pieces if p[1] == bm_off] == [(at, bm_off, BM_LEN)]          # staged once in the chunk
            assert np.array_equal(staged[at:at + BM_LEN], buf[bm_off:bm_off + BM_LEN])
            assert int(c.bitmaps["n_values"][i - c.r0]) == int(bms["n_values"][i])
        # what is not an offset is as the caller gave it
        for got, want in ((c.rows, rows), (c.recs, recs), (c.bitmaps, bms)):
            if got is not None:
                for f in got.dtype.names:
                    if f not in ("byte_off", "bitmap_off"):
                        assert np.array_equal(got[f], want[f][c.r0:c.r1]), f
    after = (rows, recs, bms)
    assert all(a is None or a.tobytes() == b.tobytes() for a, b in zip(after, before))      # the caller's tables are not written


@pytest.mark.parametrize("name", ["ccsds-mixed", "cpx-mixed", "simple"])
def test_a_bitmap_shared_across_chunks_is_staged_in_each(name):
    """Rows 5, 6 and 7 share row 5's bitmap; with three rows a chunk, row 5 ends the second chunk and rows 6 and 7 are the
    third."""
    _, _, _, _, bms, _ = call(name)
    shared = int(bms["bitmap_off"][5])
    assert shared != GRIB_NO_BITMAP and [int(v) for v in bms["bitmap_off"][5:]] == [shared] * 3
    chunks = plan(name, 3)
    assert bounds(chunks) == [(0, 3), (3, 6), (6, 8)]
    assert [sum(p[1] == shared and p[2] == BM_LEN for p in c.pieces) for c in chunks] == [0, 1, 1]
    assert int(chunks[2].bitmaps["bitmap_off"][0]) == int(chunks[2].bitmaps["bitmap_off"][1])
    assert [sum(p[1] == shared for p in c.pieces) for c in plan(name, 0)] == [1]


# ------------------------------------------------------------------------------------------------ by hand
def hand_call():
    """40 source cells, 5 destination cells.  Row 0: a CCSDS stream of 50 bytes at 3, 40 values of 12 bits.  Row 1:
    simple-packed at 61, 40 values of 7 bits = 35 bytes.  Row 2: a CCSDS stream of 21 bytes at 101, 25 values of 9 bits
    under the bitmap (5 bytes) at 200."""
    rows = np.zeros(3, dtype=GRIB_ROW_DTYPE)
    rows["byte_off"], rows["nbits"] = (999, 61, 777), (12, 7, 9)
    recs = np.zeros(3, dtype=GRIB_AEC_DTYPE)
    recs[0] = (3, 50, 40, 12, 16, 128, _lib.GRIB_AEC_PREPROCESS, 0)
    recs[2] = (101, 21, 25, 9, 8, 1, 0, 0)
    bms = np.zeros(3, dtype=GRIB_BITMAP_DTYPE)
    bms["bitmap_off"], bms["n_values"] = (GRIB_NO_BITMAP, GRIB_NO_BITMAP, 200), (40, 40, 25)
    return rows, recs, bms


def hand_plan(chunk_rows, target, buf_size=400, rows=None, recs=None):
    r, q, bms = hand_call()
    return list(_grib.plan_chunks(buf_size, r if rows is None else rows, bms, coded_of(_grib.CCSDS, r, q if recs is None else recs),
                                  40, 5, chunk_rows, target))


def test_hand_worked_offsets():
    # one chunk: stream 0 at 0 (50 -> 52), stream 1 at 52 (35 -> 36), stream 2 at 88 (21 -> 24), its bitmap at 112 (5 -> 8)
    (c,) = hand_plan(0, HUGE)
    assert (c.r0, c.r1, c.staged_bytes) == (0, 3, 120)
    assert c.pieces == [(0, 3, 50), (52, 61, 35), (88, 101, 21), (112, 200, 5)]
    assert c.recs["byte_off"].tolist() == [0, 0, 88] and c.rows["byte_off"].tolist() == [999, 52, 777]
    assert c.bitmaps["bitmap_off"].tolist() == [GRIB_NO_BITMAP, GRIB_NO_BITMAP, 112]
    # transcoded: 40 x 12 bits = 60 bytes, 25 x 9 bits = 29 -> 32 bytes
    assert c.coded_idx.tolist() == [0, 2] and c.coded_bytes == 92
    # two rows a chunk: the second chunk starts again at 0
    a, b = hand_plan(2, HUGE)
    assert (a.r0, a.r1, a.staged_bytes, a.pieces) == (0, 2, 88, [(0, 3, 50), (52, 61, 35)])
    assert a.coded_idx.tolist() == [0] and a.coded_bytes == 60 and a.bitmaps["bitmap_off"].tolist() == [GRIB_NO_BITMAP] * 2
    assert (b.r0, b.r1, b.staged_bytes, b.pieces) == (2, 3, 32, [(0, 101, 21), (24, 200, 5)])
    assert b.recs["byte_off"].tolist() == [0] and b.rows["byte_off"].tolist() == [777]
    assert b.bitmaps["bitmap_off"].tolist() == [24] and b.coded_idx.tolist() == [0] and b.coded_bytes == 32
    # costs: row 0: 52 + (60 + 4 x 40) + 5 x 8 = 312; row 1: 36 + 40 = 76; row 2: 24 + (32 + 4 x 25) + 40 + 8 = 204
    assert bounds(hand_plan(0, 592)) == [(0, 3)]
    assert bounds(hand_plan(0, 591)) == [(0, 2), (2, 3)] and bounds(hand_plan(0, 388)) == [(0, 2), (2, 3)]
    assert bounds(hand_plan(0, 387)) == [(0, 1), (1, 3)] and bounds(hand_plan(0, 280)) == [(0, 1), (1, 3)]
    assert bounds(hand_plan(0, 279)) == [(0, 1), (1, 2), (2, 3)]


def test_the_plan_refuses_bytes_outside_the_buffer_and_a_wrong_count():
    assert len(hand_plan(0, HUGE, buf_size=205)) == 1                  # the bitmap ends with the buffer
    with pytest.raises(ValueError, match="a row's bytes leave the buffer of 204 bytes"):
        hand_plan(0, HUGE, buf_size=204)
    rows, recs, _ = hand_call()
    rows["byte_off"][1] = 400 - 34
    with pytest.raises(ValueError, match="a row's bytes leave the buffer of 400 bytes"):
        hand_plan(0, HUGE, rows=rows)
    recs["byte_len"][0] = 398                                          # from 3: one byte too many
    with pytest.raises(ValueError, match="a row's bytes leave the buffer of 400 bytes"):
        hand_plan(0, HUGE, recs=recs)
    _, recs, _ = hand_call()
    recs["n_values"][2] = 40                                           # the row holds the 25 points of its bitmap
    with pytest.raises(ValueError, match="a coded row's record has n_values different from the points its row holds"):
        hand_plan(0, HUGE, recs=recs)


# ------------------------------------------------------------------------------------------------ the coded rows of a call
def test_coded_rows_keep_records_and_missing_values_together():
    """`CodedRows`: built once from the keywords with their checks; a slice or an index array is a copy that keeps each
    row's record beside its missing value management; cost and refusal read the two together."""
    recs = np.zeros(5, dtype=GRIB_CPX_DTYPE)
    recs["byte_len"], recs["n_values"], recs["n_groups"], recs["nbits"], recs["width_ref"], recs["width_bits"] = 64, 100, 4, 8, 3, 3
    recs["length_ref"], recs["length_inc"], recs["length_last"], recs["length_bits"], recs["n_oct"] = 20, 1, 40, 4, 2
    recs["order"], recs["byte_off"] = (2, _lib.GRIB_CPX_SIMPLE, 1, _lib.GRIB_CPX_SIMPLE, 0), 100 * np.arange(5)
    missing = np.array([0, 1, 2, 0, 1], dtype=np.uint8)
    rows = np.zeros(5, dtype=GRIB_ROW_DTYPE)
    coded = _grib.CodedRows.of(5, cpx=recs, cpx_missing=missing)
    assert coded.codec is _grib.CPX and coded.is_coded(rows).tolist() == [True, False, True, False, True]
    part, pick = coded[1:4], coded[np.array([4, 0])]
    assert part.recs["byte_off"].tolist() == [100, 200, 300] and part.missing.tolist() == [1, 2, 0]
    assert pick.recs["byte_off"].tolist() == [400, 0] and pick.missing.tolist() == [1, 0] and pick.codec is _grib.CPX
    part.recs["byte_off"], part.missing[:] = 7, 9
    assert coded.recs["byte_off"].tolist() == [0, 100, 200, 300, 400] and coded.missing.tolist() == [0, 1, 2, 0, 1]
    assert _grib.CodedRows.of(5, cpx=recs)[2:].missing is None and _grib.CodedRows.of(5) is None
    # the coded rows and the bytes of their transcoded streams: 4 B per value, and a bitmap slot of align4(ceil(100 / 8))
    # bytes for a coded row with missing values inside its groups -- row 1 has the octet but no coded stream
    idx, total = coded.streams(rows)
    assert idx.tolist() == [0, 2, 4] and total == 3 * 400 + 2 * 16
    assert _grib.CodedRows.of(5, cpx=recs).streams(rows)[1] == 3 * 400 and coded[1:2].streams(rows[1:2])[1] == 0
    n_val, nbits = np.full(5, 100, dtype=np.int64), np.zeros(5, dtype=np.int64)
    plain = 12 * 100 + 16 * 4 + 256
    assert coded.device_cost(coded.is_coded(rows), n_val, nbits).tolist() == \
        [plain, 0, plain + _grib.cpx_missing_cost(100), 0, plain + _grib.cpx_missing_cost(100)]
    bms = np.zeros(5, dtype=GRIB_BITMAP_DTYPE)
    bms["bitmap_off"], bms["n_values"] = GRIB_NO_BITMAP, 100
    bms["bitmap_off"][[0, 1]] = 0                     # a coded row without missing values, a row that is not coded
    assert coded.streams(rows, bms)[0].tolist() == [0, 2, 4]
    bms["bitmap_off"][2] = 0
    with pytest.raises(ValueError, match="bitmap and missing values"):
        coded.streams(rows, bms)
    assert coded[3:].streams(rows[3:], bms[3:])[0].tolist() == [1]
    # the checks of the keywords
    aec = np.zeros(5, dtype=GRIB_AEC_DTYPE)
    for kw, text in ((dict(cpx=recs[:4]), "4 complex-packing records for 5 rows"),
                     (dict(ccsds=aec[:3]), "3 CCSDS records for 5 rows"),
                     (dict(ccsds=aec, cpx=recs), "cpx does not go with ccsds"),
                     (dict(cpx_missing=missing), "cpx_missing goes with cpx"),
                     (dict(ccsds=aec, cpx_missing=missing), "cpx_missing goes with cpx"),
                     (dict(cpx=recs, cpx_missing=missing[:4]), "4 missing-value-management values for 5 rows"),
                     (dict(coded=coded, cpx=recs), "coded stands in place of"),
                     (dict(coded=coded[:4]), "coded stands in place of")):
        with pytest.raises(ValueError, match=text):
            _grib.CodedRows.of(5, **kw)
    assert _grib.CodedRows.of(5, coded=coded) is coded
