"""The complex-packing decode kernels (smm_grib_cpx_unpack / smm_grib_cpx_unpack_mv: `grib_unpack_cpx`,
`grib_unpack_cpx_mv`, `apply_grib(cpx=, cpx_missing=)`) on the rows of tests/complex_seam_cases.py: the seams of their
tiles of 256 groups and 1024 values, of the blocks of 256 positions and of the carries' steps of 64; groups of no
values; every width at every bit phase; the descriptors' edges; integers at the ends of [0, 2^32); and malformed rows,
which must end with the status the header of smm_grib_cpx.hpp gives them.  What is expected is the scalar reference of
complex_seam_cases.py, written from that header: statuses and bytes are compared exactly.  Every stream here has gone
through the host decoder under ASan + UBSan in tests/test_grib_complex_seams.py."""
import numpy as np
import pytest

from smmregrid_amd import GRIB_NO_BITMAP, _lib, grib_unpack_cpx, grib_unpack_cpx_mv, to_device
from tests import complex_mv_cases as mv
from tests import complex_seam_cases as sc
from tests.test_gpu_grib_complex import check_unpacked as check_unpacked_plain
from tests.test_gpu_grib_complex import device_bytes, operator, same_bits
from tests.test_gpu_grib_complex_mv import SENTINEL
from tests.test_gpu_grib_complex_mv import check_unpacked as check_unpacked_mv

pytestmark = pytest.mark.gpu
OK, EXHAUSTED, INVALID = sc.OK, sc.EXHAUSTED, sc.INVALID


def layout_bytes(order, with_bitmaps):
    return sum(4 * c.n_values + (c.bitmap_slot.size if with_bitmaps and c.m else 0) for c in order if c is not None)


def unpack(order, with_bitmaps, x=None, built=None):
    """The rows as one call into a buffer of sentinels: (host bytes of out, rows, rows_out, bitmaps_out or None, the
    layout's end)."""
    buf, rows, recs, missing = built or sc.call(order)
    total = layout_bytes(order, with_bitmaps)
    filled = to_device(np.full(total + 64, SENTINEL, dtype=np.uint8))
    x = device_bytes(buf) if x is None else x
    if with_bitmaps:
        out, rows_out, bms = grib_unpack_cpx_mv(x, rows, recs, missing, x_bytes=buf.size, out=filled)
    else:
        assert not missing.any()
        (out, rows_out), bms = grib_unpack_cpx(x, rows, recs, x_bytes=buf.size, out=filled), None
    return out.to_host(), rows, rows_out, bms, total


def check_rows(host, rows, rows_out, bms, order, total):
    """Every row of a call, whatever its kind, against the reference: the slot begins with the simple-packed twin of the
    row's integers at their own width, zero-padded to 4 bytes; a row with missing value management has the row's bitmap
    behind its slot, zero tail bits included; every other byte of out keeps the sentinel."""
    end = 0
    for i, c in enumerate(order):
        r = rows_out[i]
        if c is None:
            assert r.tobytes() == rows[i].tobytes()
            assert bms is None or int(bms["bitmap_off"][i]) == GRIB_NO_BITMAP
            continue
        assert (r["ref"], r["bscale"], r["ddiv"]) == (rows[i]["ref"], rows[i]["bscale"], rows[i]["ddiv"]), c
        assert int(r["nbits"]) == c.width, (c, int(r["nbits"]), c.width)
        off, packed = int(r["byte_off"]), c.packed
        assert off == end and off % 4 == 0 and packed.size <= 4 * c.n_values, (c, off, end)
        assert np.array_equal(host[off:off + packed.size], packed), c
        end = off + 4 * c.n_values
        assert (host[off + packed.size:end] == SENTINEL).all(), c            # the rest of the slot is not touched
        if bms is None:
            continue
        if c.m:
            slot = c.bitmap_slot
            assert int(bms["bitmap_off"][i]) == end and int(bms["n_values"][i]) == c.P, (c, bms[i], end)
            assert np.array_equal(host[end:end + slot.size], slot), c
            end += slot.size
        else:
            assert int(bms["bitmap_off"][i]) == GRIB_NO_BITMAP and int(bms["n_values"][i]) == c.n_values, c
    assert end == total and (host[total:] == SENTINEL).all() and host.size == total + 64
    return end


# ------------------------------------------------------------------------------------------------ valid rows
@pytest.mark.parametrize("letter", list("ABCDEFG"))
def test_a_familys_valid_rows_decode_to_the_references_bytes_in_one_call(hip, letter):
    """Per family one call of its rows without missing value management (smm_grib_cpx_unpack) and one of its rows with
    it (smm_grib_cpx_unpack_mv), a row marked simple-packed and a row of no values among them."""
    calls = 0
    for with_bitmaps in (False, True):
        order = sc.family_rows(letter, with_bitmaps)
        if len(order) == 2:
            continue                                         # the family has no such rows
        host, rows, rows_out, bms, total = unpack(order, with_bitmaps)
        check_rows(host, rows, rows_out, bms, order, total)
        if with_bitmaps:
            k = order.index(None)                            # (that checker knows no simple-packed row: the rows ahead of it)
            check_unpacked_mv(host, rows[:k], rows_out[:k], bms[:k], order[:k])
        else:
            assert check_unpacked_plain(host, rows, rows_out, order) == total
        calls += 1
    assert calls == {"C": 2, "E": 2}.get(letter, 1)


MIXED = ["A_ng255_order0", "B_n66561_order2", "A_ng16641_order1", "G_n16385_order0_m2", "B_n1024_order1", "C_whole_tile_order2_m1",
         None, "C_straddle_order0_m2", "F_tile65_top_order2", "G_n256_order2_m2", "B_n65537_order1", "G_P1024_order1_m2"]


def test_rows_of_one_tile_and_of_66_in_one_call_whole_and_in_cut_launches(hip):
    """Rows of 1 and of 66 tiles of groups and of values, orders 0 / 1 / 2, missing value management 0 / 1 / 2 and a row
    marked simple-packed in one call; then every kernel's grid cut into launches of at most 1, 2, 61 and 64 workgroups:
    the same records and the same bytes every time."""
    order = [None if n is None else sc.case(n) for n in MIXED] + [sc.empty_row()]
    assert {c.m for c in order if c} == {0, 1, 2} and {c.order for c in order if c} == {0, 1, 2}
    assert {1, 66} <= {-(-c.n_values // sc.VALUE_TILE) for c in order if c} and {1, 66} <= {-(-c.params["n_groups"] // 256) for c in order if c}
    built = sc.call(order)
    x = device_bytes(built[0])
    host, rows, rows_out, bms, total = unpack(order, True, x, built)
    check_rows(host, rows, rows_out, bms, order, total)
    try:
        for limit in (1, 2, 61, 64):
            _lib.call("smm_debug_set_grid_limit", limit)
            cut, _, rows_cut, bms_cut, _ = unpack(order, True, x, built)
            assert rows_cut.tobytes() == rows_out.tobytes() and bms_cut.tobytes() == bms.tobytes(), limit
            assert np.array_equal(cut, host), limit
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)


# ------------------------------------------------------------------------------------------------ refusals
def refusal(order):
    """(index of the row named, the status its words stand for) of a call that is refused; None: it was not.  Any other
    error than SMM_ERR_INVALID ends the test where it is."""
    try:
        unpack(order, any(c.m for c in order))
    except _lib.SmmError as err:
        if err.code != _lib.SMM_ERR_INVALID:
            raise
        text = str(err)
        assert ("ends before" in text) != ("is invalid" in text), text
        named = [i for i in range(len(order)) if f"recs[{i}]:" in text]
        assert len(named) == 1, text
        return named[0], EXHAUSTED if "ends before" in text else INVALID
    return None


@pytest.mark.parametrize("letter", ["H", "F"])
def test_a_malformed_row_is_refused_with_the_references_status(hip, letter):
    """One call per row.  A row that the reference refuses: SMM_ERR_INVALID naming recs[0], in the words of the
    reference's status -- "ends before" for exhausted, "is invalid" for invalid.  A row of H that it takes -- the intact
    one, the one whose bits fit exactly -- decodes to its integers."""
    wrong, refused = [], 0
    for c in sc.family(letter):
        if c.status == OK:
            if letter == "H":
                host, rows, rows_out, bms, total = unpack([c], bool(c.m))
                check_rows(host, rows, rows_out, bms, [c], total)
            continue
        got = refusal([c])
        if got != (0, c.status):                             # (every wrong refusal is reported, not only the first)
            wrong.append((c.name, sc.STATUS_NAMES[c.status], got))
        refused += 1
    assert not wrong, wrong
    assert refused == sum(c.status != OK for c in sc.family(letter)) > 15 and refused <= 150


def test_the_first_bad_row_of_a_call_is_named_and_the_good_rows_alone_decode(hip):
    good = [sc.case("A_ng257_order0"), sc.case("B_n1025_order2"), sc.case("G_n33_order0_m2"), sc.case("C_first_two_order2_m1")]
    invalid, exhausted = sc.case("H_width33_g256"), sc.case("H_bits_run_out_g0")
    assert refusal(good[:2] + [invalid] + good[2:]) == (2, INVALID)
    assert refusal(good[:1] + [exhausted] + good[1:3] + [invalid] + good[3:]) == (1, EXHAUSTED)
    assert refusal(good[:1] + [invalid, exhausted] + good[1:]) == (1, INVALID)
    host, rows, rows_out, bms, total = unpack(good, True)
    check_rows(host, rows, rows_out, bms, good, total)


# ------------------------------------------------------------------------------------------------ the gather behind it
def test_apply_grib_on_empty_groups_and_block_seams_has_the_bits_of_the_simple_packed_twin(hip):
    """2048 values in 774 groups, 271 of them empty (a run across the first tile seam, the whole of tile 2, the last
    one), and 2048 positions with a block of 256 missing beside one that is all present: the gather on the unpacked rows
    gives the bits it gives on the twin -- the reference's integers simple-packed at their own width, plus the bitmap."""
    op = operator()
    cs = [sc.case("C_gather_order2_m0"), next(c for c in sc.family("G") if c.name.startswith("G_gather")), sc.case("C_gather_order0_m1")]
    assert all(c.n_values == 2048 for c in cs) and [c.m for c in cs][:1] == [0] and cs[1].m and cs[2].m
    (buf, rows, cpx, missing), (tbuf, trows, tbms) = mv.build(cs)
    for skipna in (False, True):
        for masked, area_min in ((False, 0.0), (True, 0.5)):
            common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
            want = op.apply_grib(device_bytes(tbuf), trows, x_bytes=tbuf.size, bitmaps=tbms, **common).to_host()
            assert np.isfinite(want).any() and np.isnan(want).any()
            got = op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, cpx=cpx, cpx_missing=missing, **common).to_host()
            same_bits(got, want, f"apply_grib {common}")
