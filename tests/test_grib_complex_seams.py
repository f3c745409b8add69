"""The rows of tests/complex_seam_cases.py without a GPU: its scalar reference against the numpy decoders on every valid
case of the three case modules; the reference against the host entries (smm_grib_cpx_decode_host / _mv) on status and
integers for every row of the families A-H, malformed ones included; each family's census -- a case list that no longer
reaches a seam fails here, not on the GPU --; and every row through the two stand-alone harnesses under AddressSanitizer +
UBSan (tests/cpp/grib_cpx_harness.cpp, tests/cpp/grib_cpx_mv_harness.cpp, `pinned`).  The last gates
tests/test_gpu_grib_complex_seams.py: no malformed stream goes to a GPU before the scalar decoder has given it the
reference's status without a sanitizer report.

The census tests print what they counted (pytest -s): which case reaches which seam."""
import ctypes
import itertools
import os
import subprocess

import numpy as np
import pytest

from smmregrid_amd import _lib
from tests import complex_cases as xc
from tests import complex_mv_cases as mv
from tests import complex_seam_cases as sc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, EXHAUSTED, INVALID = sc.OK, sc.EXHAUSTED, sc.INVALID
ALL = sc.cases()
cp = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct))               # noqa: E731
_u8p, _u32p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint32)


def test_the_status_numbers_are_the_headers():
    assert (OK, EXHAUSTED, INVALID) == (_lib.GRIB_CPX_OK, _lib.GRIB_CPX_EXHAUSTED, _lib.GRIB_CPX_INVALID)
    assert len({c.name for c in ALL}) == len(ALL) and all(c.n_values <= 70000 for c in ALL)
    assert all(c.status == c.want for c in ALL if c.want is not None)


# ------------------------------------------------------------------------------------------------ the reference
@pytest.mark.parametrize("c", xc.cases(), ids=repr)
def test_reference_agrees_with_the_plain_cases(c):
    status, X = sc.reference(c.stream, c.n_values, c.params)
    assert status == OK and X == c.X.tolist() == xc.numpy_decode(c.stream, c.n_values, c.params).tolist()


@pytest.mark.parametrize("c", mv.cases(), ids=repr)
def test_reference_agrees_with_the_cases_with_missing_values(c):
    status, X, present = sc.reference(c.stream, c.n_values, c.params, c.m)
    want_X, want_present = mv.numpy_decode(c.stream, c.n_values, c.params, c.m)
    assert status == OK and X == c.X.tolist() == want_X.tolist()
    assert present == c.present.tolist() == want_present.tolist()


@pytest.mark.parametrize("letter", list("ABCDEFGH"))
def test_reference_agrees_with_the_numpy_decoders_and_the_builders_on_the_seam_cases(letter):
    """A valid row: the reference's integers are the builder's and numpy_decode's.  A row of family F that must be
    refused: numpy_decode, which has no range check, gives the builder's integers with the one outside [0, 2^32)."""
    seen = 0
    for c in sc.family(letter):
        if c.meant_X is None:
            continue
        if c.status == OK:
            assert c.X.tolist() == c.meant_X, c
            assert c.meant_present is None or np.array_equal(c.present, c.meant_present), c
        else:
            assert letter == "F" and c.want == INVALID and not c.X.any(), c
        if c.n_values > c.order:                          # numpy_decode cannot take the others
            if c.m:
                X, present = mv.numpy_decode(c.stream, c.n_values, c.params, c.m)
                assert X.tolist() == c.meant_X and np.array_equal(present, c.meant_present), c
            else:
                assert xc.numpy_decode(c.stream, c.n_values, c.params).tolist() == c.meant_X, c
        seen += 1
    assert seen or letter == "H"
    if letter == "H":                                     # the rows of H that are ok
        for c in sc.family("H"):
            if c.status == OK and c.m == 0:
                assert xc.numpy_decode(c.stream, c.n_values, c.params).tolist() == c.X.tolist(), c


# ------------------------------------------------------------------------------------------------ the host entries
def host_decode(c, byte_off=5):
    """(return code, status, integers, flags, count) of the host entry for the row, its stream at an odd offset."""
    buf = np.full(c.stream.size + byte_off + 6, 0xA5, dtype=np.uint8)
    buf[byte_off:byte_off + c.stream.size] = c.stream
    rec = c.record(byte_off).reshape(1)
    values, flags = np.full(max(c.n_values, 1), 7, np.uint32), np.full(max(c.n_values, 1), 7, np.uint8)
    status, count, m = ctypes.c_int(-1), ctypes.c_uint64(99), ctypes.c_uint8(c.m)
    lib = _lib.load()
    if c.m:
        rc = lib.smm_grib_cpx_decode_host_mv(buf.ctypes.data_as(ctypes.c_void_p), buf.size, cp(rec), ctypes.byref(m),
                                             values.ctypes.data_as(_u32p), flags.ctypes.data_as(_u8p), ctypes.byref(count),
                                             ctypes.byref(status))
    else:
        rc = lib.smm_grib_cpx_decode_host(buf.ctypes.data_as(ctypes.c_void_p), buf.size, cp(rec), values.ctypes.data_as(_u32p),
                                          ctypes.byref(status))
    return rc, status.value, values[:c.n_values], flags[:c.n_values], count.value


@pytest.mark.parametrize("letter", list("ABCDEFGH"))
def test_host_entries_give_the_references_status_and_integers(letter):
    for c in sc.family(letter):
        rc, status, values, flags, count = host_decode(c)
        if c.refused:                                     # n_values <= order: the entry's own refusal, the harness decodes them
            assert rc == _lib.SMM_ERR_INVALID and b"n_values must exceed the order" in _lib.load().smm_last_error(), c
            continue
        assert rc == 0 and status == c.status, (c, rc, status, c.status)
        if c.m:
            assert count == c.P and np.array_equal(values[:c.P], c.X) and not values[c.P:].any(), c
            assert np.array_equal(flags.astype(bool), c.present), c
        else:
            assert np.array_equal(values, c.X if c.status == OK else np.zeros(c.n_values, np.int64)), c


# ------------------------------------------------------------------------------------------------ the censuses
def tiles_of(n, tile):
    return -(-n // tile)


def test_census_a_group_tiles():
    cs = sc.family("A")
    assert [c.params["n_groups"] for c in cs] == sc.A_GROUPS == [255, 256, 257, 511, 512, 513, 16383, 16384, 16385, 16641]
    assert [tiles_of(ng, sc.GROUP_TILE) for ng in sc.A_GROUPS] == [1, 1, 2, 2, 2, 3, 64, 64, 65, 66]
    assert {c.order for c in cs} == {0, 1}
    for c in cs:
        t = c.tables()
        assert t["status"] == OK and set(t["ls"]) == {1, 2, 3}, c
        assert all(a != b for a, b in zip(t["ws"], t["ws"][1:])) and len(set(t["ws"])) >= 8, c
        print(f"A {c.name}: {len(t['ls'])} groups in {tiles_of(len(t['ls']), 256)} tiles, {c.n_values} values, widths {min(t['ws'])}..{max(t['ws'])}")


def test_census_b_value_tiles():
    cs = {c.name: c for c in sc.family("B")}
    assert sorted(cs) == sorted(f"B_n{n}_order{o}" for n in sc.B_SIZES for o in (0, 1, 2) if n > o)
    assert sc.B_SIZES == [1, 2, 3, 255, 256, 257, 1023, 1024, 1025, 2047, 2049, 65535, 65536, 65537, 66561]
    assert [tiles_of(n, sc.VALUE_TILE) for n in sc.B_SIZES[6:]] == [1, 1, 2, 2, 3, 64, 64, 65, 66]
    edges = 0
    for c in cs.values():
        X = c.X
        assert c.status == OK and X.size == c.n_values == int(c.name.split("_")[1][1:])
        d1 = np.diff(X, prepend=X[0])
        d2 = np.diff(d1, prepend=d1[0])
        for e in range(sc.BLOCK, c.n_values, sc.BLOCK):          # every block and tile edge
            assert d1[e] != 0 and d2[e] != 0 and (e + 1 == c.n_values or d2[e + 1] != 0), (c, e)
            edges += 1
        if c.n_values > 2 * sc.B_TURN:
            assert (d1[sc.B_TURN:] < 0).all() and (d1[1:sc.B_TURN] > 0).all(), c
    long_rows = [c for c in cs.values() if c.n_values > 2 * sc.B_TURN and c.order > 0]
    assert {(c.n_values, c.order) for c in long_rows} == set(itertools.product(sc.B_SIZES[-4:], (1, 2)))
    assert sc.B_TURN // sc.VALUE_TILE < sc.STEP - 30 and all((c.n_values - 1) // sc.VALUE_TILE >= sc.STEP - 1 for c in long_rows)
    assert (cs["B_n65537_order2"].n_values - 1) // sc.VALUE_TILE == 64 and (cs["B_n66561_order2"].n_values - 1) // sc.VALUE_TILE == 65
    print(f"B {len(cs)} rows, {edges} block and tile edges with non-zero first and second differences; first differences "
          f"negative from tile {sc.B_TURN // sc.VALUE_TILE + 1} to the row's last (63, 64 or 65) in {sorted(c.name for c in long_rows)}")


def test_census_c_empty_groups():
    cs = sc.family("C")
    assert {(c.name.rsplit("_order", 1)[0][2:], c.order, c.m) for c in cs} == set(itertools.product(sc.C_LENGTHS, (0, 2), (0, 1, 2)))
    reached = {}
    for c in cs:
        name = c.name.rsplit("_order", 1)[0][2:]
        t = c.tables()
        ls, ws, refs = t["ls"], t["ws"], t["refs"]
        assert t["status"] == OK and ls == sc.C_LENGTHS[name] and c.status == OK, c
        if c.m:
            assert c.present.any() and not c.present.all(), c
        empty = [g for g, v in enumerate(ls) if v == 0]
        seen = set()
        if ls[0] == 0 and ls[1] == 0:
            seen.add("the first two groups")
        if ls[-1] == 0 == c.params["length_last"]:
            seen.add("length_last == 0")
        if any(not any(ls[a:a + 256]) for a in range(0, len(ls) - 255, 256)):
            seen.add("a whole tile")
        if len(ls) > 263 and not any(ls[250:263]) and ls[249] and ls[263]:
            seen.add("groups 250..262")
        if any(ws[g] > 0 and refs[g] != 0 for g in empty):
            seen.add("a width and a reference")
        if any(ls[h] > 0 and ws[h] == 0 for g in empty for h in (g - 1, g + 1) if 0 <= h < len(ls)):
            seen.add("beside a group of width 0")
        for what in seen:
            reached.setdefault(what, set()).add((c.order, c.m))
        want = {"first_two": "the first two groups", "last_zero": "length_last == 0", "whole_tile": "a whole tile",
                "straddle": "groups 250..262", "forced": "a width and a reference", "beside_width0": "beside a group of width 0",
                "gather": "a whole tile"}[name]
        assert want in seen, (c, seen)
        if name == "forced":
            assert all(ws[g] > 0 and refs[g] != 0 for g in empty), c
        print(f"C {c.name}: {len(empty)} empty groups of {len(ls)}: {sorted(seen)}")
    assert all(v == set(itertools.product((0, 2), (0, 1, 2))) for v in reached.values()) and len(reached) == 6
    assert sc.case("C_gather_order2_m0").n_values == xc.S


def test_census_d_every_width_at_every_phase():
    """From the call as built: the absolute bit position of every stored value in the call's buffer."""
    order = sc.family_rows("D", False)
    buf, rows, recs, missing = sc.call(order)
    pairs, offsets, ones, tops = set(), set(), set(), set()
    for i, c in enumerate(order):
        if c is None or c.family != "D":
            continue
        off = int(recs["byte_off"][i])
        assert np.array_equal(buf[off:off + c.stream.size], c.stream)
        offsets.add(off % 4)
        t = c.tables()
        pos = 8 * off + t["data_bit"]
        for ref, w, length in zip(t["refs"], t["ws"], t["ls"]):
            for _ in range(length):
                stored = sc._peek(t["bytes"], pos - 8 * off, w)
                pairs.add((w, pos % 32))
                if stored == (1 << w) - 1:
                    ones.add(w)
                if stored == 1 << (w - 1):
                    tops.add(w)
                pos += w
    assert offsets == {0, 1, 2, 3}
    assert pairs == set(itertools.product(range(1, 33), range(32))) and len(pairs) == 1024
    assert ones == tops == set(range(1, 33))
    crossing = sum(1 for w, ph in pairs if ph + w > 32)
    print(f"D {len(pairs)} (width, phase) pairs in 4 rows at byte offsets 0..3 mod 4; {crossing} of them cross into the next word")


def test_census_e_descriptors():
    cs = sc.family("E")
    seen = set()
    for c in cs:
        if c.m or c.refused:
            continue
        n_oct, order = c.params["n_oct"], c.order
        sign, top = 1 << (8 * n_oct - 1), (1 << (8 * n_oct - 1)) - 1
        raw = [sc._peek(c.stream.tobytes(), 8 * n_oct * k, 8 * n_oct) for k in range(order + 1)]
        g = raw[order]
        kind = "minus_zero" if g == sign else "zero" if g == 0 else "plus_top" if g == top else "minus_top" if g == sign | top else \
            "neg" if g & sign else "pos"
        seen.add((n_oct, order, "g_" + kind))
        if raw[0] == sign:
            seen.add((n_oct, order, "h1_minus_zero"))
            assert c.X[0] == 0
        assert c.status == OK and c.n_values > order, c
    kinds = ("g_neg", "g_zero", "g_minus_zero", "g_plus_top", "g_minus_top", "h1_minus_zero")
    assert seen == set(itertools.product((1, 2, 3, 4), (1, 2), kinds))
    short = [c for c in cs if c.refused]
    assert all(0 < c.n_values <= c.order for c in short) and all(c.n_values > c.order for c in cs if not c.refused)
    assert {(c.n_values, c.order) for c in short if c.m == 0} == {(1, 1), (1, 2), (2, 2)}
    for m in (1, 2):
        assert {(c.n_values, c.order, c.P) for c in short if c.m == m} == {(n, o, P) for n, o in ((1, 1), (1, 2), (2, 2)) for P in range(n + 1)}
        assert {(c.order, c.P - c.order) for c in cs if c.m == m and not c.refused} == set(itertools.product((1, 2), (-1, 0, 1)))
    assert all(c.status == OK for c in cs)
    print(f"E {len(seen)} (n_oct, order, descriptor) kinds; {len(short)} rows of n_values <= order (harness only); "
          f"P - order in -1..1 under m = 1, 2: {sorted(c.name for c in cs if c.m and not c.refused)}")


def test_census_f_range():
    cs = sc.family("F")
    seen = set()
    for c in cs:
        place, kind = next(p for p in sc.F_PLACES if c.name.startswith("F_" + p)), c.name.split("_")[-2]
        X, k = np.array(c.meant_X, dtype=np.int64), c.notes["at"]
        value, want = sc.F_KINDS[kind]
        outside = (X < 0) | (X >= sc.TWO32)
        assert c.want == want == c.status and X[k] == value and (X == value).sum() == 1, c
        assert outside.sum() == (want != OK) and (want == OK or outside[k]), c
        assert c.n_values == sc.F_PLACES[place][0] and k == sc.F_PLACES[place][1]
        if c.order == 0:
            t = c.tables()
            g = int(np.searchsorted(np.cumsum(t["ls"]), k, side="right"))
            assert c.params["nbits"] == 32 and t["ls"][g] == 2 and t["refs"][g] == value - 1 and t["ws"][g] >= 1, c
        seen.add((place, kind, c.order))
    assert {s[:2] for s in seen} | {(p, "under") for p in sc.F_PLACES} == set(itertools.product(sc.F_PLACES, sc.F_KINDS))
    assert {(p, k) for p, k, o in seen if o == 0} == set(itertools.product(sc.F_PLACES, ("top", "over")))
    for place in ("tile_last", "tile_first", "row_last"):
        assert {(k, o) for p, k, o in seen if p == place and o} == set(itertools.product(sc.F_KINDS, (1, 2)))
    assert {(k, o) for p, k, o in seen if p == "tile65" and o} == {("top", 2), ("over", 1), ("under", 2)}
    n, k = sc.F_PLACES["row_last"]
    assert k == n - 1 and n % 64 and n % 256 and sc.F_PLACES["tile_last"][1] % 1024 == 1023 and sc.F_PLACES["tile_first"][1] % 1024 == 0
    assert sc.F_PLACES["tile65"][1] // 1024 == 65
    print(f"F {len(cs)} rows: " + ", ".join(f"{c.name} -> {sc.STATUS_NAMES[c.status]}" for c in cs))


def test_census_g_missing_values_at_the_block_seams():
    cs = {c.name.rsplit("_order", 1)[0][2:]: c for c in sc.family("G")}
    assert all(c.status == OK and c.m in (1, 2) for c in cs.values())
    assert {c.m for c in cs.values()} == {1, 2} and {c.order for c in cs.values()} == {0, 1, 2}
    assert [cs[f"n{n}"].n_values for n in sc.G_SIZES] == sc.G_SIZES == [1, 31, 32, 33, 255, 256, 257, 16383, 16384, 16385]
    assert all(0 < cs[f"n{n}"].P < n for n in sc.G_SIZES if n > 1)
    b = cs["block_missing_beside_block_present"].present
    assert not b[256:512].any() and b[:256].all() and b[512:768].all()
    assert cs["P256"].P == 256 and cs["P1024"].P == 1024 and cs["P1024"].order == 1 and cs["P0"].P == 0 and cs["P0"].n_values == 300
    for first in (255, 256, 257):
        assert int(np.argmax(cs[f"first_present_{first}"].present)) == first
    for at in (31, 32, 63, 64):
        assert np.flatnonzero(~cs[f"missing_at_{at}"].present).tolist() == [at]
    assert np.flatnonzero(~cs["missing_at_31_32_63_64"].present).tolist() == [31, 32, 63, 64]
    assert cs["gather"].n_values == xc.S and not cs["gather"].present[256:512].any() and cs["gather"].present[512:768].all()
    tails = sorted(c.name for c in cs.values() if c.n_values % 32)
    assert any(c.n_values % 8 for c in cs.values()) and len(tails) >= 8
    assert all(c.bitmap_slot.size == (c.n_values + 31) // 32 * 4 for c in cs.values())
    print(f"G {len(cs)} rows; a last bitmap word with zero tail bits in {tails}")


def test_census_h_every_line_at_every_placement():
    cs = {c.name[2:]: c for c in sc.family("H")}
    assert sum(c.status != OK for c in cs.values()) <= 150
    assert list(sc.H_PLACES.values()) == [0, 255, 256, 64 * 256 + 5, sc.H_GROUPS - 1] and sc.H_PLACES["tile64"] // 256 == 64
    base = cs["intact"]
    n, ng = base.n_values, sc.H_GROUPS
    room = lambda c, t: 8 * c.stream.size - t["data_bit"]                                     # noqa: E731
    bits = lambda t: sum(w * v for w, v in zip(t["ws"], t["ls"]))                             # noqa: E731
    tile_sums = lambda t: [sum(t["ls"][a:a + 256]) for a in range(0, len(t["ls"]), 256)]      # noqa: E731
    assert base.status == OK and base.params["n_groups"] == ng == len(base.tables()["ls"]) and tiles_of(ng, 256) == 66
    good = base.tables()
    for place, g in sc.H_PLACES.items():
        t = cs[f"width33_{place}"].tables()                      # line 3: a width above 32, there and nowhere else
        assert [k for k, w in enumerate(t["ws"]) if w > 32] == [g] and t["ws"][g] == 33 and t["ls"] == good["ls"]
        t = cs[f"length_over_n_{place}"].tables()                # line 3: a length above n_values
        assert [k for k, v in enumerate(t["ls"]) if v > n] == [g] and t["ls"][g] == n + 1 and t["ws"] == good["ws"]
        t = cs[f"bits_run_out_{place}"].tables()                 # line 4: that group's bits push the last ones out
        assert [k for k in range(ng) if t["ws"][k] != good["ws"][k]] == [g] and t["ls"] == good["ls"] and max(t["ws"]) <= 32
        assert bits(t) > room(base, t) >= bits(good)
        c = cs[f"integer_2p32_{place}"]                          # line 5: that group's second integer is 2^32
        t = c.tables()
        assert t["status"] == OK and [k for k in range(ng) if t["refs"][k] != good["refs"][k]] == [g] and t["refs"][g] == sc.TWO32 - 1
        for name, want in (("width33", INVALID), ("length_over_n", INVALID), ("bits_run_out", EXHAUSTED), ("integer_2p32", INVALID)):
            assert cs[f"{name}_{place}"].status == want == cs[f"{name}_{place}"].want
    assert cs["more_groups_than_values"].status == INVALID and cs["more_groups_than_values"].params["n_groups"] == 5 > 4    # line 1
    assert 5 + 3 + 3 <= cs["more_groups_than_values"].stream.size                                                        # ... its tables fit
    for name in ("tables_cut_by_one_byte", "tables_cut_by_one_byte_big", "tables_cut_by_one_byte_m2"):                     # line 2
        c = cs[name]
        sizes = sum((c.params["n_groups"] * c.params[k] + 7) // 8 for k in ("nbits", "width_bits", "length_bits"))
        assert c.status == EXHAUSTED and sizes == c.stream.size + 1 and c.tables().get("ls") is None
    t = cs["sum_over_n_in_one_tile"].tables()
    a, b = cs["sum_over_n_in_one_tile"].notes["groups"]
    assert a // 256 == b // 256 == 0 and max(t["ls"]) <= n < tile_sums(t)[0] and cs["sum_over_n_in_one_tile"].status == INVALID
    t = cs["sum_over_n_across_tiles"].tables()
    assert max(tile_sums(t)) <= n < sum(t["ls"]) and cs["sum_over_n_across_tiles"].status == INVALID
    t = cs["sum_one_less"].tables()
    assert sum(t["ls"]) == n - 1 and max(t["ws"]) <= 32 and cs["sum_one_less"].status == INVALID
    exact, over = cs["bits_fit_exactly"], cs["bits_pass_the_end_by_one_bit"]
    assert bits(exact.tables()) == room(exact, exact.tables()) and exact.status == OK == cs["bits_fit_exactly_m2"].status
    assert bits(over.tables()) == room(over, over.tables()) + 1 and over.status == EXHAUSTED and max(over.tables()["ws"]) <= 32
    # two faults: both are there, the earlier line gives the status
    c = cs["width33_and_bits_run_out"]
    t = c.tables()
    assert max(t["ws"]) == 33 and t["ws"].index(33) == sc.H_PLACES["tile64"] and bits(t) > room(c, t) and bits(good) > room(c, t)
    c = cs["sum_one_less_and_bits_run_out"]
    t = c.tables()
    assert sum(t["ls"]) == n - 1 and bits(t) > room(c, t) + 1000
    c = cs["more_groups_than_values_and_no_tables"]
    assert c.params["n_groups"] > c.n_values and c.stream.size == 3
    assert cs["width33_and_bits_run_out"].status == cs["sum_one_less_and_bits_run_out"].status == c.status == INVALID
    with_m = sorted(k for k, c in cs.items() if c.m)
    assert {cs[k].status for k in with_m} == {OK, EXHAUSTED, INVALID}
    for c in cs.values():
        print(f"H {c.name} (m = {c.m}): {sc.STATUS_NAMES[c.status]}")


# ------------------------------------------------------------------------------------------------ the harnesses
@pytest.fixture(scope="module")
def harnesses(tmp_path_factory):
    d = tmp_path_factory.mktemp("grib_cpx_seams")
    exes = {}
    for name in ("grib_cpx_harness", "grib_cpx_mv_harness"):
        exes[name] = str(d / (name + "_asan"))
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                               "-fno-sanitize-recover=all", "-o", exes[name], os.path.join(ROOT, "tests", "cpp", name + ".cpp")])
    return exes


def header(c, *more):
    return np.array([c.n_values] + [c.params[k] for k in xc.PARAM_NAMES] + [c.stream.size] + list(more), np.int64).tobytes()


def test_every_row_ends_with_the_references_status_under_the_sanitizers(harnesses, tmp_path):
    """Every row of A-H, the malformed ones and those of n_values <= order included, through decode_row / decode_row_mv in
    stand-alone programs under ASan + UBSan: the stream in a heap block of exactly its bytes at the offsets 0..3."""
    plain, coded = [c for c in ALL if c.m == 0], [c for c in ALL if c.m]
    paths = {k: str(tmp_path / (k + ".bin")) for k in harnesses}
    with open(paths["grib_cpx_harness"], "wb") as fh:
        fh.write(np.int64(len(plain)).tobytes())
        for c in plain:
            fh.write(header(c, c.status) + c.stream.tobytes())
            fh.write((c.X if c.status == OK else np.zeros(c.n_values, np.int64)).astype(np.uint32).tobytes())
    with open(paths["grib_cpx_mv_harness"], "wb") as fh:
        fh.write(np.int64(len(coded)).tobytes())
        for c in coded:
            fh.write(header(c, c.m, c.P, c.status) + c.stream.tobytes() + c.X.astype(np.uint32).tobytes())
            fh.write(c.present.astype(np.uint8).tobytes())
    for name, cs in (("grib_cpx_harness", plain), ("grib_cpx_mv_harness", coded)):
        out = subprocess.run([harnesses[name], paths[name], "pinned"], capture_output=True, text=True, timeout=600,
                             env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
        assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
        line = out.stdout.split()
        counts = [sum(c.status == s for c in cs) for s in (OK, EXHAUSTED, INVALID)]
        assert line[0] == "pinned" and [int(line[k]) for k in (1, 3, 5, 7)] == [len(cs)] + counts, out.stdout
        assert min(counts) > 0
        print(name, out.stdout.strip())
