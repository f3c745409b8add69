"""The CCSDS decoder on streams whose options the test chose (tests/ccsds_forced_cases.py), without a GPU: the
reference decoder of that file is anchored to libaec's bits by the fixtures, the writer to the reference decoder, and
the host decoder (smm_grib_aec_decode_host, the text of smm_grib_aec.hpp) must then give the writer's integers and count
exactly the options the plan named.  The project's encoder is decoded by the reference decoder as well, and the
malformed streams of group G end with the status the format text implies.  (The same G streams run under
AddressSanitizer + UBSan in tests/test_grib_ccsds.py's stand-alone harness.)"""
import ctypes
import os
import re

import numpy as np
import pytest

from smmregrid_amd import GRIB_AEC_DTYPE, _lib, griblite
from smmregrid_amd.griblite import CCSDS
from tests import ccsds_cases as cc
from tests import ccsds_encode_cases as ec
from tests import ccsds_forced_cases as fc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = cc.fixtures()


def host(case, histogram=None):
    """(status, values) of smm_grib_aec_decode_host on the case's stream in a buffer of its own"""
    stream = np.ascontiguousarray(case.stream, dtype=np.uint8)
    rec = cc.record(0, stream.size, case.n_values, case.nbits, case.block, case.rsi, case.flags).reshape(1)
    out = np.full(case.n_values, 0xDEADBEEF, dtype=np.uint32)
    status = ctypes.c_int(-1)
    hist = None if histogram is None else histogram.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64))
    _lib.call("smm_grib_aec_decode_host", ctypes.c_void_p(stream.ctypes.data), stream.size, CCSDS.cast(rec),
              out.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), hist, ctypes.byref(status))
    return status.value, out


def test_the_module_states_the_format_constants_as_the_library_does():
    assert fc.OPTIONS == tuple(_lib.GRIB_AEC_OPTIONS) and fc.PREPROCESS == _lib.GRIB_AEC_PREPROCESS
    assert (fc.OK, fc.EXHAUSTED, fc.INVALID) == (_lib.GRIB_AEC_OK, _lib.GRIB_AEC_EXHAUSTED, _lib.GRIB_AEC_INVALID)
    text = open(os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_aec.hip")).read()
    win = re.search(r"constexpr\s+int\s+kWinWords\s*=\s*(\d+)\s*;", text)
    refill = re.search(r"constexpr\s+uint32_t\s+kRefillAt\s*=\s*(\d+)\s*;", text)
    assert win and refill, "kWinWords / kRefillAt are no longer stated as the test reads them"
    assert (int(win.group(1)), int(refill.group(1))) == (fc.WIN_WORDS, fc.REFILL_AT)
    # the largest code (ID, selector, reference sample, 64 x 32 bits) that starts at the last bit before a reload ends
    # inside the window
    assert 32 * fc.REFILL_AT - 1 + 5 + 1 + 32 + 64 * 32 <= 32 * fc.WIN_WORDS


@pytest.mark.parametrize("fx", FIXTURES, ids=repr)
def test_the_reference_decoder_reads_libaecs_fixtures(fx):
    got = fc.ref_decode(fx.stream, fx.n_values, fx.nbits, fx.block, fx.rsi, fx.preprocess)
    assert np.array_equal(got, fx.values)


def test_the_writer_refuses_what_the_format_cannot_carry():
    z, r = np.zeros(16, np.int64), np.arange(16) % 7 + 1
    for values, nbits, rsi, pp, plan, word in (
            (r, 8, 4, 0, [("zero", 2, "count")], "not all zero"), (np.r_[z[:8], r[:8]], 8, 4, 0, [("zero", 2, "count")], "not all zero"),
            (np.r_[7, 6, z[2:]], 8, 4, 0, ["se", "se"], "above 12"), (r, 8, 4, 0, [("split", 6), "raw"], "id_len"),
            (r, 16, 4, 0, [("split", 14), "raw"], "id_len"), (np.zeros(40, np.int64), 8, 4, 0, [("zero", 5, "count")], "crosses"),
            (np.zeros(8 * 70, np.int64), 8, 128, 0, ["raw"] * 60 + [("zero", 5, "count")], "crosses"),
            (np.zeros(40, np.int64), 8, 16, 0, [("zero", 5, "ros")], "ROS runs to the end"),
            (np.r_[200, z[1:8]], 8, 4, 0, [("split", 0)], "rule 1"), (np.full(8, 3), 2, 4, 0, [("split", 2)], "rule 1"),
            (r, 8, 4, 0, ["raw"], "ends before"), (r[:8], 8, 4, 0, ["raw", "raw"], "more codes")):
        with pytest.raises(ValueError, match=word):
            fc.write_stream(values, nbits, 8, rsi, pp, plan)
    # strict=False lifts the refusal of a rule-1 breach and no other
    assert fc.write_stream(np.r_[200, z[1:8]], 8, 8, 4, 0, [("split", 0)], strict=False).size == 27
    with pytest.raises(ValueError, match="not all zero"):
        fc.write_stream(r, 8, 8, 4, 0, [("zero", 2, "count")], strict=False)


@pytest.mark.parametrize("letter", list("ABCDEF"))
def test_the_host_decoder_gives_the_forced_integers_and_counts_the_options_of_the_plan(letter):
    """A - E and the two small rows of F: ref_decode(stream) == values (the writer is right); the host decoder ends OK
    with the same integers and its histogram is the plan's, bin for bin.  The 2^18 + 70 row skips ref_decode only."""
    cases = fc.group(letter)
    assert cases
    for c in cases:
        assert c.values.dtype == np.uint32 and c.stream.dtype == np.uint8, c
        if c.name != "F_long_2p18":
            assert np.array_equal(fc.ref_decode(c.stream, c.n_values, c.nbits, c.block, c.rsi, c.preprocess), c.values), c
        hist = cc.new_histogram()
        status, got = host(c, hist)
        assert status == fc.OK, (c, status)
        assert np.array_equal(got, c.values), (c, np.flatnonzero(got != c.values)[:4])
        assert hist.tolist() == fc.plan_histogram(c.plan, c.rsi, c.preprocess), (c, hist.tolist(), c.plan)


def test_group_a_meets_every_option_in_every_role():
    """Per (width, J, preprocessor): every option as block 0 (a reference block under the preprocessor), as the plain
    block 1 and as the padded last block, which holds 1 sample in three of a triple's six rows and J - 1 in the other three
    (an option meets one of the two per triple) -- but for what the format has no block for."""
    seen = {}
    for c in fc.group("A"):
        key = (c.nbits, c.block, c.preprocess)
        left = c.n_values - 7 * c.block
        assert left in (1, c.block - 1) and c.rsi == 3 and len(c.plan) == 8
        for role, i in (("first", 0), ("plain", 1), ("last", 7)):
            e = c.plan[i]
            seen.setdefault(key, set()).add((role, e if isinstance(e, str) else e[0] + str(e[1]) if e[0] == "split" else "zero"))
    assert len(seen) == 16 * 4 * 2
    for (nbits, J, pp), got in seen.items():
        for role in ("first", "plain", "last"):
            ref = pp and role == "first"
            kmax = fc.split_kmax(nbits, J, ref)
            want = {"raw", "se", "zero", "split0"} | ({"split1"} if kmax >= 1 else set()) | {f"split{kmax}"}
            assert {o for r, o in got if r == role} >= want, (nbits, J, pp, role, got)
    # under the preprocessor every row jumps between the bounds and visits their neighbours: the branch of the map that
    # counts from the nearer bound
    for c in fc.group("A"):
        if c.preprocess and "raw" in c.plan[:7]:
            v, xmax = c.values.astype(np.int64), 2 ** c.nbits - 1
            jumps = set(zip(v[:-1].tolist(), v[1:].tolist()))
            assert (0, xmax) in jumps and (xmax, 0) in jumps, c
            assert c.nbits == 1 or ((xmax, 1) in jumps or (0, xmax - 1) in jumps), c
    # k >= nbits (every quotient 0) in a reference block wherever the ID carries it and a bit is left for every code
    wide = {(c.nbits, c.block) for c in fc.group("A") if c.preprocess and c.plan[0][0] == "split" and c.plan[0][1] >= c.nbits}
    assert wide == {(w, J) for w in fc.A_WIDTHS for J in (8, 16, 32, 64) if 2 ** fc.id_len(w) - 3 >= w and (J - 1) * (w + 1) <= J * w}
    assert {(9, 8), (12, 8), (17, 16)} <= {(c.nbits, c.block) for c in fc.group("A") if c.preprocess and c.plan[0] == ("split", c.nbits)}


def test_every_window_distance_asked_for_is_reached():
    cases = fc.group("D")
    assert len(cases) == 5 * 6 * 4
    reached = set()
    for c in cases:
        m = c.meta
        off = 4 * 7 + m["off4"]                       # any offset of that residue gives the same walk
        steps = fc.window_walk(c.stream, off, c.n_values, c.nbits, c.block, c.rsi, c.preprocess)
        assert steps[m["index"]] == m["step"], c
        st = m["step"]
        assert st.distance == m["distance"] % (32 * fc.REFILL_AT), c
        assert st.refilled == (m["index"] == 0 or st.entry >= 32 * fc.REFILL_AT), c
        if m["distance"] == 1919:
            assert st.entry == 1919 and not st.refilled
        if m["distance"] == 1920:
            assert st.entry == 1920 and st.refilled
        reached.add((m["target"], m["distance"], m["off4"]))
    assert len(reached) == 120


def test_libaec_decodes_the_forced_streams_alike():
    if cc.load_libaec() is None:
        pytest.skip("libaec is not installed here")
    for letter in "ABCDEF":
        for c in fc.group(letter):
            got = cc.aec_decode_libaec(c.stream, c.n_values, c.nbits, c.block, c.rsi, c.preprocess)
            assert np.array_equal(got, c.values), c


def test_the_reference_decoder_reads_what_the_projects_encoder_writes():
    """The encoder has only ever been round-tripped through the project's own decoder."""
    rows = [(f.name, f.values, f.nbits, f.block, f.rsi, f.flags) for f in FIXTURES]
    rows += [(c.name, c.values, c.nbits, c.block, c.rsi, c.flags) for c in ec.edge_cases()]
    for name, values, nbits, block, rsi, flags in rows:
        if len(values) == 0:
            continue
        rec = np.array((0, 0, len(values), nbits, block, rsi, flags, 0), dtype=GRIB_AEC_DTYPE)
        stream = griblite.aec_encode(values, rec)
        got = fc.ref_decode(stream, len(values), nbits, block, rsi, bool(flags & fc.PREPROCESS))
        assert np.array_equal(got, np.asarray(values, dtype=np.uint32)), name


def test_malformed_streams_end_with_the_status_the_format_implies():
    """G: a stream cut short is exhausted, a breach of a rule inside the stream is invalid; the samples of the blocks
    before the failing one stand, those from it on are zero."""
    cases = fc.group("G")
    assert [c.name for c in cases] == [
        "G_cut_in_raw", "G_cut_in_se", "G_cut_in_split_fs", "G_cut_in_split_remainders", "G_cut_in_zero_fs",
        "G_cut_in_id_k_too_large_behind", "G_cut_in_id_w32", "G_cut_in_reference", "G_fs_one_over_rule1", "G_second_extension_91",
        "G_second_extension_91_then_the_end", "G_second_extension_91_then_zeros_to_the_end", "G_zero_run_past_the_rsi",
        "G_zero_run_fs_65", "G_byte_len_one_short"]
    for c in cases:
        cut = "cut_in" in c.name or "one_short" in c.name
        assert c.meta["status"] == (fc.EXHAUSTED if cut else fc.INVALID), c
        status, got = host(c)
        assert status == c.meta["status"], (c, status)
        assert not got[c.meta["bad_from"]:].any() and c.meta["bad_from"] < c.n_values, c
        assert np.array_equal(got, c.values), c
        if not cut:
            continue
        with pytest.raises(ValueError):                # the reference decoder has no statuses, it only refuses
            fc.ref_decode(c.stream, c.n_values, c.nbits, c.block, c.rsi, c.preprocess)
