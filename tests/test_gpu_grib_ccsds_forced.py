"""smm_grib_aec_unpack on streams whose coding options the test chose (tests/ccsds_forced_cases.py; what they pin is
said there and in tests/test_grib_ccsds_forced.py, which holds the host decoder to the same cases).  Every comparison is
byte for byte against the simple-packed twin of the integers the writer was given; the malformed streams of group G are
refused by row and by name and leave the library able to go on."""
import numpy as np
import pytest

from smmregrid_amd import GRIB_AEC_DTYPE, _lib, grib_unpack, griblite, to_device
from smmregrid_amd._lib import SmmError
from tests import ccsds_cases as cc
from tests import ccsds_forced_cases as fc
from tests.test_gpu_grib_ccsds import check_unpacked, operator, same_bits

pytestmark = pytest.mark.gpu
GAP = 0xFF        # between and behind the streams: ones, which would end an FS code that is read past its stream


def lay_out(cases, trailing=5, constant_row=True):
    """(bytes, row records, CCSDS records) of one call with `cases` as its rows: every stream behind 1 - 4 bytes of 0xFF
    chosen so that it starts (meta off4) or ends (meta end4) on the residue mod 4 the case asks for, else on changing
    ones; `trailing` bytes of 0xFF behind the last; a constant row (nbits 0) as the last record."""
    n = len(cases) + (1 if constant_row else 0)
    rows = cc.rules(n, seed=4)
    aec = np.zeros(n, dtype=GRIB_AEC_DTYPE)
    parts, at = [], 0
    for i, c in enumerate(cases):
        want = c.meta.get("off4", (c.meta["end4"] - c.stream.size) % 4 if "end4" in c.meta else (1 + i) % 4)
        gap = (want - at - 1) % 4 + 1
        parts += [np.full(gap, GAP, np.uint8), c.stream]
        at += gap
        rows["nbits"][i] = c.nbits
        aec[i] = (at, c.stream.size, c.n_values, c.nbits, c.block, c.rsi, c.flags, 0)
        at += c.stream.size
    parts.append(np.full(trailing, GAP, np.uint8))
    if constant_row:
        rows["nbits"][-1], rows["byte_off"][-1] = 0, 4321               # passes through untouched
        aec[-1] = (0, 0, 55, 0, 0, 0, 0, 0)
    return np.concatenate(parts), rows, aec


def device_bytes(buf):
    padded = np.full((buf.size + 3) // 4 * 4, GAP, dtype=np.uint8)
    padded[:buf.size] = buf
    return to_device(padded)


def slots(cases):
    return sum((c.n_values * c.nbits + 31) // 32 * 4 for c in cases)


def unpack_and_check(cases, buf, rows, aec):
    """One grib_unpack call into a buffer of 0xFF: every slot the bytes of the twin, the records passed through, nothing
    written behind the layout.  Returns the bytes."""
    filled = to_device(np.full(slots(cases) + 64, 0xFF, dtype=np.uint8))
    out, rows_out = grib_unpack(device_bytes(buf), rows, aec, x_bytes=buf.size, out=filled)
    host = out.to_host()
    for i in range(len(cases), len(rows)):
        assert rows_out[i].tobytes() == rows[i].tobytes()
    end = check_unpacked(host, rows, rows_out, cases)
    assert end == slots(cases) and (host[end:] == 0xFF).all()
    return host


CALLS = {"A_3bit_ids": lambda: [c for c in fc.group("A") if c.nbits <= 8][::-1],
         "A_4bit_ids": lambda: [c for c in fc.group("A") if 8 < c.nbits <= 16],
         "A_5bit_ids": lambda: [c for c in fc.group("A") if c.nbits > 16],
         "A_mixed": lambda: fc.group("A")[5::7],
         # B, C and E interleaved: 16 + 16 + 16 and the last of C
         "BCE": lambda: [c for trio in zip(fc.group("B") + fc.group("C")[:2], fc.group("C")[2:18], fc.group("E")) for c in trio]
         + fc.group("C")[18:],
         "D": lambda: fc.group("D"),
         "F": lambda: fc.group("F")}


def test_the_calls_hold_every_case():
    names = {c.name for call in CALLS.values() for c in call()}
    assert names == {c.name for letter in "ABCDEF" for c in fc.group(letter)} and len(names) == 768 + 14 + 19 + 120 + 16 + 3


@pytest.mark.parametrize("call", list(CALLS))
def test_grib_unpack_gives_the_forced_integers(hip, call):
    """The cases of A - F as the rows of a handful of calls: widths, J, rsi and preprocessor settings mixed, streams at
    odd offsets with 0xFF between them, a constant row behind them.  D's rows lie at the byte_off % 4 and E's end on the
    residue their cases ask for."""
    cases = CALLS[call]()
    buf, rows, aec = lay_out(cases)
    assert len({(c.nbits, c.block, c.rsi, c.preprocess) for c in cases}) > 2
    for c, rec in zip(cases, aec):
        if "off4" in c.meta:
            assert int(rec["byte_off"]) % 4 == c.meta["off4"], c
            step = fc.window_walk(c.stream, int(rec["byte_off"]), c.n_values, c.nbits, c.block, c.rsi, c.preprocess)[c.meta["index"]]
            assert step == c.meta["step"], c                              # the distance holds where the stream really lies
        if "end4" in c.meta:
            assert int(rec["byte_off"] + rec["byte_len"]) % 4 == c.meta["end4"], c
    unpack_and_check(cases, buf, rows, aec)


@pytest.mark.parametrize("x_mod4", [1, 2, 3])
def test_the_last_row_may_end_on_the_last_byte_of_x(hip, x_mod4):
    """No byte behind the last stream, and x_bytes no multiple of 4: the word that holds the last byte is the last one
    read."""
    cases = fc.group("E")
    cases = cases[x_mod4:] + cases[:x_mod4]
    buf, rows, aec = lay_out(cases, trailing=0, constant_row=False)
    while buf.size % 4 != x_mod4:                                          # a longer first gap moves every stream
        buf = np.concatenate([np.full(1, GAP, np.uint8), buf])
        aec["byte_off"] += 1
    assert int(aec["byte_off"][-1] + aec["byte_len"][-1]) == buf.size and buf.size % 4 == x_mod4
    unpack_and_check(cases, buf, rows, aec)


def test_the_long_rows_with_cut_launch_grids_give_the_same_bytes(hip):
    """The F call under smm_debug_set_grid_limit below and above the workgroups its widest row takes (256 words a
    workgroup of the store, 64 intervals a workgroup of the inverse: four for the 193 intervals of one block)."""
    cases = fc.group("F")
    buf, rows, aec = lay_out(cases)
    words = max((c.n_values * c.nbits + 31) // 32 for c in cases)
    groups = max(-(-c.n_values // (c.block * c.rsi * 64)) for c in cases)
    per_row = max(-(-words // 256), groups)
    assert groups == 4 and per_row > 4
    whole = unpack_and_check(cases, buf, rows, aec)
    for limit in (per_row - 1, 3, 2 * per_row + 1):
        _lib.call("smm_debug_set_grid_limit", limit)
        try:
            cut = unpack_and_check(cases, buf, rows, aec)
        finally:
            _lib.call("smm_debug_set_grid_limit", 0)
        assert np.array_equal(cut, whole), limit


@pytest.mark.parametrize("skipna", [False, True])
def test_apply_grib_on_forced_rows_has_the_bits_of_the_simple_packed_twin(hip, skipna):
    """Eight forced rows of 2048 values -- widths 2, 3, 5, 7, 9, 15, 25, 31 -- through the gather."""
    op = operator()
    cases = fc.gather_rows()
    buf, rows, aec = lay_out(cases, constant_row=False)
    twin_rows, parts, at = rows.copy(), [], 0
    for i, c in enumerate(cases):
        assert c.n_values == cc.NI * cc.NJ
        packed = cc.pack_bits(c.values, c.nbits)
        parts += [np.full(3, GAP, np.uint8), packed]
        twin_rows["byte_off"][i] = at + 3
        at += 3 + packed.size
        rows["byte_off"][i] = aec["byte_off"][i]
    twin = np.concatenate(parts)
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
        want = op.apply_grib(device_bytes(twin), twin_rows, x_bytes=twin.size, **common).to_host()
        assert np.isfinite(want).any()
        got = op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, ccsds=aec, **common).to_host()
        same_bits(got, want, f"apply_grib on forced rows {common}")


def test_malformed_streams_are_refused_by_row_and_the_next_call_goes_on(hip):
    """G: one malformed row a call, at a changing index among good rows, 0xFF behind every stream.  grib_unpack raises
    SMM_ERR_INVALID, names the row and says what the host decoder says of that stream; the good rows in a call of their
    own then give their bytes as before."""
    good = fc.group("E")[:6]
    for i, bad in enumerate(fc.group("G")):
        at = i % (len(good) + 1)
        cases = good[:at] + [bad] + good[at:]
        buf, rows, aec = lay_out(cases)
        text = {fc.EXHAUSTED: "ends before its values do", fc.INVALID: "is invalid"}[bad.meta["status"]]
        with pytest.raises(SmmError) as err:
            grib_unpack(device_bytes(buf), rows, aec, x_bytes=buf.size, out=to_device(np.full(slots(cases) + 64, 0xFF, dtype=np.uint8)))
        assert err.value.code == _lib.SMM_ERR_INVALID, bad
        assert f"recs[{at}]" in str(err.value) and text in str(err.value), (bad, str(err.value))
        unpack_and_check(good, *lay_out(good))


def test_a_stream_cut_at_any_byte_is_refused_as_the_host_decoder_refuses_it(hip):
    """Short forced rows (E, and A's rows of 1 - 3 bits, where most IDs the bytes behind the end can complete are ones no
    block can have) cut after every byte, 0xFF behind the cut, the cut's end on changing residues mod 4, good rows on
    both sides.  The last byte of a stream always holds a bit the row needs, so the host decoder runs out of stream at
    every cut; the call must say the same and name the row.  (Cutting a good stream never leaves a rule breach inside
    it; those are group G's.)  449 calls of three short rows: a tenth of a second on an MI355X."""
    good = fc.group("E")[4:6]
    rows_cut = fc.group("E") + [c for c in fc.group("A") if c.nbits <= 3 and c.block == 8 and c.name[-1] in "03"]
    assert len(rows_cut) == 16 + 12
    calls = 0
    for c in rows_cut:
        for keep in range(1, c.stream.size):
            cut = c._replace(stream=c.stream[:keep], meta=dict(end4=(keep + c.nbits) % 4))
            with pytest.raises(ValueError, match="ends before its values do"):
                griblite.aec_decode(cut.stream, cc.record(0, keep, c.n_values, c.nbits, c.block, c.rsi, c.flags))
            cases = [good[0], cut, good[1]]
            buf, rows, aec = lay_out(cases)
            with pytest.raises(SmmError) as err:
                grib_unpack(device_bytes(buf), rows, aec, x_bytes=buf.size, out=to_device(np.full(slots(cases) + 64, 0xFF, dtype=np.uint8)))
            assert "recs[1]" in str(err.value) and "ends before its values do" in str(err.value), (c, keep, str(err.value))
            calls += 1
    assert calls > 400
    unpack_and_check(good, *lay_out(good))
