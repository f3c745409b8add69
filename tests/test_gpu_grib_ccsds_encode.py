"""Regrid results returned CCSDS-packed (smm_grib_aec_pack; `grib_aec_pack`, `apply_host_grib(grib_out=GribEncode(...,
ccsds=...))`, `Regridder(grib_out=True, grib_out_ccsds=True)`).  Every comparison is byte for byte against the host
encoder (`aec_encode`, smm_grib_aec_encode_host), whose streams tests/test_grib_ccsds_encode.py round-trips through the
decoder, or bit for bit against the simple-packed road."""
import numpy as np
import pytest

from smmregrid_amd import (GRIB_AEC_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CdoGenerate, DataArray, GribEncode, GribField,
                           Regridder, _lib, aec_encode, grib_aec_pack, grib_unpack, to_device)
from smmregrid_amd.io import open_dataset
from tests import ccsds_cases as cc
from tests import ccsds_encode_cases as ec
from tests.test_gpu_grib_ccsds import build, operator, same_bits

pytestmark = pytest.mark.gpu
_HOST = {}


def host_stream(case):
    if case.name not in _HOST:
        _HOST[case.name] = aec_encode(case.values, cc.record(0, 0, 0, case.nbits, case.block, case.rsi, case.flags))
    return _HOST[case.name]


class Constant:
    """A row of width 0: no integers, no stream."""
    name, values, nbits, block, rsi, flags, n_values = "constant", np.zeros(0, np.uint32), 0, 0, 0, 0, 77


def pack_records(cases, offsets):
    """(rows, wanted records) of the cases with their simple-packed twins at byte `offsets`."""
    rows = np.zeros(len(cases), dtype=GRIB_ROW_DTYPE)
    want = np.zeros(len(cases), dtype=GRIB_AEC_DTYPE)
    for i, (c, at) in enumerate(zip(cases, offsets)):
        rows[i] = (at, 1.5, 0.25, 10.0, c.nbits, 0)
        want[i] = (0xDEAD, 0xBEEF, c.n_values, c.nbits, c.block, c.rsi, c.flags, 0)      # byte_off / byte_len are not read
    return rows, want


def pack_call(cases, gap=3):
    """The cases as the rows of one smm_grib_aec_pack call: their simple-packed twins at odd offsets with garbage
    between them.  Returns (device bytes, x_bytes, rows, wanted records)."""
    parts, at, offsets = [], 0, []
    for i, c in enumerate(cases):
        twin = cc.pack_bits(c.values, c.nbits)
        parts += [np.full(gap + i % 2, 0xA5, np.uint8), twin]
        at += gap + i % 2
        offsets.append(at)
        at += twin.size
    rows, want = pack_records(cases, offsets)
    buf = np.concatenate(parts)
    padded = np.full((buf.size + 3) // 4 * 4, 0x5A, dtype=np.uint8)
    padded[:buf.size] = buf
    return to_device(padded), buf.size, rows, want


def check_against_host(cases, out, rows_out, recs, used):
    """Every row's stream, its length and its place are the host encoder's; the pad to 4 bytes is zero."""
    host = out.to_host()
    assert host.size == used
    end = 0
    for i, c in enumerate(cases):
        r = recs[i]
        assert int(r["byte_off"]) == end == int(rows_out["byte_off"][i]) and end % 4 == 0, (c, int(r["byte_off"]), end)
        assert (int(r["n_values"]), int(r["nbits"]), int(r["rsi"] if c.nbits else 0), int(r["reserved"])) == \
            (c.n_values, c.nbits, c.rsi, 0), c
        if c.nbits == 0:
            assert int(r["byte_len"]) == 0 and int(r["block_size"]) == 0, c
            continue
        want = host_stream(c)
        assert int(r["block_size"]) == c.block and int(r["flags"]) == c.flags
        assert int(r["byte_len"]) == want.size, (c, int(r["byte_len"]), want.size)
        slot = (want.size + 3) // 4 * 4
        padded = np.zeros(slot, np.uint8)
        padded[:want.size] = want
        got = host[end:end + slot]
        assert np.array_equal(got, padded), (c, np.flatnonzero(got != padded)[:8].tolist())
        end += slot
    assert end == used


def test_every_fixture_and_edge_case_in_one_call_equals_the_host_encoder(hip):
    """All fixtures and edge cases as the rows of one call -- every width class, block size, interval, both preprocessor
    settings, a row of width 0 among them, more than 64 rows (the row scan takes two steps) -- into a buffer full of 0xFF."""
    cases = cc.fixtures() + ec.edge_cases()
    cases.insert(5, Constant)
    assert len(cases) > 70
    x, x_bytes, rows, want = pack_call(cases)
    filled = to_device(np.full(1 << 18, 0xFF, dtype=np.uint8))
    out, rows_out, recs = grib_aec_pack(x, rows, want, x_bytes=x_bytes, out=filled)
    check_against_host(cases, out, rows_out, recs, out.nbytes)
    assert all(rows_out[k][i] == rows[k][i] for i in range(len(cases)) for k in ("ref", "bscale", "ddiv", "nbits"))
    # the same call with the launch grids cut: the rows go out in several launches, with the same bytes
    _lib.call("smm_debug_set_grid_limit", 300)
    try:
        out2, _, recs2 = grib_aec_pack(x, rows, want, x_bytes=x_bytes)
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    assert recs2.tobytes() == recs.tobytes() and np.array_equal(out2.to_host(), out.to_host())


def test_rows_of_many_segments_and_a_mixed_call(hip):
    """5000 blocks of 8: 79 segments with an interval of 128 blocks (the segment scan of a row takes two steps), 5000
    segments of one block with an interval of 1; a bitmapped row's 1500 values; widths, block sizes and preprocessor
    settings mixed, a width-0 row between them."""
    rng = np.random.default_rng(7)
    walk = np.clip(30000 + np.cumsum(rng.integers(-40, 41, 40000)), 0, 65535)
    walk[9000:15000] = walk[9000]                                    # long zero runs under the preprocessor
    sparse = np.where(rng.random(40000) < 0.002, rng.integers(0, 4096, 40000), 0)
    cases = [ec.Case("long_rsi128", walk, 16, 8, 128, 1), Constant, ec.Case("long_rsi1", walk[:40000 - 3], 16, 8, 1, 1),
             cc.fixture("short_w16_smooth"), ec.Case("long_sparse_pp0", sparse, 12, 8, 4096, 0),
             ec.Case("long_j64", walk[:20001] >> 4, 12, 64, 100, 1), cc.fixture("grid_w1_bits")]
    x, x_bytes, rows, want = pack_call(cases)
    out, rows_out, recs = grib_aec_pack(x, rows, want, x_bytes=x_bytes)
    check_against_host(cases, out, rows_out, recs, out.nbytes)


def test_many_short_rows_in_one_call(hip):
    """150 rows of 3 to 14 values, every seventh of width 0: the scan over the rows of the call (layout kernel, 64 rows at
    a step) takes three steps, and rows' offsets carry over both step boundaries."""
    rng = np.random.default_rng(11)
    cases = [Constant if i % 7 == 3 else
             ec.Case(f"short{i}", rng.integers(0, 1 << (1 + i % 16), 3 + i % 12), 1 + i % 16, (8, 16, 32, 64)[i % 4], 1 + i % 5, i % 2)
             for i in range(150)]
    x, x_bytes, rows, want = pack_call(cases)
    out, rows_out, recs = grib_aec_pack(x, rows, want, x_bytes=x_bytes)
    check_against_host(cases, out, rows_out, recs, out.nbytes)
    assert int(recs["byte_off"][64]) > 0 and int(recs["byte_off"][128]) > int(recs["byte_off"][64])


def test_round_trip_on_the_device(hip):
    """grib_unpack(grib_aec_pack(x)) is x: the integers come back at their width, byte for byte."""
    cases = [c for c in cc.fixtures() + ec.edge_cases()]
    x, x_bytes, rows, want = pack_call(cases, gap=4)
    coded, rows_c, recs = grib_aec_pack(x, rows, want, x_bytes=x_bytes)
    if coded.nbytes % 4:
        pytest.fail("the bytes used are a multiple of 4")
    back, rows_b = grib_unpack(coded, rows_c, recs)
    host = back.to_host()
    for i, c in enumerate(cases):
        twin = cc.pack_bits(c.values, c.nbits)
        off = int(rows_b["byte_off"][i])
        assert np.array_equal(host[off:off + twin.size], twin), c


# ------------------------------------------------------------------------------------------------ the whole road
ROAD = {"plain": dict(names=["grid_w12_smooth", "grid_w16_runs", "grid_w8_near_constant", "grid_w24_noise", "grid_w32_extremes",
                             "grid_w17_sparse", "grid_w1_bits", "grid_w16_rough"]),
        "bitmaps": dict(names=["grid_w12_smooth", "grid_w16_runs", "short_w16_smooth", "short_w12_rough", "short_w24_runs",
                               "grid_w32_extremes"], bitmapped={2: 2, 3: 2, 4: 4})}


def same_field(got, want, what):
    assert got.shape == want.shape and got.n_points == want.n_points, what
    assert got.rows.tobytes() == want.rows.tobytes(), (what, got.rows, want.rows)
    assert got.bitmaps.tobytes() == want.bitmaps.tobytes(), (what, got.bitmaps, want.bitmaps)
    assert got.ccsds.tobytes() == want.ccsds.tobytes(), (what, got.ccsds, want.ccsds)
    assert np.array_equal(np.asarray(got.buf), np.asarray(want.buf)), what


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("case", list(ROAD))
def test_apply_host_grib_returns_ccsds_streams(hip, case, skipna):
    """The 2048-cell grid to 333 cells, B rows of different widths: simple-packed and CCSDS input (ccsds=), one chunk and
    chunks of three rows.  The result decodes to the bits of the simple-packed grib_out result and has the bytes of the
    host encode of the float64 result."""
    op = operator()
    (buf, rows, aec, bms), (tbuf, trows, _, tbms) = build(**ROAD[case])
    widths = np.array([16, 12, 9, 24, 32, 16, 7, 12][:rows.size], dtype=np.int32)
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
        y = op.apply_host_grib(tbuf, trows, bitmaps=tbms, **common)
        simple = op.apply_host_grib(tbuf, trows, bitmaps=tbms, grib_out=GribEncode(widths, 1), **common)
        for ccsds in (True, [(8, 1, False), (16, 3, True), (64, 128, True), (32, 4096, False)] * 2):
            ccsds = ccsds if ccsds is True else ccsds[:rows.size]
            enc = GribEncode(widths, 1, ccsds=ccsds)
            want = enc.encode(y)
            assert np.array_equal(want.decode().view(np.uint32), simple.decode().view(np.uint32))
            for what, args in (("simple-packed input", dict(buf=tbuf, rows=trows, bitmaps=tbms)),
                               ("CCSDS input", dict(buf=buf, rows=rows, bitmaps=bms, ccsds=aec))):
                for chunk_rows in (0, 3):
                    got = op.apply_host_grib(grib_out=enc, chunk_rows=chunk_rows, **args, **common)
                    assert isinstance(got, GribField) and got.ccsds is not None and got.bitmaps is not None
                    same_field(got, want, f"{case} {what} chunk_rows={chunk_rows} {common}")
                    assert np.array_equal(np.asarray(got).view(np.uint32), simple.decode().view(np.uint32))
        if masked and not skipna:
            assert (want.bitmaps["bitmap_off"] != GRIB_NO_BITMAP).any()          # the masked target cells are missing
    with pytest.raises(ValueError, match="ccsds does not go with grib_out"):
        op.apply_host_grib(buf, rows, bitmaps=bms, ccsds=aec, grib_out=GribEncode(widths, 1))


# ------------------------------------------------------------------------------------------------ Regridder
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("ccsds_out")
    paths = {}
    for kind in (True, False):
        paths[kind] = str(d / f"t_{'ccsds' if kind else 'simple'}.grib2")
        with open(paths[kind], "wb") as f:
            f.write(cc.grib2_message(cc.message_fields(kind), cc.NI, cc.NJ))
    return paths


@pytest.mark.parametrize("coded_source", [True, False], ids=["ccsds_source", "simple_source"])
def test_regridder_returns_ccsds_fields_that_ship_raw_again(hip, files, caplog, monkeypatch, coded_source):
    dec = open_dataset(files[False])
    raw = open_dataset(files[coded_source], decode=False, bitmaps=True)
    src = raw["t"].data
    assert isinstance(src, GribField) and (src.ccsds is not None) == coded_source
    w = CdoGenerate(dec["t"], "r16x8").weights(method="con")
    plain = Regridder(weights=w, packed=True, grib_out=True).regrid(open_dataset(files[False], decode=False, bitmaps=True)["t"])
    assert isinstance(plain.data, GribField) and plain.data.ccsds is None
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, grib_out=True, grib_out_ccsds=True, loglevel="INFO").regrid(raw["t"])
    assert not [r.getMessage() for r in caplog.records if "decoded on the host" in r.getMessage()
                or r.getMessage().startswith("grib_out:") or r.levelname == "WARNING"]
    f = got.data
    assert isinstance(f, GribField) and f.ccsds is not None and f.bitmaps is not None and f.shape == plain.data.shape
    assert names.count("smm_grib_aec_pack") == 1 and names.count("smm_grib_pack") == 1
    assert names.count("smm_grib_aec_unpack") == (1 if coded_source else 0)
    assert "smm_grib_aec_decode_host" not in names and "smm_apply_host" not in names
    # each field is coded with its source's parameters, or the defaults
    live = f.ccsds["block_size"] != 0
    if coded_source:
        assert np.array_equal(f.ccsds["block_size"][live], src.ccsds["block_size"][live])
        assert np.array_equal(f.ccsds["rsi"][live], src.ccsds["rsi"][live])
    else:
        assert set(f.ccsds["block_size"][live].tolist()) == {32} and set(f.ccsds["rsi"][live].tolist()) == {128}
    assert got.dims == plain.dims and np.array_equal(np.asarray(got.values).view(np.uint32),
                                                     np.asarray(plain.values).view(np.uint32))
    # once more, raw: the coded result goes through the decode road of a second Regridder
    w2 = CdoGenerate(got, "r8x4").weights(method="con")
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        second = Regridder(weights=w2, packed=True, loglevel="INFO").regrid(got)
    assert names.count("smm_grib_aec_unpack") == 1 and "smm_grib_aec_decode_host" not in names
    assert not any("decoded on the host" in r.getMessage() for r in caplog.records)
    ref = Regridder(weights=w2).regrid(DataArray(np.asarray(got.values), dims=got.dims, coords=got.coords, attrs=got.attrs,
                                                 name=got.name))
    same_bits(np.asarray(second.values), np.asarray(ref.values), "second regrid, raw")
    # without the new keyword everything is as it was
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        old = Regridder(weights=w, packed=True, grib_out=True, loglevel="INFO").regrid(raw["t"])
    assert "smm_grib_aec_pack" not in names
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    if coded_source:
        assert len(lines) == 1 and "grib_out" in lines[0] and not isinstance(old.data, GribField)
    else:
        assert not lines and isinstance(old.data, GribField) and old.data.ccsds is None
        assert old.data.rows.tobytes() == plain.data.rows.tobytes() and np.array_equal(old.data.buf, plain.data.buf)
