"""Regrid results returned complex-packed (smm_grib_cpx_pack; `grib_cpx_pack`, `apply_host_grib(grib_out=GribEncode(...,
cpx=...))`, `Regridder(grib_out=True, grib_out_cpx=True)`).  Every comparison is byte for byte against the host encoder
(`cpx_encode`, smm_grib_cpx_encode_host), which tests/test_grib_complex_encode.py pins against the template encoder of
tests/complex_cases.py, or bit for bit against the simple-packed road."""
import numpy as np
import pytest

from smmregrid_amd import (GRIB_CPX_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CdoGenerate, DataArray, GribEncode, GribField,
                           Regridder, _lib, cpx_encode, grib_cpx_pack, grib_unpack_cpx, to_device)
from smmregrid_amd.griblite import GRIB_CPX_SIMPLE, cpx_want
from smmregrid_amd.io import open_dataset
from tests import complex_cases as xc
from tests.ccsds_cases import pack_bits
from tests.test_gpu_grib_complex import operator, same_bits
from tests.test_grib_complex_encode import ROWS, bound_of

pytestmark = pytest.mark.gpu


class PackCase:
    """n integers of `nbits` bits wanted at `order` in groups of L."""

    def __init__(self, name, X, order, L, nbits=None):
        self.name, self.X, self.order, self.L = name, np.asarray(X, dtype=np.int64), order, L
        self.nbits = xc.width_of(self.X) if nbits is None else nbits
        self.n_values = int(self.X.size)
        self._host = None

    def host(self):
        if self._host is None:
            self._host = cpx_encode(self.X, cpx_want(self.nbits, self.order, self.L))
        return self._host

    def __repr__(self):
        return f"{self.name}/o{self.order}/L{self.L}"


def every_case():
    """Every row of the CPU test at orders 0 / 1 / 2, the group lengths taken in turn; the overflow rows; a row of width
    0 and one of no values among them."""
    out, k = [], 0
    for name, X in ROWS:
        for order in (0, 1, 2):
            out.append(PackCase(name, X, order, (8, 16, 32, 64)[k % 4]))
            k += 1
    out += [PackCase("descriptor_overflow", np.array([2 ** 31, 2 ** 31 + 5, 2 ** 31 + 9, 2 ** 31 + 11] * 40), 2, 8),
            PackCase("z_overflow", np.array([0, 2 ** 32 - 1] * 600), 1, 16),
            PackCase("extreme29", np.array([0, 2 ** 29 - 1] * 700), 2, 32),
            PackCase("no_cascade", np.array([0, 2 ** 31 - 1] * 50), 2, 64)]
    out.insert(5, PackCase("width0", np.zeros(77), 2, 32))
    out.insert(9, PackCase("empty", np.zeros(0), 1, 8, nbits=12))
    return out


def pack_records(cases, offsets):
    """(rows, wanted records) of the cases with their simple-packed streams at byte `offsets`."""
    rows = np.zeros(len(cases), dtype=GRIB_ROW_DTYPE)
    want = np.zeros(len(cases), dtype=GRIB_CPX_DTYPE)
    for i, (c, at) in enumerate(zip(cases, offsets)):
        rows[i] = (at, 1.5, 0.25, 10.0, c.nbits, 0)
        # only n_values, nbits, order and length_ref are read
        want[i] = (0xDEAD, 0xBEEF, c.n_values, 77, c.nbits, 9, 9, c.L, 9, 9, 9, c.order, 9, 0)
    return rows, want


def pack_call(cases, gap=3):
    """The cases as the rows of one smm_grib_cpx_pack call: their simple-packed streams at odd offsets with garbage
    between them.  Returns (device bytes, x_bytes, rows, wanted records)."""
    parts, at, offsets = [], 0, []
    for i, c in enumerate(cases):
        twin = pack_bits(c.X, c.nbits)
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
    """Every row's stream, its record and its place are the host encoder's; the pad to 4 bytes is zero."""
    host = out.to_host()
    assert host.size == used
    end = 0
    for i, c in enumerate(cases):
        r = recs[i]
        want, rec = c.host()
        assert int(r["byte_off"]) == end == int(rows_out["byte_off"][i]) and end % 4 == 0, (c, int(r["byte_off"]), end)
        rec = rec.copy()
        rec["byte_off"] = end
        assert r.tobytes() == rec.tobytes(), (c, r, rec)
        if c.nbits == 0:
            assert int(r["byte_len"]) == 0 and int(r["order"]) == GRIB_CPX_SIMPLE, c
            continue
        slot = (want.size + 3) // 4 * 4
        padded = np.zeros(slot, np.uint8)
        padded[:want.size] = want
        got = host[end:end + slot]
        assert np.array_equal(got, padded), (c, np.flatnonzero(got != padded)[:8].tolist())
        end += slot
    assert end == used


def test_every_case_in_one_call_equals_the_host_encoder(hip):
    """All rows of the CPU test at every order with the group lengths in turn -- the 300 000-value row, rows of 1, 2 and 3
    values, the rows that fall back to order 0, a row of width 0 and one of no values among them, more than 64 rows (the
    scan over the rows of the call takes two steps) -- into a buffer full of 0xFF."""
    cases = every_case()
    assert len(cases) > 64
    x, x_bytes, rows, want = pack_call(cases)
    bound = sum(bound_of(c.n_values, c.nbits, c.order, c.L) for c in cases)
    filled = to_device(np.full(bound + 64, 0xFF, dtype=np.uint8))
    out, rows_out, recs = grib_cpx_pack(x, rows, want, x_bytes=x_bytes, out=filled)
    check_against_host(cases, out, rows_out, recs, out.nbytes)
    assert all(rows_out[k][i] == rows[k][i] for i in range(len(cases)) for k in ("ref", "bscale", "ddiv", "nbits"))
    fallen = {c.name for c, r in zip(cases, recs) if c.order > 0 and c.n_values > c.order and c.nbits and int(r["order"]) == 0}
    assert {"descriptor_overflow", "z_overflow", "no_cascade"} <= fallen and "extreme29" not in fallen
    # the same call with the launch grids cut: the rows go out in several launches, with the same bytes
    _lib.call("smm_debug_set_grid_limit", 300)
    try:
        out2, _, recs2 = grib_cpx_pack(x, rows, want, x_bytes=x_bytes)
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    assert recs2.tobytes() == recs.tobytes() and np.array_equal(out2.to_host(), out.to_host())


def test_long_rows(hip):
    """40 000 values at L = 8 (5000 groups, 40 tiles of 1024 values) and at L = 64; a bitmapped field's 1500 values; and
    70 001 values, 69 tiles: the scan over a row's tiles (rows kernel, 64 tiles at a step) takes two steps.  The scan over
    the groups of a tile is a workgroup scan of eight steps at any size; the scan over the rows of a call takes two steps
    in the test above."""
    rng = np.random.default_rng(7)
    walk = np.clip(30000 + np.cumsum(rng.integers(-40, 41, 70001)), 0, 65535)
    walk[9000:15000] = walk[9000]                                    # groups of width 0
    cases = [PackCase("long_L8", walk[:40000], 2, 8), PackCase("width0", np.zeros(5), 1, 8),
             PackCase("long_L64", walk[:40000 - 3], 1, 64), PackCase("short1500", xc.case("short1500_order2").X, 2, 32),
             PackCase("two_steps", walk, 2, 16), PackCase("long_order0", walk[:40000] >> 4, 0, 32)]
    x, x_bytes, rows, want = pack_call(cases)
    out, rows_out, recs = grib_cpx_pack(x, rows, want, x_bytes=x_bytes)
    check_against_host(cases, out, rows_out, recs, out.nbytes)
    assert int(recs["n_groups"][0]) == 5000


def test_many_short_rows_in_one_call(hip):
    """150 rows of 3 to 14 values, every seventh of width 0: the scan over the rows of the call (layout kernel, 64 rows at
    a step) takes three steps, and rows' offsets carry over both step boundaries."""
    rng = np.random.default_rng(11)
    cases = [PackCase(f"short{i}", np.zeros(3 + i % 12) if i % 7 == 3 else rng.integers(0, 1 << (1 + i % 16), 3 + i % 12),
                      i % 3, (8, 16, 32, 64)[i % 4], nbits=0 if i % 7 == 3 else 1 + i % 16) for i in range(150)]
    x, x_bytes, rows, want = pack_call(cases)
    out, rows_out, recs = grib_cpx_pack(x, rows, want, x_bytes=x_bytes)
    check_against_host(cases, out, rows_out, recs, out.nbytes)
    assert int(recs["byte_off"][64]) > 0 and int(recs["byte_off"][128]) > int(recs["byte_off"][64])


def test_round_trip_on_the_device(hip):
    """grib_unpack_cpx(grib_cpx_pack(x)) is x: the integers come back at their minimal width, byte for byte."""
    cases = [c for c in every_case() if c.n_values <= 5000]
    x, x_bytes, rows, want = pack_call(cases, gap=4)
    coded, rows_c, recs = grib_cpx_pack(x, rows, want, x_bytes=x_bytes)
    assert coded.nbytes % 4 == 0
    back, rows_b = grib_unpack_cpx(coded, rows_c, recs)
    host = back.to_host()
    for i, c in enumerate(cases):
        if c.nbits == 0:
            continue
        assert int(rows_b["nbits"][i]) == xc.width_of(c.X), c
        twin = pack_bits(c.X, xc.width_of(c.X))
        off = int(rows_b["byte_off"][i])
        assert np.array_equal(host[off:off + twin.size], twin), c


# ------------------------------------------------------------------------------------------------ the whole road
def same_field(got, want, what):
    assert got.shape == want.shape and got.n_points == want.n_points, what
    assert got.rows.tobytes() == want.rows.tobytes(), (what, got.rows, want.rows)
    assert got.bitmaps.tobytes() == want.bitmaps.tobytes(), (what, got.bitmaps, want.bitmaps)
    assert got.cpx.tobytes() == want.cpx.tobytes(), (what, got.cpx, want.cpx)
    assert np.array_equal(np.asarray(got.buf), np.asarray(want.buf)), what


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("case", ["plain", "bitmaps"])
def test_apply_host_grib_returns_complex_packed_streams(hip, case, skipna):
    """The 2048-cell grid of complex_cases to 333 cells, B = 8 rows: simple-packed and complex-packed input (cpx=), one
    chunk and chunks of three rows (three chunks).  The result has the bytes and the records of the host encode of the
    float64 result and decodes to the bits of the simple-packed grib_out result.  With cpx= input and SOURCE_WIDTH rows the
    oracle's widths are the widths of the source integers (`complex_cases.width_of`)."""
    op = operator()
    (buf, rows, cpx, bms), (tbuf, trows, _, tbms) = xc.build(**xc.CALLS[case])
    names = xc.CALLS[case]["names"]
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
        y = op.apply_host_grib(tbuf, trows, bitmaps=tbms, **common)
        simple = op.apply_host_grib(tbuf, trows, bitmaps=tbms, grib_out=GribEncode(16), **common)
        for par in (True, [(0, 8), (1, 64), (2, 16), (2, 32)] * 2):
            enc = GribEncode(16, cpx=par)
            want = enc.encode(y)
            assert np.array_equal(want.decode().view(np.uint32), simple.decode().view(np.uint32))
            for what, args in (("simple-packed input", dict(buf=tbuf, rows=trows, bitmaps=tbms)),
                               ("complex-packed input", dict(buf=buf, rows=rows, bitmaps=bms, cpx=cpx))):
                for chunk_rows in (0, 3):
                    got = op.apply_host_grib(grib_out=enc, chunk_rows=chunk_rows, **args, **common)
                    assert isinstance(got, GribField) and got.cpx is not None and got.bitmaps is not None and got.ccsds is None
                    same_field(got, want, f"{case} {what} chunk_rows={chunk_rows} {common}")
                    assert np.array_equal(np.asarray(got).view(np.uint32), simple.decode().view(np.uint32))
        # every second row takes the width of its source integers; a source of width 0 resolves within its chunk
        widths = np.array([xc.case(n).width for n in names], dtype=np.int32)
        marked = np.where(np.arange(widths.size) % 2 == 0, GribEncode.SOURCE_WIDTH, 12).astype(np.int32)
        enc = GribEncode(marked, cpx=True)
        for chunk_rows in (0, 3):
            step = chunk_rows or widths.size
            plain_w = np.where(marked == GribEncode.SOURCE_WIDTH, widths, marked)
            for r0 in range(0, widths.size, step):      # a constant source: the chunk's largest width, or 16
                part = plain_w[r0:r0 + step]
                part[part == 0] = part.max() if part.max() > 0 else 16
            want = GribEncode(plain_w, cpx=True).encode(y)
            got = op.apply_host_grib(buf, rows, bitmaps=bms, cpx=cpx, grib_out=enc, chunk_rows=chunk_rows, **common)
            same_field(got, want, f"{case} SOURCE_WIDTH chunk_rows={chunk_rows} {common}")
            assert np.array_equal(got.rows["nbits"] != 0, want.rows["nbits"] != 0)
        if masked and not skipna:
            assert (want.bitmaps["bitmap_off"] != GRIB_NO_BITMAP).any()          # the masked target cells are missing
    with pytest.raises(ValueError, match="SOURCE_WIDTH"):
        op.apply_host_grib(tbuf, trows, bitmaps=tbms, grib_out=enc)
    with pytest.raises(ValueError, match="cpx does not go with grib_out"):
        op.apply_host_grib(buf, rows, bitmaps=bms, cpx=cpx, grib_out=GribEncode(16, ccsds=True))
    with pytest.raises(ValueError, match="buffer of its own"):
        op.apply_host_grib(tbuf, trows, bitmaps=tbms, grib_out=GribEncode(16, cpx=True), out=np.zeros(1 << 20, np.uint8))


def test_ccsds_input_does_not_go_with_a_complex_result(hip):
    from smmregrid_amd import GRIB_AEC_DTYPE
    op = operator()
    _, (tbuf, trows, _, _) = xc.build(names=xc.GRID_ROWS[:2])
    with pytest.raises(ValueError, match="ccsds does not go with grib_out"):
        op.apply_host_grib(tbuf, trows, ccsds=np.zeros(2, dtype=GRIB_AEC_DTYPE), grib_out=GribEncode(16, cpx=True))


# ------------------------------------------------------------------------------------------------ Regridder
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("complex_out")
    paths = {}
    for kind in ("complex", "simple"):
        paths[kind] = str(d / f"t_{kind}.grib2")
        with open(paths[kind], "wb") as fh:
            fh.write(xc.grib2_message(xc.message_fields(kind == "complex")))
    return paths


@pytest.mark.parametrize("source", ["complex", "simple"])
def test_regridder_returns_complex_packed_fields_that_ship_raw_again(hip, files, caplog, monkeypatch, source):
    """The simple-packed twin file stores every field at the width of its integers (`width_of`), so its simple-packed
    grib_out result is the complex-packed result `at the same widths`."""
    dec = open_dataset(files["simple"])
    raw = open_dataset(files[source], decode=False, bitmaps=True)
    src = raw["t"].data
    assert isinstance(src, GribField) and (src.cpx is not None) == (source == "complex")
    w = CdoGenerate(dec["t"], "r16x8").weights(method="con")
    plain = Regridder(weights=w, packed=True, grib_out=True).regrid(open_dataset(files["simple"], decode=False, bitmaps=True)["t"])
    assert isinstance(plain.data, GribField) and plain.data.cpx is None
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, grib_out=True, grib_out_cpx=True, loglevel="INFO").regrid(raw["t"])
    assert not [r.getMessage() for r in caplog.records if "decoded on the host" in r.getMessage()
                or r.getMessage().startswith("grib_out:") or r.levelname == "WARNING"]
    f = got.data
    assert isinstance(f, GribField) and f.cpx is not None and f.bitmaps is not None and f.ccsds is None
    assert f.shape == plain.data.shape
    assert names.count("smm_grib_cpx_pack") == 1 and names.count("smm_grib_pack") == 1
    assert names.count("smm_grib_cpx_unpack") == (1 if source == "complex" else 0)
    assert "smm_grib_cpx_decode_host" not in names and "smm_apply_host" not in names
    # a complex-packed source field keeps its order, a simple-packed one gets order 2; all in groups of 32
    live = f.cpx["order"] != GRIB_CPX_SIMPLE
    want_order = np.where(src.cpx["order"] == GRIB_CPX_SIMPLE, 2, src.cpx["order"]) if source == "complex" else np.full(live.size, 2)
    assert np.array_equal(f.cpx["order"][live], want_order[live])
    assert np.array_equal(f.rows["nbits"], plain.data.rows["nbits"])
    assert got.dims == plain.dims and np.array_equal(np.asarray(got.values).view(np.uint32),
                                                     np.asarray(plain.values).view(np.uint32))
    # once more, raw: the coded result goes through the decode road of a second Regridder
    w2 = CdoGenerate(got, "r8x4").weights(method="con")
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        second = Regridder(weights=w2, packed=True, loglevel="INFO").regrid(got)
    assert names.count("smm_grib_cpx_unpack") == 1 and "smm_grib_cpx_decode_host" not in names
    assert not any("decoded on the host" in r.getMessage() for r in caplog.records)
    ref = Regridder(weights=w2).regrid(DataArray(np.asarray(got.values), dims=got.dims, coords=got.coords, attrs=got.attrs,
                                                 name=got.name))
    same_bits(np.asarray(second.values), np.asarray(ref.values), "second regrid, raw")
    # without the new keyword everything is as it was
    del names[:]
    caplog.clear()
    with caplog.at_level("INFO"):
        old = Regridder(weights=w, packed=True, grib_out=True, loglevel="INFO").regrid(raw["t"])
    assert "smm_grib_cpx_pack" not in names
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    if source == "complex":
        assert len(lines) == 1 and "grib_out" in lines[0] and not isinstance(old.data, GribField)
    else:
        assert not lines and isinstance(old.data, GribField) and old.data.cpx is None
        assert old.data.rows.tobytes() == plain.data.rows.tobytes() and np.array_equal(old.data.buf, plain.data.buf)
