"""Complex-packed GRIB-2 fields (templates 5.2 / 5.3) on the GPU (smm_grib_cpx_unpack; `grib_unpack_cpx`,
`apply_grib(cpx=)`, `apply_host_grib(cpx=)`, `Regridder(packed=True)` on a complex-packed variable).  Every comparison is
bit for bit: against the cases' integers (tests/complex_cases.py, coded by its numpy encoder) and against the same call on
the simple-packed twin of those integers.  Streams with bad offsets or lengths are the business of
tests/test_grib_complex.py and its host harness; the one error status provoked here is arithmetic."""
import numpy as np
import pytest

from smmregrid_amd import GRIB_CPX_DTYPE, CdoGenerate, GribField, Regridder, SparseOperator, _lib, grib_unpack_cpx, to_device
from smmregrid_amd.io import open_dataset
from smmregrid_amd.lazy import LazyArray
from tests import ccsds_cases as cc
from tests import complex_cases as xc
from tests.ccsds_cases import pack_bits

pytestmark = pytest.mark.gpu
S = xc.S


def same_bits(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == np.float64, (what, got.shape, want.shape, got.dtype)
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f"{what}: {int(diff.sum())} results differ in their bits, first at {np.argwhere(diff)[:3].tolist()}"


rules, simple_record, build = cc.rules, xc.simple_record, xc.build      # shared with tests/test_grib_chunk_plan.py


def device_bytes(buf):
    padded = np.full((buf.size + 3) // 4 * 4, 0x5A, dtype=np.uint8)
    padded[:buf.size] = buf
    return to_device(padded)


# ------------------------------------------------------------------------------------------------ grib_unpack_cpx
def all_cases_call():
    """Every case as a row of one call, streams at odd offsets with garbage between them, and a simple-packed row among
    them: (buf, rows, records, cases or None per row)."""
    cs = xc.cases()
    order = cs[:5] + [None] + cs[5:]
    rows = rules(len(order), seed=2)
    recs = np.zeros(len(order), dtype=GRIB_CPX_DTYPE)
    parts, at = [], 0
    for i, c in enumerate(order):
        pad = 1 + 2 * (i % 2)                                  # 1 or 3 bytes of garbage: every stream starts at an odd offset
        parts.append(np.full(pad, 0xA5, np.uint8))
        at += pad
        if c is None:
            rows["nbits"][i], rows["byte_off"][i] = 12, 12345   # passes through untouched
            recs[i] = simple_record()
            continue
        rows["nbits"][i] = c.params["nbits"]
        recs[i] = c.record(at)
        parts.append(c.stream)
        at += c.stream.size
    return np.concatenate(parts), rows, recs, order


def check_unpacked(host, rows, rows_out, order):
    end = 0
    for i, c in enumerate(order):
        r = rows_out[i]
        if c is None:
            assert r.tobytes() == rows[i].tobytes()
            continue
        assert (r["ref"], r["bscale"], r["ddiv"]) == (rows[i]["ref"], rows[i]["bscale"], rows[i]["ddiv"]), c
        assert int(r["nbits"]) == c.width, (c, int(r["nbits"]), c.width)
        off = int(r["byte_off"])
        assert off == end and off % 4 == 0, (c, off, end)          # the layout's slots: back to back, 4 bytes per value
        twin = pack_bits(c.X, c.width)
        written = (twin.size + 3) // 4 * 4
        want = np.zeros(written, np.uint8)
        want[:twin.size] = twin
        assert np.array_equal(host[off:off + written], want), c
        end = off + 4 * c.n_values
    return end


def test_grib_unpack_cpx_gives_every_cases_integers_in_one_call(hip):
    """All cases in one call -- orders 0 to 2, one to four octets per descriptor, group widths 0 to 32, 1 to 40000 groups,
    2 to 300000 values, an empty stream, X up to 2^32 - 1 -- and a simple-packed row among them: each slot starts with
    the bytes of the simple-packed twin at the row's minimal width, zero-padded to 4."""
    buf, rows, recs, order = all_cases_call()
    total = 4 * sum(c.n_values for c in order if c is not None)
    filled = to_device(np.full(total + 64, 0xFF, dtype=np.uint8))
    out, rows_out = grib_unpack_cpx(device_bytes(buf), rows, recs, x_bytes=buf.size, out=filled)
    host = out.to_host()
    assert check_unpacked(host, rows, rows_out, order) == total
    assert (host[total:] == 0xFF).all()                                    # nothing behind the layout is written
    widths = {int(r["nbits"]) for r, c in zip(rows_out, order) if c is not None}
    assert {0, 32} <= widths


def test_grib_unpack_cpx_with_split_launch_grids_gives_the_same_bytes(hip):
    """smm_debug_set_grid_limit(61): every kernel's grid is cut into launches of at most 61 workgroups (the big row alone
    needs 1172), rows and tiles falling on either side of a cut."""
    buf, rows, recs, order = all_cases_call()
    x = device_bytes(buf)
    whole, rows_whole = grib_unpack_cpx(x, rows, recs, x_bytes=buf.size)
    whole = whole.to_host()
    _lib.call("smm_debug_set_grid_limit", 61)
    try:
        cut, rows_cut = grib_unpack_cpx(x, rows, recs, x_bytes=buf.size)
        cut = cut.to_host()
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    assert rows_cut.tobytes() == rows_whole.tobytes()
    check_unpacked(cut, rows, rows_cut, order)
    check_unpacked(whole, rows, rows_whole, order)


def test_an_integer_outside_32_bits_is_the_rows_error(hip):
    """The one error status on the GPU, an arithmetic one: the same valid tables and bits, but the overall minimum g of
    the second differences replaced by 2^20, so that the prefix sums pass 2^32 in row 1 -- SMM_ERR_INVALID naming that
    row.  No offset or length of the stream is touched."""
    good, bad = xc.case("order1_noct2"), xc.case("order2_noct4")
    stream = bad.stream.copy()
    assert bad.params["n_oct"] == 4 and bad.params["order"] == 2
    stream[8:12] = (0x00, 0x10, 0x00, 0x00)                     # g: the third descriptor of four octets
    want = xc.numpy_decode(stream, bad.n_values, bad.params)
    assert want.min() >= 0 and want.max() >= 2 ** 32
    buf = np.concatenate([good.stream, stream])
    recs = np.array([good.record(0), bad.record(good.stream.size)], dtype=GRIB_CPX_DTYPE)
    with pytest.raises(_lib.SmmError) as err:
        grib_unpack_cpx(device_bytes(buf), rules(2), recs, x_bytes=buf.size)
    assert err.value.code == _lib.SMM_ERR_INVALID and "recs[1]" in str(err.value) and "invalid" in str(err.value)
    out, rows_out = grib_unpack_cpx(device_bytes(buf), rules(2)[:1], recs[:1], x_bytes=buf.size)       # row 0 alone is fine
    assert int(rows_out["nbits"][0]) == good.width


# ------------------------------------------------------------------------------------------------ the gather behind it
_OP = []


def operator():
    """2048 source cells, 333 destination rows (no multiple of 64), three links a row, one row without links, an
    epilogue."""
    if not _OP:
        rng = np.random.default_rng(3)
        n_dst = 333
        dst = np.repeat(np.arange(1, n_dst + 1), 3)
        dst = dst[dst != 6]
        src = rng.integers(1, S + 1, size=dst.size)
        src[:3] = (1, S, S)
        op = SparseOperator(S, n_dst, src, dst, rng.random(dst.size), device=0)
        op.set_epilogue((rng.random(n_dst) > 0.2).astype(np.int32), rng.random(n_dst))
        _OP.append(op)
    return _OP[0]


CASES = xc.CALLS


@pytest.mark.parametrize("skipna", [False, True])
@pytest.mark.parametrize("case", list(CASES))
def test_apply_grib_and_apply_host_grib_have_the_bits_of_the_simple_packed_twin(hip, case, skipna):
    """B = 8 rows of different orders, widths and groupings in one call; with bitmaps (one shared by two rows); with
    simple-packed rows among the complex-packed ones; plain and under skipna; the host form with chunk_rows=3 (8 = 3 + 3 +
    2: three chunks)."""
    op = operator()
    (buf, rows, cpx, bms), (tbuf, trows, _, tbms) = build(**CASES[case])
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        common = dict(masked=masked, remap_area_min=area_min, skipna=skipna)
        want = op.apply_grib(device_bytes(tbuf), trows, x_bytes=tbuf.size, bitmaps=tbms, **common).to_host()
        assert np.isfinite(want).any() and (case == "plain" or skipna or np.isnan(want).any())
        got = op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, bitmaps=bms, cpx=cpx, **common).to_host()
        same_bits(got, want, f"apply_grib {case} {common}")
        for chunk_rows in (0, 3):
            got = op.apply_host_grib(buf, rows, bitmaps=bms, cpx=cpx, chunk_rows=chunk_rows, **common)
            same_bits(got, want, f"apply_host_grib {case} chunk_rows={chunk_rows} {common}")


def test_cpx_goes_neither_with_ccsds_nor_with_grib_out(hip):
    from smmregrid_amd import GRIB_AEC_DTYPE, GribEncode
    op = operator()
    (buf, rows, cpx, _), _ = build(names=xc.GRID_ROWS[:2])
    with pytest.raises(ValueError, match="ccsds"):
        op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, cpx=cpx, ccsds=np.zeros(2, dtype=GRIB_AEC_DTYPE))
    with pytest.raises(ValueError, match="ccsds"):
        op.apply_host_grib(buf, rows, cpx=cpx, ccsds=np.zeros(2, dtype=GRIB_AEC_DTYPE))
    with pytest.raises(ValueError, match="grib_out"):
        op.apply_host_grib(buf, rows, cpx=cpx, grib_out=GribEncode(16))


# ------------------------------------------------------------------------------------------------ Regridder
def same_arrays(got, want, what):
    same_bits(np.asarray(got.values), np.asarray(want.values), what)
    assert got.dims == want.dims and got.attrs == want.attrs and got.name == want.name, what
    assert list(got.coords) == list(want.coords), what
    for k in got.coords:
        assert np.array_equal(got.coords[k].values, want.coords[k].values), (what, k)


@pytest.fixture(scope="module")
def files(tmp_path_factory):
    d = tmp_path_factory.mktemp("complex")
    paths = {}
    for kind in ("complex", "simple"):
        paths[kind] = str(d / f"t_{kind}.grib2")
        with open(paths[kind], "wb") as fh:
            fh.write(xc.grib2_message(xc.message_fields(kind == "complex")))
    return paths


def test_regridder_ships_a_complex_packed_variable_raw(hip, files, caplog, monkeypatch):
    """Six fields, two of them bitmapped (one through the bitmap of the field before), one simple-packed: plain, under
    skipna, lazily -- the bits of regridding the simple-packed twin file, raw and decoded."""
    dec, raw = open_dataset(files["complex"]), open_dataset(files["complex"], decode=False, bitmaps=True)
    twin = open_dataset(files["simple"], decode=False, bitmaps=True)
    f = raw["t"].data
    assert isinstance(f, GribField) and f.cpx is not None and f.bitmaps is not None and np.isnan(dec["t"].values).any()
    assert isinstance(twin["t"].data, GribField) and twin["t"].data.cpx is None
    w = CdoGenerate(dec["t"], "r16x8").weights(method="con")
    want = Regridder(weights=w).regrid(dec["t"])
    assert want.dtype == np.float64 and np.isfinite(want.values).any()
    same_arrays(Regridder(weights=w, packed=True).regrid(twin["t"]), want, "the simple-packed twin, raw")
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, loglevel="INFO").regrid(raw["t"])
    assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
    assert names.count("smm_grib_cpx_unpack") == 1 and names.count("smm_apply_grib_bm") == 1
    assert "smm_grib_cpx_decode_host" not in names and "smm_apply_host" not in names
    same_arrays(got, want, "packed=True on the complex-packed variable")
    # under skipna the raw road renormalises in the gather
    want_na = Regridder(weights=w, skipna=True).regrid(dec["t"])
    del names[:]
    got_na = Regridder(weights=w, packed=True, skipna=True, packed_skipna=True).regrid(raw["t"])
    assert names.count("smm_grib_cpx_unpack") == 1 and names.count("smm_apply_grib_na") == 1
    same_arrays(got_na, want_na, "skipna")
    # lazy
    lazy = Regridder(weights=w, packed=True, lazy=True).regrid(raw["t"])
    assert isinstance(lazy.data, LazyArray)
    same_bits(np.asarray(lazy.values), want.values, "lazy")
    # what does not take the road decodes on the host with one INFO line and gives the bits of the decoded variable
    for kw, word in ((dict(out_dtype=np.float32), "out_dtype float32"), (dict(grib_out=True), "grib_out")):
        caplog.clear()
        with caplog.at_level("INFO"):
            fb = Regridder(weights=w, packed=True, loglevel="INFO", **kw).regrid(raw["t"])
        lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
        assert len(lines) == 1 and word in lines[0], lines
        ref = Regridder(weights=w, **{k: v for k, v in kw.items() if k != "grib_out"}).regrid(dec["t"])
        assert fb.dtype == ref.dtype and np.array_equal(np.asarray(fb.values).view(np.uint8), ref.values.view(np.uint8)), word


def test_regridder_decodes_a_complex_packed_variable_on_the_host_for_masked_levels(hip, files, caplog):
    dec, raw = open_dataset(files["complex"]), open_dataset(files["complex"], decode=False, bitmaps=True)
    w3 = CdoGenerate(dec["t"], "r16x8").weights(method="con", mask_dim="isobaricInhPa")
    want = Regridder(weights=w3).regrid(dec["t"])
    for kw in (dict(), dict(packed_levels=True)):
        caplog.clear()
        with caplog.at_level("INFO"):
            got = Regridder(weights=w3, packed=True, loglevel="INFO", **kw).regrid(raw["t"])
        lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
        assert len(lines) == 1 and "complex packing" in lines[0] and "masked levels" in lines[0], lines
        same_arrays(got, want, f"masked levels {kw}")
