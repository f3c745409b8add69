"""CCSDS-packed GRIB-2 fields (data representation template 5.42) without a GPU: the host decoder
(smm_grib_aec_decode_host, the text of smmregrid_amd/csrc/smm_grib_aec.hpp) against the fixtures libaec's encoder wrote
and, where libaec is installed, against `aec_buffer_decode` on random streams; `griblite` on synthesized messages; the
refusals of the entries, which come before any device is touched; and the decoder on truncated and corrupted streams
in a stand-alone program under AddressSanitizer + UBSan (tests/cpp/grib_aec_harness.cpp)."""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import GRIB_AEC_DTYPE, GRIB_ROW_DTYPE, GribField, _lib, griblite
from smmregrid_amd.io import open_dataset
from tests import ccsds_cases as cc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIXTURES = cc.fixtures()


def test_the_fixture_set_is_there_and_small():
    names = {f.name for f in FIXTURES}
    assert len(FIXTURES) >= 30 and {"grid_w12_smooth", "grid_w16_runs", "short_w16_smooth"} <= names
    assert {f.nbits for f in FIXTURES} >= set(cc.WIDTHS) and {f.preprocess for f in FIXTURES} == {True, False}
    assert {f.block for f in FIXTURES} == {8, 16, 32, 64}
    edge = sorted({f.n_values for f in FIXTURES if f.name.startswith("edge_")})
    assert edge == [5, 7, 8, 9, 16, 17, 43]           # 5, J - 1, J, J + 1, J rsi, J rsi + 1, three RSIs and a ragged block
    for f in FIXTURES:
        assert os.path.getsize(os.path.join(cc.GOLDEN, f.name + ".npz")) < 256 * 1024


@pytest.mark.parametrize("fx", FIXTURES, ids=repr)
def test_host_decoder_equals_the_fixture(fx):
    got = cc.host_decode(fx.stream, fx.n_values, fx.nbits, fx.block, fx.rsi, fx.flags)
    assert got.dtype == np.uint32 and np.array_equal(got, fx.values)
    # the stream anywhere in a larger buffer, at an odd offset, garbage around it
    buf = np.full(fx.stream.size + 11, 0xA5, dtype=np.uint8)
    buf[5:5 + fx.stream.size] = fx.stream
    rec = cc.record(5, fx.stream.size, fx.n_values, fx.nbits, fx.block, fx.rsi, fx.flags)
    assert np.array_equal(griblite.aec_decode(buf, rec), fx.values)


def test_the_fixtures_take_every_coding_option():
    hist = cc.new_histogram()
    for fx in FIXTURES:
        cc.host_decode(fx.stream, fx.n_values, fx.nbits, fx.block, fx.rsi, fx.flags, hist)
    taken = dict(zip(_lib.GRIB_AEC_OPTIONS, hist.tolist()))
    assert len(taken) == 7 and all(taken.values()), f"a coding option is never taken: {taken}"


def test_container_flags_are_ignored_and_the_preprocessor_flag_is_not():
    fx = cc.fixture("grid_w12_smooth")
    for extra in (0, cc.MSB, cc.THREE_BYTE, cc.MSB | cc.THREE_BYTE):
        assert np.array_equal(cc.host_decode(fx.stream, fx.n_values, 12, fx.block, fx.rsi, cc.PREPROCESS | extra), fx.values)
    try:
        other = cc.host_decode(fx.stream, fx.n_values, 12, fx.block, fx.rsi, 0)
    except ValueError:
        return
    assert not np.array_equal(other, fx.values)


def test_random_streams_decode_as_libaec_decodes_them():
    if cc.load_libaec() is None:
        pytest.skip("libaec is not installed here")
    rng = np.random.default_rng(42)
    for it in range(300):
        nbits = int(rng.choice(cc.WIDTHS + (3, 5, 9, 25, 31)))
        block, rsi = int(rng.choice([8, 16, 32, 64])), int(rng.choice([1, 2, 3, 64, 128, 4096]))
        pp = bool(it & 1)
        n = min(int(rng.choice([1, 5, block - 1, block, block + 1, block * rsi, block * rsi + 1, 777, 2048, 5000])), 6000)
        xmax = (1 << nbits) - 1
        kind = it % 5
        if kind == 0:
            v = rng.integers(0, xmax + 1, n, dtype=np.uint64)
        elif kind == 1:
            v = np.clip(np.cumsum(rng.integers(-3, 4, n)) + xmax // 2, 0, xmax).astype(np.uint64)
        elif kind == 2:
            v = np.where(rng.random(n) < 0.5, 0, xmax).astype(np.uint64)
        elif kind == 3:
            v = np.clip(xmax // 3 + (rng.random(n) < 0.1), 0, xmax).astype(np.uint64)
        else:
            v = np.clip(np.cumsum(rng.integers(-40, 41, n)) + xmax // 2, 0, xmax).astype(np.uint64)
            v[n // 3:n // 3 + 700] = v[n // 3]
        stream = cc.aec_encode(v, nbits, block, rsi, pp)
        want = cc.aec_decode_libaec(stream, n, nbits, block, rsi, pp)
        got = cc.host_decode(stream, n, nbits, block, rsi, cc.PREPROCESS if pp else 0)
        assert np.array_equal(got, want), (it, nbits, block, rsi, pp, n, kind)


# ------------------------------------------------------------------------------------------------ griblite
NI, NJ = cc.NI, cc.NJ


@pytest.fixture(scope="module")
def twins(tmp_path_factory):
    d = tmp_path_factory.mktemp("ccsds_grib")
    paths = {}
    for kind in ("ccsds", "simple"):
        paths[kind] = str(d / f"{kind}.grib2")
        with open(paths[kind], "wb") as fh:
            fh.write(cc.grib2_message(cc.message_fields(kind == "ccsds"), NI, NJ))
    return paths


def test_decoded_opening_gives_the_floats_of_the_simple_packed_twin(twins):
    got, want = open_dataset(twins["ccsds"]), open_dataset(twins["simple"])
    assert got["t"].shape == want["t"].shape == (2, 3, NJ, NI)
    assert got["t"].values.dtype == np.float32
    assert got["t"].values.tobytes() == want["t"].values.tobytes()
    assert np.isnan(want["t"].values[1, 2]).sum() == NI * NJ - 1500       # the bitmapped fields are there


@pytest.mark.parametrize("bitmaps", [False, True])
def test_raw_opening_keeps_the_records(twins, bitmaps):
    decoded = open_dataset(twins["simple"])["t"].values
    ds = open_dataset(twins["ccsds"], decode=False, bitmaps=bitmaps)
    data = ds["t"].data
    if not bitmaps:      # a variable with bitmapped messages is decoded unless bitmaps=True
        assert isinstance(data, np.ndarray) and data.tobytes() == decoded.tobytes()
        return
    assert isinstance(data, GribField) and data.ccsds is not None and data.ccsds.dtype == GRIB_AEC_DTYPE
    assert data.ccsds.size == data.rows.size == 6 and "CCSDS" in repr(data)
    names = [name for name, *_ in sorted(cc.MESSAGE_SPECS, key=lambda sp: (sp[2], sp[1]))]     # (time, level ascending)
    assert names[2] == "short_w16_smooth" and names[5] == "short_w12_rough"
    for rec, row, name in zip(data.ccsds, data.rows, names):
        fx = cc.fixture(name)
        assert (int(rec["nbits"]), int(rec["block_size"]), int(rec["rsi"]), int(rec["flags"])) == \
            (fx.nbits, fx.block, fx.rsi, fx.flags)
        assert int(rec["n_values"]) == fx.n_values and int(rec["byte_len"]) == fx.stream.size
        assert int(rec["byte_off"]) == int(row["byte_off"]) and int(row["nbits"]) == fx.nbits
        off = int(rec["byte_off"])
        assert np.array_equal(data.buf[off:off + fx.stream.size], fx.stream)
    assert int((data.bitmaps["bitmap_off"] != smmregrid_amd.GRIB_NO_BITMAP).sum()) == 2
    assert data.bitmaps["bitmap_off"][2] == data.bitmaps["bitmap_off"][5]          # the reused bitmap
    assert data.decode().tobytes() == decoded.tobytes()
    assert np.asarray(data).tobytes() == decoded.tobytes()


def test_a_constant_ccsds_field_has_no_stream(tmp_path):
    msg = cc.grib2_message([dict(q=np.zeros(NI * NJ, np.uint64), nbits=0, R=7.5, ccsds=(np.zeros(0, np.uint8), 14, 32, 128))],
                           NI, NJ)
    p = tmp_path / "const.grib2"
    p.write_bytes(msg)
    assert np.array_equal(open_dataset(str(p))["t"].values, np.full((NJ, NI), 7.5, np.float32))
    raw = open_dataset(str(p), decode=False)["t"].data
    assert isinstance(raw, GribField) and raw.ccsds is None and np.array_equal(raw.decode(), np.full((NJ, NI), 7.5, np.float32))


@pytest.mark.parametrize("flag, what", [(1, "AEC_DATA_SIGNED"), (16, "AEC_RESTRICTED"), (32, "AEC_PAD_RSI")])
def test_refused_flags_are_named(tmp_path, flag, what):
    fx = cc.fixture("grid_w12_smooth")
    msg = cc.grib2_message([dict(q=fx.values, nbits=12, ccsds=(fx.stream, fx.flags | flag, fx.block, fx.rsi))], NI, NJ)
    p = tmp_path / "flag.grib2"
    p.write_bytes(msg)
    for decode in (True, False):
        with pytest.raises(griblite.GribUnsupported, match=what):
            open_dataset(str(p), decode=decode)


def test_a_stream_that_ends_early_is_an_error_not_numbers(tmp_path):
    fx = cc.fixture("grid_w12_smooth")
    msg = cc.grib2_message([dict(q=fx.values, nbits=12, ccsds=(fx.stream[:fx.stream.size // 2], fx.flags, fx.block, fx.rsi))],
                           NI, NJ)
    p = tmp_path / "short.grib2"
    p.write_bytes(msg)
    with pytest.raises(ValueError, match="ends before"):
        open_dataset(str(p))


# ------------------------------------------------------------------------------------------------ the ABI and its refusals
def test_record_dtype_is_the_struct_field_for_field():
    assert GRIB_AEC_DTYPE.itemsize == ctypes.sizeof(_lib.GribAecStruct) == 48
    for name, ctype in _lib.GribAecStruct._fields_:
        assert GRIB_AEC_DTYPE.fields[name][1] == getattr(_lib.GribAecStruct, name).offset
        assert GRIB_AEC_DTYPE.fields[name][0].itemsize == ctypes.sizeof(ctype)
    header = open(os.path.join(ROOT, "include", "smmregrid_amd.h")).read()
    assert "SMM_GRIB_AEC_OPTIONS 7" in header and len(_lib.GRIB_AEC_OPTIONS) == 7


def _rec(**kw):
    r = np.zeros(1, dtype=GRIB_AEC_DTYPE)
    r["byte_len"], r["n_values"], r["nbits"], r["block_size"], r["rsi"], r["flags"] = 64, 100, 12, 32, 128, 8
    for k, v in kw.items():
        r[k] = v
    return r


def _unpack_status(rec, x=0x1000, x_bytes=64, out=0x2000, out_bytes=1 << 20, n_batch=None, rows_nbits=None, null=()):
    """smm_grib_aec_unpack with pointers that are never followed: every refusal comes before the device is touched."""
    n_batch = rec.size if n_batch is None else n_batch
    rows = np.zeros(max(rec.size, 1), dtype=GRIB_ROW_DTYPE)
    rows["nbits"] = rec["nbits"] if rows_nbits is None else rows_nbits
    rows_out = np.zeros_like(rows)
    rp = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))               # noqa: E731
    return _lib.load().smm_grib_aec_unpack(
        0, None if "x" in null else ctypes.c_void_p(x), x_bytes,
        None if "recs" in null else ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribAecStruct)),
        None if "rows_in" in null else rp(rows), n_batch, None if "out" in null else ctypes.c_void_p(out), out_bytes,
        None if "rows_out" in null else rp(rows_out), None)


REFUSALS = [dict(rec=_rec(nbits=-1)), dict(rec=_rec(nbits=33)), dict(rec=_rec(block_size=0)), dict(rec=_rec(block_size=12)),
            dict(rec=_rec(block_size=128)), dict(rec=_rec(rsi=0)), dict(rec=_rec(rsi=4097)), dict(rec=_rec(flags=8 | 1)),
            dict(rec=_rec(flags=8 | 16)), dict(rec=_rec(flags=8 | 32)), dict(rec=_rec(flags=8 | 64)), dict(rec=_rec(reserved=1)),
            dict(rec=_rec(n_values=2 ** 31)), dict(rec=_rec(byte_off=1)), dict(rec=_rec(byte_len=65)),
            dict(rec=_rec(byte_off=2 ** 63, byte_len=2 ** 63)), dict(rec=_rec(), out_bytes=149), dict(rec=_rec(), x=0x1002),
            dict(rec=_rec(), out=0x2001), dict(rec=_rec(), n_batch=-1), dict(rec=_rec(), x_bytes=-1), dict(rec=_rec(), out_bytes=-1),
            dict(rec=_rec(), rows_nbits=16), dict(rec=_rec(), null=("x",)), dict(rec=_rec(), null=("out",)),
            dict(rec=_rec(), null=("recs",)), dict(rec=_rec(), null=("rows_in",)), dict(rec=_rec(), null=("rows_out",))]


@pytest.mark.parametrize("kw", REFUSALS, ids=lambda kw: ",".join(f"{k}" for k in kw if k != "rec") or "rec")
def test_unpack_refuses_before_any_device(kw):
    assert _unpack_status(**kw) == _lib.SMM_ERR_INVALID
    assert _lib.load().smm_last_error()


def test_refusals_name_the_flag_and_the_row():
    lib = _lib.load()
    two = np.concatenate([_rec(), _rec(flags=8 | 16)])
    assert _unpack_status(two, out_bytes=1 << 20) == _lib.SMM_ERR_INVALID
    assert b"recs[1]" in lib.smm_last_error() and b"AEC_RESTRICTED" in lib.smm_last_error()
    assert _unpack_status(_rec(flags=9)) == _lib.SMM_ERR_INVALID and b"AEC_DATA_SIGNED" in lib.smm_last_error()
    assert _unpack_status(_rec(flags=40)) == _lib.SMM_ERR_INVALID and b"AEC_PAD_RSI" in lib.smm_last_error()


def test_what_unpack_takes_without_a_device():
    """An empty call and a call of constant rows alone have nothing to do: SMM_OK with no device looked for; a row of
    width 0 passes through whatever its other fields hold."""
    assert _unpack_status(_rec(), n_batch=0, null=("x", "out", "recs", "rows_in", "rows_out")) == _lib.SMM_OK
    assert _unpack_status(_rec(nbits=0, block_size=0, rsi=0, flags=0xFFFF, byte_len=0), out_bytes=0, null=("x", "out")) == _lib.SMM_OK


def test_layout_and_host_decode_entries():
    lib = _lib.load()
    recs = np.concatenate([_rec(n_values=5, nbits=12), _rec(nbits=0), _rec(n_values=2048, nbits=17), _rec(n_values=3, nbits=1)])
    offs, total = np.zeros(4, np.uint64), ctypes.c_uint64(0)
    ap = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribAecStruct))               # noqa: E731
    assert lib.smm_grib_aec_layout(ap(recs), 4, offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(total)) == 0
    assert offs.tolist() == [0, 8, 8, 8 + 4352] and total.value == 8 + 4352 + 4          # each rounded up to 4 bytes
    assert lib.smm_grib_aec_layout(ap(recs), 4, None, None) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_layout(ap(_rec(block_size=7)), 1, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    fx = cc.fixture("edge_n5_w16_pp1")
    values, status = np.zeros(5, np.uint32), ctypes.c_int(-1)
    vp = values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32))
    rec = cc.record(0, fx.stream.size, 5, fx.nbits, fx.block, fx.rsi, fx.flags).reshape(1)
    sp = fx.stream.ctypes.data_as(ctypes.c_void_p)
    assert lib.smm_grib_aec_decode_host(sp, fx.stream.size, ap(rec), vp, None, ctypes.byref(status)) == 0
    assert status.value == _lib.GRIB_AEC_OK and np.array_equal(values, fx.values)
    assert lib.smm_grib_aec_decode_host(sp, fx.stream.size - 1, ap(rec), vp, None, ctypes.byref(status)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_decode_host(sp, fx.stream.size, ap(rec), None, None, ctypes.byref(status)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_aec_decode_host(sp, fx.stream.size, ap(rec), vp, None, None) == _lib.SMM_ERR_INVALID
    short = cc.record(0, 1, 5, fx.nbits, fx.block, fx.rsi, fx.flags).reshape(1)
    assert lib.smm_grib_aec_decode_host(sp, fx.stream.size, ap(short), vp, None, ctypes.byref(status)) == 0
    assert status.value == _lib.GRIB_AEC_EXHAUSTED


def grib_reason(dims, levels=False, out_dtype=np.float64, codec=None, mask_dim="isobaricInhPa", **switches):
    """why `road.decide` sends a `GribField` with these dims to the host decoder, or None: it stays raw"""
    from smmregrid_amd import road
    horizontal = [d for d in dims if d in ("lat", "lon", "latitude", "longitude")]
    way = road.decide(road.Switches.of(out_dtype=out_dtype, **switches),
                      road.Facts("t", road.GRIB, np.float32, dims, horizontal, mask_dim if levels else None, codec=codec))
    assert (way.source == road.RAW_GRIB) == (way.why is None) and way.source in (road.RAW_GRIB, road.DECODED)
    return way.why


def test_regridder_knows_why_a_ccsds_field_is_decoded():
    """road.decide: masked levels, grib_out and a non-float64 result send a CCSDS field to the host decoder."""
    on = dict(packed=True, packed_levels=True)
    dims = ("isobaricInhPa", "latitude", "longitude")
    assert grib_reason(dims, codec="ccsds", **on) is None
    assert "CCSDS" in grib_reason(dims, levels=True, codec="ccsds", **on)
    assert "float32" in grib_reason(dims, out_dtype=np.float32, codec="ccsds", **on)
    on["grib_out"] = True
    assert "grib_out" in grib_reason(dims, codec="ccsds", **on)
    assert grib_reason(dims, **on) is None
    on["skipna"] = True
    assert grib_reason(dims, **on) == "skipna"


# ------------------------------------------------------------------------------------------------ malformed streams
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib_aec") / "grib_aec_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_aec_harness.cpp")])
    return exe


def test_truncated_and_corrupted_streams_end_with_a_status_and_no_sanitizer_report(harness, tmp_path):
    """Every fixture, and behind them the malformed forced streams of tests/ccsds_forced_cases.py (group G): those end
    with the status the case names as they stand, and are cut and corrupted like the fixtures.  The device kernel meets
    the G streams in tests/test_gpu_grib_ccsds_forced.py."""
    from tests import ccsds_forced_cases as fc
    forced = fc.group("G")
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.int64(len(FIXTURES) + len(forced)).tobytes())
        for i, fx in enumerate(FIXTURES + forced):
            status = fx.meta["status"] if i >= len(FIXTURES) else _lib.GRIB_AEC_OK
            fh.write(np.array([fx.n_values, fx.nbits, fx.block, fx.rsi, int(fx.preprocess), fx.stream.size, status], np.int64).tobytes())
            fh.write(fx.stream.tobytes())
            fh.write(fx.values.astype(np.uint32).tobytes())
    out = subprocess.run([harness, path], capture_output=True, text=True, timeout=600,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(FIXTURES) + len(forced)
    for g, ln in zip(forced, lines[len(FIXTURES):]):
        runs, ok, exhausted, invalid = int(ln[3]), int(ln[5]), int(ln[7]), int(ln[9])
        assert runs == ok + exhausted + invalid and runs >= 2 + g.stream.size, (g, ln)
    for fx, ln in zip(FIXTURES, lines):
        runs, ok, exhausted, invalid = int(ln[3]), int(ln[5]), int(ln[7]), int(ln[9])
        assert runs == ok + exhausted + invalid and runs >= 2 + fx.stream.size
        assert exhausted >= fx.stream.size - 8, (fx, ln)      # a cut stream runs out (but for the encoder's pad bytes)
