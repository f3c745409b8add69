"""Complex-packed GRIB-2 fields whose missing values are coded inside the groups (missing value management 1 / 2) without
a GPU: the host decoder (smm_grib_cpx_decode_host_mv, the text of smmregrid_amd/csrc/smm_grib_cpx.hpp) against the numpy
decoder of tests/complex_mv_cases.py on every case and on the hand-assembled row; `open_dataset(..., cpx_missing=True)`;
the three _mv entries' signatures, layout and refusals, which come before any device is touched; the chunk plan's budget;
and the decoder on truncated and corrupted input in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/grib_cpx_mv_harness.cpp)."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import smmregrid_amd
from smmregrid_amd import GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribField, _grib, _lib, griblite
from smmregrid_amd.io import open_dataset
from tests import complex_cases as xc
from tests import complex_mv_cases as mv

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES = mv.cases()
_u8p, _u64p = ctypes.POINTER(ctypes.c_uint8), ctypes.POINTER(ctypes.c_uint64)
cp = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribCpxStruct))               # noqa: E731


# ------------------------------------------------------------------------------------------------ the decoders
def test_the_case_list_covers_what_it_should():
    names = {c.name for c in CASES}
    assert {c.m for c in CASES} == {1, 2} and {c.order for c in CASES} == {0, 1, 2}
    assert mv.case("all_missing_nbits0_m1").params["nbits"] == 0 and mv.case("all_missing_nbits5_m2").params["nbits"] == 5
    assert mv.case("order2_P1_m2").P == 1 and mv.case("order2_P2_m1").P == 2 and mv.case("order2_none_missing_m1").P == mv.S
    assert not mv.case("order2_first3_missing_m2").present[:3].any()
    assert mv.case("order0_width32_group_m1").width == 32 and mv.case("short1500_order2_m1").n_values % 8
    assert mv.case("big70000_order2_m2").n_values == 70000 and "hand_m1" in names


@pytest.mark.parametrize("c", CASES, ids=repr)
def test_numpy_decoder_and_host_entry_agree(c):
    X, present = mv.numpy_decode(c.stream, c.n_values, c.params, c.m)
    assert np.array_equal(X, c.X) and np.array_equal(present, c.present)
    got, there = griblite.cpx_decode_mv(c.stream, c.record(0), c.m)
    assert got.dtype == np.uint32 and np.array_equal(got, c.X) and np.array_equal(there, c.present)
    # the entry itself, the stream at an odd offset in a larger buffer
    buf = np.full(c.stream.size + 11, 0xA5, dtype=np.uint8)
    buf[5:5 + c.stream.size] = c.stream
    rec = c.record(5).reshape(1)
    values, flags = np.full(c.n_values, 7, np.uint32), np.full(c.n_values, 7, np.uint8)
    status, count, m = ctypes.c_int(-1), ctypes.c_uint64(99), ctypes.c_uint8(c.m)
    assert _lib.load().smm_grib_cpx_decode_host_mv(buf.ctypes.data_as(ctypes.c_void_p), buf.size, cp(rec), ctypes.byref(m),
                                                   values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)),
                                                   flags.ctypes.data_as(_u8p), ctypes.byref(count), ctypes.byref(status)) == 0
    assert status.value == _lib.GRIB_CPX_OK and count.value == c.P
    assert np.array_equal(values[:c.P], c.X) and not values[c.P:].any() and np.array_equal(flags.astype(bool), c.present)


def test_mvm_zero_is_the_plain_decoder():
    c = xc.case("order2_noct3")
    got, there = griblite.cpx_decode_mv(c.stream, c.record(0), 0)
    assert np.array_equal(got, c.X) and there.all()


def test_the_hand_assembled_row():
    """The bytes were worked out by hand (the docstring of tests/complex_mv_cases.py)."""
    with open(os.path.join(mv.GOLDEN, "hand_mvm1.grib2"), "rb") as fh:
        msg = fh.read()
    assert msg == mv.hand_message() and len(msg) < 512
    c = mv.case("hand_m1")
    assert c.stream.tobytes() == mv.HAND_STREAM
    at = msg.index(mv.HAND_STREAM)
    assert msg[at - 5:at] == (5 + len(mv.HAND_STREAM)).to_bytes(4, "big") + bytes([7])
    s5 = msg[msg.index(bytes([0, 0, 0, 49, 5])):][:49]
    assert s5[5:11] == (10).to_bytes(4, "big") + (3).to_bytes(2, "big") and s5[19:49] == mv.HAND_S5
    assert c.bitmap.tobytes() == mv.HAND_BITMAP and c.width == 5 and c.packed.tobytes() == mv.HAND_COMPACT
    X, present = mv.numpy_decode(np.frombuffer(mv.HAND_STREAM, np.uint8), 10, c.params, 1)
    assert X.tolist() == [20, 23, 25, 24, 30] and np.array_equal(present, mv.HAND_PRESENT)
    got, there = griblite.cpx_decode_mv(mv.HAND_STREAM, c.record(0), 1)
    assert got.tolist() == [20, 23, 25, 24, 30] and np.array_equal(there, mv.HAND_PRESENT)


def test_the_hand_assembled_row_opens():
    path = os.path.join(mv.GOLDEN, "hand_mvm1.grib2")
    want = np.full(10, np.nan, np.float32)
    want[mv.HAND_PRESENT] = mv.HAND_X
    got = open_dataset(path, cpx_missing=True)["t"].values
    assert got.dtype == np.float32 and got.tobytes() == want.reshape(2, 5).tobytes()
    raw = open_dataset(path, decode=False, cpx_missing=True)["t"].data
    assert isinstance(raw, GribField) and raw.cpx_missing.tolist() == [1] and raw.cpx_missing.dtype == np.uint8
    assert np.asarray(raw).tobytes() == raw.decode().tobytes() == want.reshape(2, 5).tobytes()
    assert "missing values inside the groups" in repr(raw)
    for decode in (True, False):
        with pytest.raises(griblite.GribUnsupported, match="missing value management 1") as err:
            open_dataset(path, decode=decode)
        assert "cpx_missing" in str(err.value)


# ------------------------------------------------------------------------------------------------ griblite
RULES = [(270.0, -4, 0), (0.0, 2, 2), (-12.5, -6, 1)]
NAMES = ["order2_third_m1", "order1_third_m2", "order0_width32_group_m2"]


def _field(c, k, **kw):
    R, E, D = RULES[k]
    return dict(cpx=(c.stream, c.params, c.n_values), s5=xc.section5(c.n_values, c.params, R, E, D, mvm=c.m), R=R, E=E, D=D,
                level=(85000, 50000, 25000)[k], **kw)


def _rule(c, k):
    R, E, D = RULES[k]
    out = np.full(c.n_values, np.nan, dtype=np.float32)
    out[c.present] = ((float(np.float32(R)) + c.X.astype(np.float64) * 2.0 ** E) / 10.0 ** D).astype(np.float32)
    return out


def test_open_dataset_decodes_and_keeps_raw(tmp_path):
    cs = [mv.case(n) for n in NAMES]
    plain = xc.case("order1_noct2")
    p = tmp_path / "mv.grib2"
    p.write_bytes(xc.grib2_message([_field(c, k) for k, c in enumerate(cs)]) +
                  xc.grib2_message([dict(cpx=(plain.stream, plain.params, plain.n_values), level=10000)]))
    want = np.stack([(plain.X).astype(np.float32)] + [_rule(c, k) for k, c in reversed(list(enumerate(cs)))])   # level ascending
    got = open_dataset(str(p), cpx_missing=True)["t"].values
    assert got.dtype == np.float32 and got.reshape(4, -1).tobytes() == want.tobytes()
    raw = open_dataset(str(p), decode=False, cpx_missing=True)["t"].data
    assert isinstance(raw, GribField) and raw.cpx_missing.tolist() == [0, 2, 2, 1]
    assert raw.decode().reshape(4, -1).tobytes() == want.tobytes()
    with pytest.raises(griblite.GribUnsupported, match="missing value management"):
        open_dataset(str(p))
    # a file without such messages: the attribute is None
    q = tmp_path / "plain.grib2"
    q.write_bytes(xc.grib2_message([dict(cpx=(plain.stream, plain.params, plain.n_values))]))
    assert open_dataset(str(q), decode=False, cpx_missing=True)["t"].data.cpx_missing is None


def test_a_bitmap_and_codes_together_decode_on_the_host(tmp_path):
    c = mv.case("short1500_order2_m1")
    bitmap = xc.present_1500()
    p = tmp_path / "both.grib2"
    p.write_bytes(xc.grib2_message([_field(c, 0, bitmap=bitmap)]))
    coded = _rule(c, 0)
    want = np.full(xc.S, np.nan, dtype=np.float32)
    want[bitmap] = coded
    for kw in (dict(), dict(decode=False), dict(decode=False, bitmaps=True)):
        data = open_dataset(str(p), cpx_missing=True, **kw)["t"].data
        assert isinstance(data, np.ndarray) and data.ravel().tobytes() == want.tobytes()


def test_mvm_3_is_refused_with_the_keyword_too(tmp_path):
    c = mv.case("order1_third_m1")
    p = tmp_path / "m3.grib2"
    p.write_bytes(xc.grib2_message([dict(cpx=(c.stream, c.params, c.n_values), s5=xc.section5(c.n_values, c.params, mvm=3))]))
    with pytest.raises(griblite.GribUnsupported, match="missing value management 3"):
        open_dataset(str(p), cpx_missing=True)


# ------------------------------------------------------------------------------------------------ the ABI and its refusals
def test_header_exports_and_ctypes_table_agree():
    header = open(os.path.join(ROOT, "include", "smmregrid_amd.h")).read()
    lib = _lib.load()
    for entry in ("smm_grib_cpx_layout_mv", "smm_grib_cpx_unpack_mv", "smm_grib_cpx_decode_host_mv"):
        assert entry in _lib.SIGNATURES and getattr(lib, entry)
        proto = re.search(r"^int " + entry + r"\((.*?)\);", header, re.M | re.S).group(1)
        assert len(re.sub(r"/\*.*?\*/", "", proto).split(",")) == len(_lib.SIGNATURES[entry])
        assert "const uint8_t* mvm" in proto
    assert lib.smm_abi_version() == 6 and "#define SMM_ABI_VERSION 6" in header
    assert GRIB_CPX_DTYPE.itemsize == ctypes.sizeof(_lib.GribCpxStruct) == 72          # the record stays as it is
    assert "grib_unpack_cpx_mv" in smmregrid_amd.__all__ and smmregrid_amd.grib_unpack_cpx_mv is smmregrid_amd.device.grib_unpack_cpx_mv


def _rec(**kw):
    r = np.zeros(1, dtype=GRIB_CPX_DTYPE)
    r["byte_len"], r["n_values"], r["n_groups"], r["nbits"], r["width_ref"], r["width_bits"] = 64, 100, 4, 8, 3, 3
    r["length_ref"], r["length_inc"], r["length_last"], r["length_bits"], r["order"], r["n_oct"] = 20, 1, 40, 4, 2, 2
    for k, v in kw.items():
        r[k] = v
    return r


def test_layout_entry_on_a_hand_table():
    lib = _lib.load()
    recs = np.concatenate([_rec(n_values=5), _rec(order=-1, n_values=777), _rec(n_values=2048), _rec(n_values=33, order=0),
                           _rec(n_values=5)])
    mvm = np.array([1, 2, 0, 2, 0], dtype=np.uint8)
    offs, bms, total = np.zeros(5, np.uint64), np.zeros(5, np.uint64), ctypes.c_uint64(0)
    up = lambda a: a.ctypes.data_as(_u64p)               # noqa: E731
    assert lib.smm_grib_cpx_layout_mv(cp(recs), mvm.ctypes.data_as(_u8p), 5, up(offs), up(bms), ctypes.byref(total)) == 0
    # 20 + 4 (one bitmap byte rounded up) | nothing for the marked row | 8192 | 132 + 8 (five bitmap bytes rounded up) | 20
    assert offs.tolist() == [0, 24, 24, 24 + 8192, 24 + 8192 + 140]
    assert bms.tolist() == [20, GRIB_NO_BITMAP, GRIB_NO_BITMAP, 24 + 8192 + 132, GRIB_NO_BITMAP]
    assert total.value == 24 + 8192 + 140 + 20
    plain = ctypes.c_uint64(0)
    assert lib.smm_grib_cpx_layout_mv(cp(recs), None, 5, up(offs), up(bms), ctypes.byref(total)) == 0
    assert lib.smm_grib_cpx_layout(cp(recs), 5, None, ctypes.byref(plain)) == 0 and plain.value == total.value
    assert set(bms.tolist()) == {GRIB_NO_BITMAP}
    assert lib.smm_grib_cpx_layout_mv(cp(recs), mvm.ctypes.data_as(_u8p), 5, None, None, ctypes.byref(total)) == 0
    assert lib.smm_grib_cpx_layout_mv(cp(recs), mvm.ctypes.data_as(_u8p), 5, None, None, None) == _lib.SMM_ERR_INVALID
    mvm[3] = 3
    assert lib.smm_grib_cpx_layout_mv(cp(recs), mvm.ctypes.data_as(_u8p), 5, None, None, ctypes.byref(total)) == _lib.SMM_ERR_INVALID
    assert b"mvm[3]" in lib.smm_last_error()


def _unpack_status(rec, mvm, out_bytes=1 << 20, null=()):
    """smm_grib_cpx_unpack_mv with pointers that are never followed: every refusal comes before the device is touched."""
    rows, rows_out = np.zeros(rec.size, dtype=GRIB_ROW_DTYPE), np.zeros(rec.size, dtype=GRIB_ROW_DTYPE)
    bms = np.zeros(rec.size, dtype=GRIB_BITMAP_DTYPE)
    rp = lambda a: ctypes.cast(a.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))               # noqa: E731
    mvm = np.asarray(mvm, dtype=np.uint8)
    return _lib.load().smm_grib_cpx_unpack_mv(
        0, ctypes.c_void_p(0x1000), 64, cp(rec), mvm.ctypes.data_as(_u8p), rp(rows), rec.size, ctypes.c_void_p(0x2000), out_bytes,
        rp(rows_out), None if "bitmaps_out" in null else ctypes.cast(bms.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), None)


def test_unpack_mv_refuses_before_any_device():
    lib = _lib.load()
    two = np.concatenate([_rec(), _rec()])
    assert _unpack_status(two, [0, 3]) == _lib.SMM_ERR_INVALID and b"mvm[1]" in lib.smm_last_error()
    assert _unpack_status(two, [1, 1], null=("bitmaps_out",)) == _lib.SMM_ERR_INVALID and b"bitmap" in lib.smm_last_error()
    # the _mv layout: 400 + 16 (13 bitmap bytes rounded up) per row
    assert _unpack_status(two, [1, 1], out_bytes=831) == _lib.SMM_ERR_INVALID and b"832" in lib.smm_last_error()
    assert _unpack_status(two, [0, 1], out_bytes=815) == _lib.SMM_ERR_INVALID and b"816" in lib.smm_last_error()
    assert _unpack_status(np.concatenate([_rec(), _rec(reserved=1)]), [1, 1]) == _lib.SMM_ERR_INVALID
    # the host decode: a value above 2, null flags
    c = mv.case("hand_m1")
    rec, m = c.record(0).reshape(1), ctypes.c_uint8(3)
    values, flags, count, status = np.zeros(10, np.uint32), np.zeros(10, np.uint8), ctypes.c_uint64(0), ctypes.c_int(0)
    vp, sp = values.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)), c.stream.ctypes.data_as(ctypes.c_void_p)
    assert lib.smm_grib_cpx_decode_host_mv(sp, c.stream.size, cp(rec), ctypes.byref(m), vp, flags.ctypes.data_as(_u8p),
                                           ctypes.byref(count), ctypes.byref(status)) == _lib.SMM_ERR_INVALID
    m = ctypes.c_uint8(1)
    assert lib.smm_grib_cpx_decode_host_mv(sp, c.stream.size, cp(rec), ctypes.byref(m), vp, None, ctypes.byref(count),
                                           ctypes.byref(status)) == _lib.SMM_ERR_INVALID
    assert lib.smm_grib_cpx_decode_host_mv(sp, c.stream.size, cp(rec), ctypes.byref(m), vp, flags.ctypes.data_as(_u8p), None,
                                           ctypes.byref(status)) == _lib.SMM_ERR_INVALID


def test_operator_refuses_cpx_missing_without_cpx_or_with_a_bitmap_before_any_device():
    from smmregrid_amd import SparseOperator
    op = SparseOperator.__new__(SparseOperator)
    rows = np.zeros(2, dtype=GRIB_ROW_DTYPE)
    with pytest.raises(ValueError, match="cpx_missing goes with cpx"):
        op.apply_host_grib(np.zeros(64, np.uint8), rows, cpx_missing=[1, 1])
    with pytest.raises(ValueError, match="cpx_missing goes with cpx"):
        op.apply_grib(None, rows, cpx_missing=[1, 1])
    # a row with a bitmap of its own and codes inside its groups: both calls refuse it, rows without both pass that check
    cpx = np.concatenate([_rec(), _rec()])
    bms = np.zeros(2, dtype=GRIB_BITMAP_DTYPE)
    bms["bitmap_off"], bms["n_values"] = (GRIB_NO_BITMAP, 0), 100
    with pytest.raises(ValueError, match="bitmap and missing values"):
        op.apply_grib(None, rows, cpx=cpx, cpx_missing=[0, 1], bitmaps=bms)
    with pytest.raises(TypeError, match="uint8 DeviceArray"):          # past the refusal: the next check is x itself
        op.apply_grib(None, rows, cpx=cpx, cpx_missing=[1, 0], bitmaps=bms)
    op.n_src, op.n_dst = 100, 10
    with pytest.raises(ValueError, match="bitmap and missing values"):
        op.apply_host_grib(np.zeros(64, np.uint8), rows, cpx=cpx, cpx_missing=[0, 1], bitmaps=bms)


def test_plan_chunks_budgets_a_row_with_missing_values_by_the_stated_cost():
    """Beside CPX.device_cost: the bitmap slot, 8 B per value of second scratch, 4 B per 256 values."""
    n, ng = 2048, 64
    assert _grib.cpx_missing_cost(n) == 256 + 8 * n + 4 * 8 and _grib.cpx_missing_cost(1500) == 188 + 12000 + 24
    rows = np.zeros(4, dtype=GRIB_ROW_DTYPE)
    recs = np.concatenate([_rec(n_values=n, n_groups=ng, byte_len=1000, byte_off=1000 * i) for i in range(4)])
    missing = np.array([0, 1, 2, 0], dtype=np.uint8)
    n_dst = 100
    plain = 1000 + 12 * n + 16 * ng + 256 + 8 * n_dst
    coded = _grib.CodedRows.of(4, cpx=recs, cpx_missing=missing)
    chunks = list(_grib.plan_chunks(4000, rows, None, coded, n, n_dst, 0, plain + 2 * (plain + _grib.cpx_missing_cost(n)), 0))
    assert [(c.r0, c.r1) for c in chunks] == [(0, 3), (3, 4)] and chunks[0].missing.tolist() == [0, 1, 2]
    assert chunks[0].coded_bytes == 3 * 4 * n + 2 * 256 and chunks[1].coded_bytes == 4 * n
    one_less = list(_grib.plan_chunks(4000, rows, None, coded, n, n_dst, 0, plain + 2 * (plain + _grib.cpx_missing_cost(n)) - 1, 0))
    assert [(c.r0, c.r1) for c in one_less] == [(0, 2), (2, 4)]
    without = list(_grib.plan_chunks(4000, rows, None, _grib.CodedRows.of(4, cpx=recs), n, n_dst, 0, 3 * plain, 0))
    assert [(c.r0, c.r1) for c in without] == [(0, 3), (3, 4)] and without[0].missing is None
    bms = np.zeros(4, dtype=GRIB_BITMAP_DTYPE)
    bms["bitmap_off"], bms["n_values"] = 0, n
    with pytest.raises(ValueError, match="bitmap and missing values"):
        list(_grib.plan_chunks(4000, rows, bms, coded, n, n_dst, 0, 1 << 30, 0))


# ------------------------------------------------------------------------------------------------ malformed input
@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("grib_cpx_mv") / "grib_cpx_mv_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, os.path.join(ROOT, "tests", "cpp", "grib_cpx_mv_harness.cpp")])
    return exe


def test_malformed_input_ends_with_a_status_and_no_sanitizer_report(harness, tmp_path):
    cs = [c for c in CASES if c.n_values <= 4096]
    path = str(tmp_path / "cases.bin")
    with open(path, "wb") as fh:
        fh.write(np.int64(len(cs)).tobytes())
        for c in cs:
            fh.write(np.array([c.n_values] + [c.params[k] for k in xc.PARAM_NAMES] + [c.stream.size, c.m, c.P], np.int64).tobytes())
            fh.write(c.stream.tobytes())
            fh.write(c.X.astype(np.uint32).tobytes())
            fh.write(c.present.astype(np.uint8).tobytes())
    out = subprocess.run([harness, path], capture_output=True, text=True, timeout=600, env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    lines = [ln.split() for ln in out.stdout.splitlines() if ln.startswith("case ")]
    assert len(lines) == len(cs)
    for c, ln in zip(cs, lines):
        runs, ok, exhausted, invalid = int(ln[3]), int(ln[5]), int(ln[7]), int(ln[9])
        assert runs == ok + exhausted + invalid and runs >= 2 + c.stream.size + c.stream.size // 7 and ok >= 2
        assert exhausted >= c.stream.size - 8, (c, ln)          # a cut stream runs out (but for the pad bits)
