"""The GRIB device entries that came after tests/test_gpu_far_offsets.py, at byte offsets past 2^31, 2^32 and 2^34 and at
bit positions past 2^32 inside one row: the gathers smm_apply_grib_na, smm_group_apply_grib and smm_group_apply_grib_na,
the packer smm_grib_pack, and the four transcoders smm_grib_cpx_unpack, smm_grib_aec_unpack, smm_grib_cpx_pack and
smm_grib_aec_pack, whose bit-stream and addressing code is smm_grib_xcode.hpp's.  (smm_apply_grib, smm_apply_grib_bm and
every entry that takes no packed bytes are the business of tests/test_gpu_far_offsets.py, whose buffers, fixture, memory
rule and seed are used here.)

Input far: the packed bytes are "one buffer of the whole file" of just over 2^34 bytes, filled with decoys; three true
rows lie just past 2^31, 2^32 (at an odd offset) and 2^34 bytes, the last one ending in the buffer's last word; two more
lie near, and a sixth sits where the second one's offset lands mod 2^32 and holds a different valid stream of the same
record shape, so that a narrowed offset decodes cleanly to the wrong integers (tests/far_cases.py; tests/test_far_cases.py
shows on the CPU that each narrowing is caught).

Output far: an output offset is never an argument, it is the sum of the rows before it.  smm_grib_pack gets 1030 rows of
2^20 points; the transcoders get SPACER rows between three true rows A, B and C: the decoy bits of X taken as 32-bit
samples.  No host array of a spacer's size exists: the spacers are sized from a host encode of a 2^20-sample of the same
bits, the records the call returns must put B past 2^31 and C past 2^32 bytes, and after the way back through the
unpacker (input, slots and scratch all far) the first and the last 1024 values of every spacer must be the samples of X.

Every expected value comes from code that is not the entry under test: the simple-packed twin (`pack_bits`), the template
encoder of tests/complex_cases.py, the libaec-written fixtures, the host encoders, and smm_apply / smm_group_apply on the
host-decoded field.  Every output buffer is filled with 0x42 and is checked behind the bytes used.

SMM_FAR_REPORT=<path> writes per case the peak device bytes and the wall time as JSON lines (profiles/grib_far_offsets.jsonl)."""
import ctypes

import numpy as np
import pytest

from smmregrid_amd import (GRIB_AEC_DTYPE, GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribEncode,
                           _grib, _lib, aec_encode, cpx_encode, grib_aec_pack, grib_cpx_pack, grib_unpack, grib_unpack_cpx)
from smmregrid_amd.device import DeviceArray, mem_info
from smmregrid_amd.griblite import cpx_want
from tests import ccsds_cases as cc
from tests import ccsds_encode_cases as ec
from tests import complex_cases as xc
from tests import far_cases as fc
from tests import grib_pack_cases as pc
from tests import test_gpu_grib_ccsds as t_aec
from tests import test_gpu_grib_ccsds_encode as t_aec_pack
from tests import test_gpu_grib_complex as t_cpx
from tests import test_gpu_grib_complex_encode as t_cpx_pack
from tests.test_gpu_far_offsets import (AREA_MIN, F32, F64, GIB, LEVEL_INDEX, MASKED_LEVELS, SEED, SELL, U8, Far, far,  # noqa: F401
                                        grib_case, reference, sell_operator, tile_group)
from tests.test_gpu_grib_pack import check as check_packed

pytestmark = pytest.mark.gpu

_vp = ctypes.c_void_p
P31, P32, P33 = 1 << 31, 1 << 32, 1 << 33


# ------------------------------------------------------------------ buffers

def byte_view(arr, start=0, n=None):
    """Bytes [start, start + n) of a device array, as a uint8 view."""
    n = arr.nbytes - start if n is None else n
    assert 0 <= start and start + n <= arr.nbytes
    return DeviceArray((int(n),), U8, ptr=arr.ptr + int(start), base=arr)


def reader(arr):
    """read(start, stop) -> host bytes of a device array, for the checks of tests/far_cases.py."""
    return lambda s, e: byte_view(arr, s, e - s).to_host()


def decoy_bytes(far, x_bytes, pieces, seed):
    """The packed bytes of a case: x_bytes (rounded up to a word) of `fill_random` float32 decoys, then the pieces
    [(byte offset, bytes)] copied in.  The decoys reach the far end of the buffer."""
    xa = far.alloc(fc._round4(x_bytes) // 4, F32).fill_random(seed=seed, mean=1000.0, sigma=50.0)
    tail = byte_view(xa, xa.nbytes - 64, 64).to_host().view(np.float32)
    assert (np.abs(tail - 1000.0) < 400.0).all(), tail
    for off, data in pieces:
        data = np.frombuffer(data, U8)
        assert off + data.size <= x_bytes
        byte_view(xa, off, data.size).copy_from_host(data)
    return xa


def sentinel_bytes(far, n):
    return far.alloc(n, U8).fill_bytes(fc.SENTINEL)


def release(far, arr):
    """Free one buffer of a case as soon as it is checked."""
    far.live.remove(arr)
    far.bytes -= arr.nbytes
    arr.free()


def scratch(far, nbytes):
    """The memory rule for what an entry allocates itself: skip if it does not fit, count it into the case's peak."""
    free = mem_info()[0]
    if free < nbytes + 2 * GIB:
        pytest.skip(f"{free / GIB:.1f} GiB of device memory free, the call needs {nbytes / GIB:.1f} GiB of scratch + 2 GiB")
    far.peak = max(far.peak, far.bytes + int(nbytes))


def _rp(rows):
    return ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))


def _bp(bitmaps):
    return None if bitmaps is None else ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct))


def same_bits(got, want, what):
    diff = got.view(np.uint64) != want.view(np.uint64)
    assert not diff.any(), f"{what}: {int(diff.sum())} results differ in their bits, first at {np.argwhere(diff)[:3].tolist()}"


# ------------------------------------------------------------------ A: the gathers that came after the far test

@pytest.mark.parametrize("bitmapped", [False, True], ids=["plain", "bitmaps"])
def test_apply_grib_na(far, bitmapped):
    """The buffer of `grib_case` -- rows just past 2^32 and (odd) 2^34 bytes, a far bitmap with a near stream and the
    reverse -- under skipna, with the bitmap pointer null and with bitmaps: the bits of smm_apply with SKIPNA | SELL on
    the decoded field, itself tied to the skipna oracle."""
    op, csr, imask, frac = sell_operator()
    x_bytes, pieces, rows, bitmaps, fld = grib_case()
    sel = [0, 1, 2, 3, 4] if bitmapped else [0, 1, 4]
    xa = decoy_bytes(far, x_bytes, pieces, seed=9)
    x = np.ascontiguousarray(fld[sel])
    assert np.isnan(x).any() == bitmapped
    flags = _lib.APPLY_MASKED | _lib.APPLY_SKIPNA
    lx, ly = fc.near_layout(len(sel), op.n_src), fc.near_layout(len(sel), op.n_dst)
    Xd, Yd = far.x(lx, F32, x), far.y(ly, F64)
    _lib.call("smm_apply", op.handle, Xd.ptr, _lib.SMM_F32, op.n_src, Yd.ptr, _lib.SMM_F64, op.n_dst, len(sel), AREA_MIN,
              SELL | flags, None)
    want = Yd.rows()
    fc.check_rows(want, reference(csr, x, imask, frac, skipna=True), "smm_apply with SKIPNA on the decoded field")
    Y = far.y(ly, F64)
    r = np.ascontiguousarray(rows[sel])
    bm = np.ascontiguousarray(bitmaps[sel]) if bitmapped else None
    _lib.call("smm_apply_grib_na", op.handle, _vp(xa.ptr), x_bytes, _rp(r), _bp(bm), Y.ptr, _lib.SMM_F64, op.n_dst, len(sel),
              AREA_MIN, flags, None)
    same_bits(Y.rows(), want, f"smm_apply_grib_na {'with' if bitmapped else 'without'} bitmaps")


def near_pieces(pieces, rows, bitmaps):
    """The same pieces back to back at odd near offsets: (x_bytes, pieces, rows, bitmaps) of the case whose X is near."""
    moved, out, at = {}, [], 0
    for off, data in sorted(pieces):
        at = (at + 8) | 1
        moved[off] = at
        out.append((at, data))
        at += len(data)
    rows, bitmaps = rows.copy(), bitmaps.copy()
    rows["byte_off"] = [moved[int(o)] for o in rows["byte_off"]]
    bitmaps["bitmap_off"] = [GRIB_NO_BITMAP if int(o) == GRIB_NO_BITMAP else moved[int(o)] for o in bitmaps["bitmap_off"]]
    return at + 3, out, rows, bitmaps


@pytest.mark.parametrize("side", ["x", "y"])
@pytest.mark.parametrize("skipna", [False, True], ids=["grib", "grib_na"])
def test_group_apply_grib(far, skipna, side):
    """2 levels x 3 outer x 1 inner on the small tile group: record (o, l) is row 2 o + l of `grib_case(S, 6)`, so each
    level has a record past 2^32 and one past 2^34 bytes, two of the six with a bitmap (one far, one near).  side x: that
    buffer, Y near.  side y: the same pieces near, Y on the far strides of `rows_layout` -- ys_outer * o crosses 2^31 and
    2^32 elements -- with every guard band and alias window checked.  The bits of smm_group_apply on the decoded field."""
    grp, members = tile_group()
    S, D = grp.n_src, grp.n_dst
    n_outer, n_lev, n_inner = 3, 2, 1
    lev = np.ascontiguousarray(LEVEL_INDEX[:n_lev])
    x_bytes, pieces, rows, bitmaps, fld = grib_case(S, n_outer * n_lev)
    assert sum(o > P32 for o in rows["byte_off"][0::2]) >= 2 and sum(o > P32 for o in rows["byte_off"][1::2]) >= 2
    assert (rows["byte_off"][0::2] > 1 << 34).any() and (rows["byte_off"][1::2] > 1 << 34).any()
    if side == "y":
        x_bytes, pieces, rows, bitmaps = near_pieces(pieces, rows, bitmaps)
    xa = decoy_bytes(far, x_bytes, pieces, seed=9)
    x = fld.reshape(n_outer, n_lev, S)
    ref = np.empty((n_outer, n_lev, D))
    for l in range(n_lev):
        _, csr, imask, frac = members[lev[l]]
        ref[:, l] = reference(csr, x[:, l], imask, frac, skipna=skipna, masked=bool(MASKED_LEVELS[lev[l]]))
    flags = _lib.APPLY_MASKED | (_lib.APPLY_SKIPNA if skipna else 0)
    lev_p, msk_p = lev.ctypes.data_as(_vp), MASKED_LEVELS.ctypes.data_as(_vp)
    n = n_outer * n_lev
    Xd, Yd = far.x(fc.near_layout(n, S), F32, fld), far.y(fc.near_layout(n, D), F64)
    _lib.call("smm_group_apply", grp.handle, Xd.ptr, _lib.SMM_F32, n_lev * S, S, S, Yd.ptr, _lib.SMM_F64, n_lev * D, D, D,
              n_outer, n_lev, n_inner, lev_p, msk_p, AREA_MIN, SELL | flags, None)
    want = Yd.rows()
    fc.check_rows(want, ref.reshape(n, D), "smm_group_apply on the decoded field")
    if side == "y":
        ly, ld = fc.rows_layout(n_outer, D, inner=n_lev)
        s1 = ly.offsets[1] - ly.offsets[0]
        ys = (ld, s1, s1)
        assert ld * 1 >= P31 and ld * 2 >= P32
    else:
        ly, ys = fc.near_layout(n, D), (n_lev * D, D, D)
    Y = far.y(ly, F64)
    entry = "smm_group_apply_grib_na" if skipna else "smm_group_apply_grib"
    _lib.call(entry, grp.handle, _vp(xa.ptr), x_bytes, _rp(rows), _bp(bitmaps), Y.ptr, _lib.SMM_F64, *ys, n_outer, n_lev,
              n_inner, lev_p, msk_p, AREA_MIN, flags, None)
    same_bits(Y.rows(), want, f"{entry}, far {side}")
    fc.check_windows(Y.read, ly, 8, f"{entry}, far {side}")


# ------------------------------------------------------------------ B: smm_grib_pack

def _grib_pack(y_ptr, ldy, n_dst, enc, n_rows, out):
    rec = enc.records(n_rows)
    rows, bitmaps = np.zeros(n_rows, dtype=GRIB_ROW_DTYPE), np.zeros(n_rows, dtype=GRIB_BITMAP_DTYPE)
    _lib.call("smm_grib_pack", 0, _vp(y_ptr), ldy, n_dst, n_rows, ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)),
              _vp(out.ptr), out.nbytes, _rp(rows), _bp(bitmaps), None)
    return rows, bitmaps


def test_grib_pack_y_far(far):
    """5 rows of 300 cells on the far pitch of 2^30 + K float64 (row 2 past 2^31 elements, row 4 past 2^32) among
    decoys; out is near: the bytes and the records of `GribEncode.encode` on the host copy of the rows."""
    n_dst = 300
    lay, ldy = fc.rows_layout(5, n_dst)
    values, nbits, dec, kinds = pc.batch(n_dst, seed=13, passes=1)
    pick = [kinds.index(k) for k in ("full", "missing50", "ties", "one_last", "inf")]
    values, nbits, dec, kinds = values[pick], nbits[pick], dec[pick], [kinds[i] for i in pick]
    enc = GribEncode(nbits, dec)
    want = enc.encode(values)
    Y = far.x(lay, F64, values)
    out = sentinel_bytes(far, want.buf.size + fc.GUARD)
    rows, bitmaps = _grib_pack(Y.arr.ptr + lay.offsets[0] * 8, ldy, n_dst, enc, 5, out)
    host = out.to_host()
    check_packed(host, rows, bitmaps, want, kinds, "Y far")
    assert (host[want.buf.size:] == fc.SENTINEL).all()


def test_grib_pack_out_far(far):
    """1030 rows of 2^20 cells at 32 bits: slots of 4.2 MB back to back, 4.15 GiB in all.  Y (8.6 GB) is `fill_random`
    on the device with true values copied into the checked rows: row 0, the first row whose slot begins past 2^31 bytes,
    and the last two, past 2^32.  Their slots hold the bytes of `GribEncode.encode`, their records are its records moved to
    the slot; of every other row the record's place is smm_grib_out_layout's; 4096 bytes behind the layout keep 0x42."""
    n_dst, n_rows = 1 << 20, 1030
    enc = GribEncode(32)
    offs, total = enc.layout(n_dst, n_rows)
    lib_offs, lib_total = np.zeros(n_rows, np.uint64), ctypes.c_uint64(0)
    rec = enc.records(n_rows)
    _lib.call("smm_grib_out_layout", n_dst, ctypes.cast(rec.ctypes.data, ctypes.POINTER(_lib.GribEncodeStruct)), n_rows,
              lib_offs.ctypes.data_as(ctypes.POINTER(ctypes.c_uint64)), ctypes.byref(lib_total))
    assert np.array_equal(lib_offs, offs) and lib_total.value == total > P32
    slot = int(offs[1])
    checked = [0, int(np.argmax(offs >= P31)), n_rows - 2, n_rows - 1]
    assert offs[checked[1]] >= P31 > offs[checked[1] - 1] and offs[checked[2]] >= P32
    rng = np.random.default_rng([SEED, 30])
    true = rng.normal(250.0, 30.0, size=(len(checked), n_dst))
    true[1, rng.random(n_dst) < 0.3] = np.nan                       # a row with missing cells: its bitmap slot is used
    true[2, ::7] = np.inf
    want = GribEncode(32).encode(true)
    w_offs, _ = enc.layout(n_dst, len(checked))
    y = far.alloc(n_rows * n_dst, F64).fill_random(seed=5, mean=1000.0, sigma=50.0)
    for b, v in zip(checked, true):
        DeviceArray((n_dst,), F64, ptr=y.ptr + b * n_dst * 8, base=y).copy_from_host(v)
    out = sentinel_bytes(far, total + fc.GUARD)
    rows, bitmaps = _grib_pack(y.ptr, n_dst, n_dst, enc, n_rows, out)
    bm_bytes = fc._round4((n_dst + 7) // 8)
    assert np.array_equal(rows["byte_off"], offs + np.uint64(bm_bytes)), np.flatnonzero(rows["byte_off"] != offs + np.uint64(bm_bytes))[:4]
    others = np.setdiff1d(np.arange(n_rows), checked)
    assert (rows["nbits"][others] == 32).all() and (bitmaps["bitmap_off"][others] == GRIB_NO_BITMAP).all()
    assert (bitmaps["n_values"][others] == n_dst).all()
    for k, b in enumerate(checked):
        move = np.uint64(int(offs[b]) - int(w_offs[k]))
        wr, wb = want.rows[k:k + 1].copy(), want.bitmaps[k:k + 1].copy()
        wr["byte_off"] += move
        wb["bitmap_off"][wb["bitmap_off"] != GRIB_NO_BITMAP] += move
        assert rows[b].tobytes() == wr.tobytes() and bitmaps[b].tobytes() == wb.tobytes(), (b, rows[b], wr, bitmaps[b], wb)
    slots = [(int(offs[b]), want.buf[int(w_offs[k]):int(w_offs[k]) + slot]) for k, b in enumerate(checked)]
    fc.check_slots(reader(out), slots, total, out.nbytes, "smm_grib_pack, out far")


# ------------------------------------------------------------------ C: the four transcoders, input far

def far_streams(far, rows, seed):
    """rows: three far rows, the alias of the second, then the near rows, each with its `stream`.  Returns the layout
    and the device bytes (a uint8 view that covers x_bytes rounded up to a word)."""
    lay = fc.stream_layout([r.stream.size for r in rows[:3]], [r.stream.size for r in rows[4:]])
    assert rows[3].stream.size == rows[1].stream.size
    assert lay.far[0] > P31 and lay.far[1] > P32 and lay.far[1] % 2 == 1 and lay.far[2] > 1 << 34
    assert lay.alias == lay.far[1] % P32 and lay.x_bytes == lay.far[2] + rows[2].stream.size
    xa = decoy_bytes(far, lay.x_bytes, list(zip(lay.offsets(), (r.stream for r in rows))), seed)
    return lay, byte_view(xa)


def guarded_tail(out, used, what):
    host = out.to_host()
    assert used + fc.GUARD <= host.size
    bad = np.flatnonzero(host[used:] != fc.SENTINEL)
    assert bad.size == 0, f"{what}: byte {used + int(bad[0])} behind the {used} bytes used was written"


def test_cpx_unpack_input_far(far):
    """order2_noct3 past 2^31, order1_noct2 (odd, aliased) past 2^32, order0_widths_0_1_31_32 past 2^34 to the buffer's
    last word; the alias, short1500_order2 and n3_order2 near: every slot holds its simple-packed twin."""
    order = [xc.case(n) for n in ("order2_noct3", "order1_noct2", "order0_widths_0_1_31_32")]
    order += [fc.cpx_alias(order[1])] + [xc.case(n) for n in ("short1500_order2", "n3_order2")]
    lay, x = far_streams(far, order, seed=11)
    rows = cc.rules(len(order), seed=2)
    recs = np.zeros(len(order), dtype=GRIB_CPX_DTYPE)
    for i, (c, off) in enumerate(zip(order, lay.offsets())):
        rows["nbits"][i], recs[i] = c.params["nbits"], c.record(off)
    total = 4 * sum(c.n_values for c in order)
    out = sentinel_bytes(far, total + fc.GUARD)
    scratch(far, 16 * total)
    _, rows_out = grib_unpack_cpx(x, rows, recs, x_bytes=lay.x_bytes, out=out)
    assert t_cpx.check_unpacked(out.to_host(), rows, rows_out, order) == total
    guarded_tail(out, total, "smm_grib_cpx_unpack")


class _Stream:
    """A fixture with the `stream` attribute holding what lies in X for a packer: its simple-packed twin."""

    def __init__(self, case, twin):
        self.case, self.stream = case, twin


def test_aec_unpack_input_far(far):
    """Five fixtures of tests/golden/ccsds -- the preprocessor on and off, widths 12, 16 and 32 -- and the alias of
    grid_w32_extremes: every slot holds its simple-packed twin and decodes to the floats of the fixture's integers."""
    fxs = [cc.fixture(n) for n in ("grid_w12_noise_pp0", "grid_w32_extremes", "grid_w12_smooth")]
    fxs += [fc.aec_alias(fxs[1])] + [cc.fixture(n) for n in ("edge_n43_w32_pp0", "short_w16_smooth")]
    assert {bool(f.flags & cc.PREPROCESS) for f in fxs} == {True, False} and {12, 32} <= {f.nbits for f in fxs}
    lay, x = far_streams(far, fxs, seed=12)
    rows = cc.rules(len(fxs), seed=2)
    aec = np.zeros(len(fxs), dtype=GRIB_AEC_DTYPE)
    for i, (f, off) in enumerate(zip(fxs, lay.offsets())):
        rows["nbits"][i] = f.nbits
        aec[i] = (off, f.stream.size, f.n_values, f.nbits, f.block, f.rsi, f.flags, 0)
    total = sum(fc._round4((f.n_values * f.nbits + 7) // 8) for f in fxs)
    out = sentinel_bytes(far, total + fc.GUARD)
    _, rows_out = grib_unpack(x, rows, aec, x_bytes=lay.x_bytes, out=out)
    assert t_aec.check_unpacked(out.to_host(), rows, rows_out, fxs) == total
    guarded_tail(out, total, "smm_grib_aec_unpack")


def _cpx_pack_rows():
    """Rows of `every_case()` of 2048 values or fewer at orders 2, 1 and 0 (far) and two more (near), of 16, 12, 32, 30
    and 12 bits, with the group lengths `every_case` gives them; the alias row has the second one's integers reversed:
    the same width, order and group length."""
    pool = {(c.name, c.order): c for c in t_cpx_pack.every_case()}
    far_rows = [pool[k] for k in (("order2_noct3", 2), ("order1_noct2", 1), ("order0_widths_0_1_31_32", 0))]
    near = [pool[k] for k in (("order2_noct4", 2), ("short1500_order1", 1))]
    assert all(c.n_values <= 2048 for c in far_rows + near) and len({c.L for c in far_rows + near}) >= 3
    alias = t_cpx_pack.PackCase("alias_of_" + far_rows[1].name, far_rows[1].X[::-1], far_rows[1].order, far_rows[1].L,
                                nbits=far_rows[1].nbits)
    assert (alias.X != far_rows[1].X).any()
    return far_rows + [alias] + near


def test_cpx_pack_input_far(far):
    cases = _cpx_pack_rows()
    lay, x = far_streams(far, [_Stream(c, cc.pack_bits(c.X, c.nbits)) for c in cases], seed=13)
    rows, want = t_cpx_pack.pack_records(cases, lay.offsets())
    bound = _grib.CodedRows(_grib.CPX, want).bound()
    out = sentinel_bytes(far, bound + fc.GUARD)
    coded, rows_out, recs = grib_cpx_pack(x, rows, want, x_bytes=lay.x_bytes, out=out)
    assert coded.nbytes <= bound
    t_cpx_pack.check_against_host(cases, coded, rows_out, recs, coded.nbytes)
    guarded_tail(out, coded.nbytes, "smm_grib_cpx_pack")


def test_aec_pack_input_far(far):
    """The CCSDS twins: fixtures of 2048 values or fewer as simple-packed rows, coded with their own block size, interval
    and preprocessor switch; the alias row has the second one's integers reversed."""
    cases = [cc.fixture(n) for n in ("grid_w12_noise_pp0", "grid_w32_extremes", "grid_w12_smooth")]
    a = cases[1]
    alias = ec.Case("alias_of_" + a.name, a.values[::-1], a.nbits, a.block, a.rsi, a.flags & cc.PREPROCESS)
    alias.flags = a.flags
    assert (alias.values != a.values).any()
    cases += [alias] + [cc.fixture(n) for n in ("edge_n43_w32_pp0", "short_w16_smooth")]
    lay, x = far_streams(far, [_Stream(c, cc.pack_bits(c.values, c.nbits)) for c in cases], seed=14)
    rows, want = t_aec_pack.pack_records(cases, lay.offsets())
    bound = _grib.CodedRows(_grib.CCSDS, want).bound()
    out = sentinel_bytes(far, bound + fc.GUARD)
    coded, rows_out, recs = grib_aec_pack(x, rows, want, x_bytes=lay.x_bytes, out=out)
    assert coded.nbytes <= bound
    t_aec_pack.check_against_host(cases, coded, rows_out, recs, coded.nbytes)
    guarded_tail(out, coded.nbytes, "smm_grib_aec_pack")


# ------------------------------------------------------------------ D: the four transcoders, output (and scratch) far

SAMPLE = 1 << 20          # samples of the host encode that sizes the spacers
EDGE = 1024               # values checked at either end of a spacer
HEAD = 1 << 16            # bytes of X ahead of the spacers: A, B and C lie there
SPACER_SEED = 77


class Spacer:
    """A row of X's decoy bits taken as big-endian 32-bit samples from byte `off` on."""

    def __init__(self, off, n_values, **par):
        self.off, self.n_values, self.nbits = int(off), int(n_values), 32
        self.__dict__.update(par)

    def edges(self, read):
        """(first, last) EDGE samples, read back from X."""
        n = 4 * EDGE
        return tuple(np.frombuffer(read(s, s + n).tobytes(), ">u4").astype(np.uint32)
                     for s in (self.off, self.off + 4 * self.n_values - n))


def spacer_sample(far, off):
    """SAMPLE samples as a spacer at byte `off` of X holds them: `fill_random` gives element i from (seed, i) alone, so a
    small array filled with X's seed starts with X's bits."""
    n = off // 4 + SAMPLE + 2
    a = far.alloc(n, F32).fill_random(seed=SPACER_SEED, mean=1000.0, sigma=50.0)
    raw = a.to_host().view(U8)
    release(far, a)
    return np.frombuffer(raw[off:off + 4 * SAMPLE].tobytes(), ">u4").astype(np.uint32)


def spacer_values(bytes_per_value):
    """Values of spacers between A and B that put B a tenth past 2^31 bytes (and C, behind as many again, past 2^32)."""
    return int(1.1 * P31 / bytes_per_value)


def read_values(read, slot, first, count, width):
    """`count` integers of `width` bits from value `first` on of the simple-packed stream at byte `slot`."""
    bit = first * width
    raw = read(slot + bit // 8, slot + (bit + count * width + 7) // 8)
    bits = np.unpackbits(np.asarray(raw, dtype=U8))[bit % 8:bit % 8 + count * width].reshape(count, width).astype(np.uint64)
    return (bits << np.arange(width - 1, -1, -1, dtype=np.uint64)).sum(axis=1).astype(np.uint32)


def check_chain(recs, b, c, used, bound):
    """The conditions of an output-far case, on the records the packer returned."""
    off, length = recs["byte_off"].astype(np.int64), recs["byte_len"].astype(np.int64)
    assert off[b] >= P31 and off[c] >= P32, f"the case has not run: B at {off[b]}, C at {off[c]} bytes"
    assert off[0] == 0 and np.array_equal(off[1:], (off[:-1] + length[:-1] + 3) // 4 * 4)
    assert (off[-1] + length[-1] + 3) // 4 * 4 == used <= bound


def check_twin_slots(read, rows_back, idx, ints, widths, n_values_all, slot_bytes, out_size, what):
    """The true rows came back as their simple-packed twins at `widths`, in slots laid back to back."""
    offs = np.concatenate([[0], np.cumsum([slot_bytes(n, w) for n, w in n_values_all])])
    assert np.array_equal(rows_back["byte_off"].astype(np.int64), offs[:-1]), what
    slots = []
    for i, X, w in zip(idx, ints, widths):
        assert int(rows_back["nbits"][i]) == w, (what, i, int(rows_back["nbits"][i]), w)
        twin = cc.pack_bits(X, w)
        pad = np.zeros(fc._round4(twin.size), U8)
        pad[:twin.size] = twin
        slots.append((int(offs[i]), pad))
    fc.check_slots(read, slots, int(offs[-1]), out_size, what)
    return offs


def test_cpx_output_far(far):
    """smm_grib_cpx_pack of [A, spacer, B, spacer, C] -- A, B, C at orders 0, 1, 2 in groups of 8, 64, 32, the spacers at
    order 0 in groups of 64 -- then smm_grib_cpx_unpack of the coded buffer with the returned records: its input past
    2^32 bytes, its slots (4 bytes a value) past 2^32, its scratch (8 bytes a value) past 2^33."""
    true = [t_cpx_pack.PackCase(name, xc.case(name).X, order, L) for name, order, L in
            (("order0_widths_0_1_31_32", 0, 8), ("short1500_order1", 1, 64), ("order2_noct3", 2, 32))]
    offs_in, at = [], 3
    for c in true:
        offs_in.append(at)
        at += (c.n_values * c.nbits + 7) // 8 + 5
    assert at <= HEAD
    sample = spacer_sample(far, HEAD + 1)
    stream, _ = cpx_encode(sample, cpx_want(32, 0, 64))
    n_sp = spacer_values(stream.size / SAMPLE)
    assert n_sp < P31
    # both at an odd offset of the same residue mod 4: which byte of a float32 leads a sample decides how well it codes
    sp = [Spacer(HEAD + 1, n_sp, order=0, L=64), Spacer(HEAD + 1 + 4 * n_sp + 8, n_sp, order=0, L=64)]
    x_bytes = sp[1].off + 4 * n_sp + 8
    xa = decoy_bytes(far, x_bytes, [(o, cc.pack_bits(c.X, c.nbits)) for o, c in zip(offs_in, true)], seed=SPACER_SEED)
    assert np.array_equal(Spacer(HEAD + 1, SAMPLE).edges(reader(xa))[0], sample[:EDGE])
    cases = [true[0], sp[0], true[1], sp[1], true[2]]
    rows, want = t_cpx_pack.pack_records(cases, [offs_in[0], sp[0].off, offs_in[1], sp[1].off, offs_in[2]])
    bound = _grib.CodedRows(_grib.CPX, want).bound()
    out = sentinel_bytes(far, bound + fc.GUARD)
    scratch(far, (2 * (n_sp // 64 + 1) + 3 * 256) * 8 + (2 * (n_sp // 1024 + 1) + 6) * 12 + 4096)   # groups and tiles
    coded, rows_c, recs = grib_cpx_pack(byte_view(xa), rows, want, x_bytes=x_bytes, out=out)
    used = coded.nbytes
    check_chain(recs, 2, 4, used, bound)
    read = reader(out)
    slots = []
    for i in (0, 2, 4):
        st, rec = cases[i].host()
        rec = rec.copy()
        rec["byte_off"] = recs["byte_off"][i]
        assert recs[i].tobytes() == rec.tobytes(), (cases[i], recs[i], rec)
        pad = np.zeros(fc._round4(st.size), U8)
        pad[:st.size] = st
        slots.append((int(recs["byte_off"][i]), pad))
    fc.check_slots(read, slots, used, min(out.nbytes, used + (16 << 20)), "smm_grib_cpx_pack, out far")
    fc.check_guard(read, out.nbytes - fc.GUARD, out.nbytes, "smm_grib_cpx_pack, out far")
    for i in (1, 3):
        assert int(recs["order"][i]) == 0 and int(recs["n_values"][i]) == n_sp and int(recs["n_groups"][i]) == -(-n_sp // 64)
    edges = [s.edges(reader(xa)) for s in sp]
    release(far, xa)
    # the way back
    n_all = [c.n_values for c in cases]
    total = 4 * sum(n_all)
    assert 4 * (n_all[0] + n_sp) >= P31 and 4 * sum(n_all[:4]) >= P32 and 8 * sum(n_all[:4]) >= P33
    back = sentinel_bytes(far, total + fc.GUARD)
    scratch(far, 8 * sum(n_all) + 16 * int(recs["n_groups"].sum()) + (1 << 20))
    _, rows_b = grib_unpack_cpx(byte_view(out, 0, used), rows_c, recs, x_bytes=used, out=back)
    read = reader(back)
    widths = [xc.width_of(c.X) for c in true]
    offs = check_twin_slots(read, rows_b, (0, 2, 4), [c.X for c in true], widths, [(n, 32) for n in n_all],
                            lambda n, w: 4 * n, back.nbytes, "smm_grib_cpx_unpack, all far")
    for i, (first, last) in zip((1, 3), edges):
        w = int(rows_b["nbits"][i])
        assert 28 <= w <= 32, w
        assert (n_sp - EDGE) * w > P32                                 # a bit position past 2^32 inside one row
        got = read_values(read, int(offs[i]), 0, EDGE, w), read_values(read, int(offs[i]), n_sp - EDGE, EDGE, w)
        assert np.array_equal(got[0], first) and np.array_equal(got[1], last), f"spacer row {i}"


def test_aec_output_far(far):
    """The CCSDS road in the same shape.  The decoder's parse kernel walks a row's blocks serially, one wave a row, so a
    spacer is R rows of 2^24 samples (blocks of 64, an interval of 128 blocks, no preprocessor): [A, R spacers, B,
    R spacers, C].  smm_grib_aec_pack against the host encoder, smm_grib_aec_unpack of the coded buffer against the twins
    and the samples of X."""
    true = [cc.fixture(n) for n in ("grid_w12_noise_pp0", "grid_w32_extremes", "grid_w16_runs")]
    offs_in, at = [], 3
    for c in true:
        offs_in.append(at)
        at += (c.n_values * c.nbits + 7) // 8 + 5
    assert at <= HEAD
    n_sp, par = 1 << 24, dict(block=64, rsi=128, flags=0)
    sample = spacer_sample(far, HEAD + 2)
    stream = aec_encode(sample, cc.record(0, 0, 0, 32, 64, 128, 0))
    R = -(-spacer_values(stream.size / SAMPLE) // n_sp)
    assert 8 <= R <= 64, R
    sp = [Spacer(HEAD + 2 + k * (4 * n_sp + 4), n_sp, **par) for k in range(2 * R)]
    x_bytes = sp[-1].off + 4 * n_sp + 8
    xa = decoy_bytes(far, x_bytes, [(o, cc.pack_bits(c.values, c.nbits)) for o, c in zip(offs_in, true)], seed=SPACER_SEED)
    assert np.array_equal(Spacer(HEAD + 2, SAMPLE).edges(reader(xa))[0], sample[:EDGE])
    cases = [true[0]] + sp[:R] + [true[1]] + sp[R:] + [true[2]]
    ib, ic = R + 1, 2 * R + 2
    rows, want = t_aec_pack.pack_records(cases, [offs_in[0]] + [s.off for s in sp[:R]] + [offs_in[1]] + [s.off for s in sp[R:]]
                                         + [offs_in[2]])
    bound = _grib.CodedRows(_grib.CCSDS, want).bound()
    out = sentinel_bytes(far, bound + fc.GUARD)
    scratch(far, (2 * R * n_sp // 8 + 64) * 20 + (1 << 20))
    coded, rows_c, recs = grib_aec_pack(byte_view(xa), rows, want, x_bytes=x_bytes, out=out)
    used = coded.nbytes
    check_chain(recs, ib, ic, used, bound)
    read = reader(out)
    slots = []
    for i in (0, ib, ic):
        c, r = cases[i], recs[i]
        st = t_aec_pack.host_stream(c)
        assert (int(r["byte_len"]), int(r["n_values"]), int(r["nbits"]), int(r["block_size"]), int(r["rsi"]), int(r["flags"])) == \
            (st.size, c.n_values, c.nbits, c.block, c.rsi, c.flags), (c, r)
        pad = np.zeros(fc._round4(st.size), U8)
        pad[:st.size] = st
        slots.append((int(r["byte_off"]), pad))
    fc.check_slots(read, slots, used, min(out.nbytes, used + (16 << 20)), "smm_grib_aec_pack, out far")
    fc.check_guard(read, out.nbytes - fc.GUARD, out.nbytes, "smm_grib_aec_pack, out far")
    edges = [s.edges(reader(xa)) for s in sp]
    release(far, xa)
    # the way back
    n_all = [(c.n_values, c.nbits) for c in cases]
    slot_bytes = lambda n, w: fc._round4((n * w + 7) // 8)          # noqa: E731
    total = sum(slot_bytes(n, w) for n, w in n_all)
    back = sentinel_bytes(far, total + fc.GUARD)
    scratch(far, 4 * sum(n for n, _ in n_all) + (1 << 20))
    _, rows_b = grib_unpack(byte_view(out, 0, used), rows_c, recs, x_bytes=used, out=back)
    read = reader(back)
    offs = check_twin_slots(read, rows_b, (0, ib, ic), [c.values for c in true], [c.nbits for c in true], n_all, slot_bytes,
                            back.nbytes, "smm_grib_aec_unpack, all far")
    assert offs[ib] >= P31 and offs[ic] >= P32
    for i, (first, last) in zip(list(range(1, ib)) + list(range(ib + 1, ic)), edges):
        assert int(rows_b["nbits"][i]) == 32
        got = read_values(read, int(offs[i]), 0, EDGE, 32), read_values(read, int(offs[i]), n_sp - EDGE, EDGE, 32)
        assert np.array_equal(got[0], first) and np.array_equal(got[1], last), f"spacer row {i}"
