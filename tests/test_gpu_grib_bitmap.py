"""Bitmapped GRIB fields regridded raw (smm_apply_grib_bm, smm_apply_host_grib_bm, `Regridder(packed=True)` on a file
opened with decode=False, bitmaps=True): every result is compared bit for bit -- uint64 views, NaNs included -- with
smm_apply on the float32 field a host decode gives (SMM_F32 X, SMM_APPLY_KERNEL_SELL; NaN where the bitmap is 0), which
is itself checked against the oracle.  The fields are built from chosen integers and chosen bitmaps: each bitmapped
row's packed stream holds its present cells only, bitmaps and streams lie shuffled in one buffer at byte offsets of all
four residues with garbage between them, and the pad bits of a bitmap's last byte are set."""
import ctypes
import os
import re

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import (GRIB_BITMAP_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, CdoGenerate, GribField, Regridder,
                           SparseOperator, _lib, pinned_empty, to_device)
from smmregrid_amd.io import open_dataset
from tests import grib_cases
from tests.grib_cases import WIDTHS
from tests.test_gpu_grib import _OPS, device_bytes, expected, operator, same_arrays, same_bits
from tests.test_griblite import encode, encode2

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_bm(specs, rng, tail_residue=None, shuffle=True):
    """specs: one dict per batch row with q (an integer for EVERY cell), nbits, E, D, ref, residue (of its data), and
    bitmap: None, a bool array (its own bitmap, at byte residue bm_residue) or ("row", i) -- the bitmap of row i, shared.
    Only the present cells' integers are packed.  The pieces -- streams and bitmaps -- are laid into one buffer in
    shuffled order, each at the next offset with its residue, garbage between them; the last one laid ends exactly at
    the end of the buffer (tail_residue: the buffer length mod 4 wanted).  Returns (buf, rows, bitmaps, field) with the
    float32 field decoded from the chosen q, NaN where the bitmap is 0."""
    S = len(specs[0]["q"])
    pieces = []                                   # (kind, row, bytes, residue)
    masks = []
    for i, s in enumerate(specs):
        bm = s.get("bitmap")
        if isinstance(bm, tuple):
            bm = specs[bm[1]]["bitmap"]
        masks.append(None if bm is None else np.asarray(bm, bool))
    for i, s in enumerate(specs):
        q = np.asarray(s["q"], np.uint64)
        pieces.append(("data", i, grib_cases.pack_bits(q if masks[i] is None else q[masks[i]], s["nbits"]), s.get("residue", 0)))
        if masks[i] is not None and not isinstance(s["bitmap"], tuple):
            packed = np.packbits(masks[i].astype(np.uint8))
            if S % 8:
                packed[-1] |= 0xFF >> (S % 8)                    # pad bits beyond n_src: set, and never looked at
            pieces.append(("bitmap", i, packed.tobytes(), s.get("bm_residue", 0)))
    order = rng.permutation(len(pieces)) if shuffle else np.arange(len(pieces))
    if tail_residue is not None:                  # the piece laid last is not an empty one: it ends at the buffer's end
        nonempty = [k for k in order if len(pieces[k][2])]
        order = [k for k in order if k != nonempty[-1]] + [nonempty[-1]]
    rows = np.zeros(len(specs), dtype=GRIB_ROW_DTYPE)
    bitmaps = np.zeros(len(specs), dtype=GRIB_BITMAP_DTYPE)
    bitmaps["bitmap_off"] = GRIB_NO_BITMAP
    chunks, pos = [], 0
    for n, k in enumerate(order):
        kind, i, data, want = pieces[k]
        want %= 4
        if n == len(order) - 1 and tail_residue is not None:
            want = (tail_residue - len(data)) % 4
        gap = (want - pos) % 4 + 4 * int(rng.integers(0, 2))
        chunks.append(bytes(rng.integers(0, 256, size=gap, dtype=np.uint8).tolist()))
        pos += gap
        if kind == "data":
            s = specs[i]
            rows[i] = (pos, s["ref"], 2.0 ** s["E"], 10.0 ** s["D"], s["nbits"], 0)
        else:
            bitmaps["bitmap_off"][i] = pos
        chunks.append(data)
        pos += len(data)
    for i, s in enumerate(specs):
        if isinstance(s.get("bitmap"), tuple):
            bitmaps["bitmap_off"][i] = bitmaps["bitmap_off"][s["bitmap"][1]]
        bitmaps["n_values"][i] = S if masks[i] is None else int(masks[i].sum())
    buf = np.frombuffer(b"".join(chunks), dtype=np.uint8).copy()
    field = np.stack([grib_cases.decode_ref(s["q"], s["ref"], s["E"], s["D"]) for s in specs])
    for i, m in enumerate(masks):
        if m is not None:
            field[i, ~m] = np.float32(np.nan)
    return buf, rows, bitmaps, field


def random_bitmaps(rng, specs, S, residues=(0, 1, 2, 3)):
    """every row its own random bitmap at its own density, the bitmaps' byte residues cycling through all four"""
    for b, s in enumerate(specs):
        s["bitmap"] = rng.random(S) < rng.uniform(0.05, 0.95)
        s["bm_residue"] = residues[(b + 1) % len(residues)]
    return specs


def expected_bm(name, field, masked=False, area_min=0.0, no_fill=False):
    """`expected` of tests/test_gpu_grib.py with SMM_APPLY_NO_FILL at choice"""
    if not no_fill:
        return expected(name, field, masked, area_min)
    op, csr, imask, frac = operator(name)
    want = op.apply(to_device(field), masked=masked, remap_area_min=area_min,
                    flags=_lib.APPLY_KERNEL_SELL | _lib.APPLY_NO_FILL).to_host()
    ref = oracle.apply_c(csr, field, masked=masked, dst_imask=imask, dst_frac=frac, area_min=area_min, fill=False)
    assert np.array_equal(np.isnan(want), np.isnan(ref)) and np.array_equal(want[~np.isnan(ref)], ref[~np.isnan(ref)])
    return want


def run_bm(name, buf, rows, bitmaps, masked=False, area_min=0.0, flags=0):
    op = operator(name)[0]
    return op.apply_grib(device_bytes(buf), rows, x_bytes=buf.size, masked=masked, remap_area_min=area_min, flags=flags,
                         bitmaps=bitmaps).to_host()


def check_all(name, buf, rows, bitmaps, field, what):
    for masked, area_min in ((False, 0.0), (True, 0.5)):
        same_bits(run_bm(name, buf, rows, bitmaps, masked, area_min), expected_bm(name, field, masked, area_min),
                  f"{what} masked={masked} area_min={area_min}")


# ---------------------------------------------------------------------------------------------- 1: widths and residues

@pytest.mark.parametrize("nbits", (0, 1, 12, 16, 25, 32))
@pytest.mark.parametrize("name", ["bil_r180x90_r90x45", "ragged_random", "tiny"])
def test_bitmapped_rows_match_apply_on_the_decoded_field(hip, name, nbits):
    assert nbits in WIDTHS
    rng = np.random.default_rng(2000 + nbits)
    S = operator(name)[0].n_src
    seen = set()
    for n_batch in (1, 5, 9):
        specs = grib_cases.row_specs(rng, S, n_batch, (nbits,), D=(0,) if n_batch == 1 else (0, 2, -1))
        random_bitmaps(rng, specs, S, residues=(n_batch % 4, 1, 2, 3, 0))
        buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=1 + n_batch % 3)
        assert buf.size % 4 != 0 and np.isnan(field).any() and (bitmaps["bitmap_off"] != GRIB_NO_BITMAP).all()
        seen |= set((bitmaps["bitmap_off"] % 4).tolist())
        check_all(name, buf, rows, bitmaps, field, f"{name} nbits={nbits} B={n_batch}")
    assert seen == {0, 1, 2, 3}


# ---------------------------------------------------------------------------------------------- 2: edge bitmaps

def edge_case(name, rng):
    S = operator(name)[0].n_src
    assert S > 96
    ones, zeros = np.ones(S, bool), np.zeros(S, bool)
    first, last, hole = zeros.copy(), zeros.copy(), ones.copy()
    first[0], last[-1] = True, True
    hole[32:64] = False                                        # one whole block missing between two full ones
    some = rng.random(S) < 0.6
    specs = grib_cases.row_specs(rng, S, 9, (16, 12, 7, 25, 16, 12, 17, 24, 0), D=(0, 0, 1))
    for s, bm in zip(specs, (ones, zeros, first, last, hole, None, some, ("row", 6), some.copy())):
        s["bitmap"] = bm
    for b, s in enumerate(specs):
        s["bm_residue"] = b % 4
    return specs


@pytest.mark.parametrize("name", ["bil_r180x90_r90x45", "ragged_random"])
def test_edge_bitmaps_in_one_call(hip, name):
    """all present, all missing (no data byte), only the first / only the last cell, one whole block missing, a row
    without a bitmap, two rows on one bitmap_off, a constant (0-bit) row with a bitmap.  The all-missing row is NaN
    wherever a destination row has links under SMM_APPLY_NO_FILL (w * NaN); with the fill on, where the filled sum
    passes 1e19 -- which the decoded road decides, bit for bit."""
    rng = np.random.default_rng(21)
    specs = edge_case(name, rng)
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=3)
    S = len(specs[0]["q"])
    assert bitmaps["n_values"].tolist()[:6] == [S, 0, 1, 1, S - 32, S] and bitmaps["bitmap_off"][5] == GRIB_NO_BITMAP
    assert bitmaps["bitmap_off"][6] == bitmaps["bitmap_off"][7] and rows["nbits"][8] == 0 and np.isnan(field[8]).any()
    assert np.isnan(field[1]).all()
    check_all(name, buf, rows, bitmaps, field, f"{name} edges")
    op = operator(name)[0]
    z = np.load(os.path.join(ROOT, "tests", "golden", name + ".npz"))
    linked = np.zeros(op.n_dst, bool)
    linked[z["dst_address"] - 1] = True
    for flags, no_fill in ((0, False), (_lib.APPLY_NO_FILL, True)):
        got = run_bm(name, buf, rows, bitmaps, flags=flags)
        want = expected_bm(name, field, no_fill=no_fill)
        same_bits(got, want, f"{name} edges no_fill={no_fill}")
        # the all-missing row: NaN wherever a destination row has links
        assert np.isnan(got[1]).any() and np.array_equal(np.isnan(got[1]), np.isnan(want[1]))
        if no_fill:
            assert linked.any() and np.isnan(got[1][linked]).all()
    # the all-present row has the bits of the no-bitmap call on the same integers
    plain = op.apply_grib(device_bytes(buf), rows[[0, 5]], x_bytes=buf.size).to_host()
    same_bits(run_bm(name, buf, rows, bitmaps)[[0, 5]], plain, "all present == no bitmap")
    # a table of records without one bitmap runs the plain gather
    none = np.zeros(2, GRIB_BITMAP_DTYPE)
    none["bitmap_off"], none["n_values"] = GRIB_NO_BITMAP, S
    same_bits(run_bm(name, buf, rows[[0, 5]], none), plain, "records without a bitmap")


# ---------------------------------------------------------------------------------------------- 3: the scan across segments

def segment_cells():
    with open(os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_grib_codec.hpp")) as fh:
        m = re.search(r"constexpr\s+int\s+kGribSegBlocks\s*=\s*(\d+)\s*;", fh.read())
    assert m, "the segment constant of the table build"
    return 32 * int(m.group(1))


def segments_operator():
    if "segments" not in _OPS:
        seg = segment_cells()
        n_src, n_dst = 3 * seg + 1000 + 13, 320
        assert n_src % 32 and n_src // seg >= 3
        rng = np.random.default_rng(33)
        cells = {0, n_src - 1, n_src - 2, 31, 32, 33}
        for k in range(1, 4):                                   # either side of every segment boundary
            cells |= {k * seg - 2, k * seg - 1, k * seg, k * seg + 1}
        for sub in (seg // 4, seg // 256):                      # a wave's share, a thread's share of a segment
            ks = np.arange(1, n_src // sub + 1)
            for k in rng.choice(ks, size=min(40, ks.size), replace=False):
                cells |= {int(k) * sub - 1, int(k) * sub}
        cells = sorted(c for c in cells if 0 <= c < n_src)
        src = np.concatenate([cells, rng.integers(0, n_src, size=3 * n_dst - len(cells))]) + 1
        assert len(cells) < 3 * n_dst
        dst = np.repeat(np.arange(1, n_dst + 1), 3)
        w = rng.random(src.size)
        op = SparseOperator(n_src, n_dst, src, dst, w, device=0)
        imask, frac = (rng.random(n_dst) > 0.2).astype(np.int32), rng.random(n_dst)
        op.set_epilogue(imask, frac)
        _OPS["segments"] = (op, oracle.coo_to_csr_c(n_src, n_dst, src, dst, w), imask, frac)
    return _OPS["segments"]


def test_the_rank_scan_across_segments(hip):
    """n_src spans three segments of the table build and a ragged tail; the links sit on the first and the last cell and
    on either side of every segment, wave and thread boundary; the bitmaps have dense and empty stretches.  B = 5: the
    4-rows-per-thread tail runs."""
    op = segments_operator()[0]
    S, seg = op.n_src, segment_cells()
    rng = np.random.default_rng(34)
    specs = grib_cases.row_specs(rng, S, 5, (12, 16, 7, 25, 16), D=(0, 1))
    for b, s in enumerate(specs):
        bm = rng.random(S) < (0.5, 0.9, 0.1, 0.7, 0.3)[b]
        bm[:20000] = True                                       # dense, then empty, stretches -- one across a boundary
        bm[20000:40000] = False
        bm[seg - 100:seg + 5000] = b % 2 == 0
        bm[2 * seg + 64:2 * seg + 4096] = b % 2 == 1
        s["bitmap"], s["bm_residue"] = bm, (b + 1) % 4
    specs[3]["bitmap"] = None
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=2)
    assert (bitmaps["n_values"][[0, 1]] > seg).all() and bitmaps["bitmap_off"][3] == GRIB_NO_BITMAP
    check_all("segments", buf, rows, bitmaps, field, "segments")


# ---------------------------------------------------------------------------------------------- 4: host entry

def host_case():
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(40)
    S = operator(name)[0].n_src
    specs = grib_cases.row_specs(rng, S, 7, (16, 12, 0, 24, 17, 7, 32), D=(0, 1))
    random_bitmaps(rng, specs, S)
    specs[1]["bitmap"] = None
    specs[5]["bitmap"] = ("row", 4)                             # shares row 4's bitmap: staged twice
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=1)
    return name, buf, rows, bitmaps, field


def staged_bytes_bm(rows, bitmaps, S):
    total = 0
    for r, b in zip(rows, bitmaps):
        has = int(b["bitmap_off"]) != GRIB_NO_BITMAP
        n = int(b["n_values"]) if has else S
        total += 40 + 16 + ((n * int(r["nbits"]) + 7) // 8 + 3) // 4 * 4 + (((S + 7) // 8 + 3) // 4 * 4 if has else 0)
    return total


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("chunk_rows", [0, 1, 3])
def test_apply_host_grib_bm_has_the_bits_of_the_device_entry(hip, pinned, chunk_rows):
    name, buf, rows, bitmaps, field = host_case()
    op = operator(name)[0]
    S, D = op.n_src, op.n_dst
    x_host = buf
    if pinned:
        x_host = pinned_empty(buf.size, np.uint8)
        x_host[:] = buf
    want = run_bm(name, buf, rows, bitmaps, True, 0.5)
    same_bits(want, expected_bm(name, field, True, 0.5), "device entry")
    _lib.host_stats(reset=True)
    got = op.apply_host_grib(x_host, rows, masked=True, remap_area_min=0.5, chunk_rows=chunk_rows, bitmaps=bitmaps)
    st = _lib.host_stats(reset=True)
    same_bits(got, want, f"host entry pinned={pinned} chunk_rows={chunk_rows}")
    assert st["calls"] == 1 and st["chunks"] == {0: 1, 1: 7, 3: 3}[chunk_rows]
    assert st["h2d_bytes"] == staged_bytes_bm(rows, bitmaps, S) and st["d2h_bytes"] == 7 * D * 8
    for y in (np.full((7, D + 3), -1.0), pinned_empty((7, D + 3), np.float64)):
        y[:] = -1.0
        _lib.call("smm_apply_host_grib_bm", op.handle, x_host.ctypes.data, buf.size,
                  ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct)),
                  ctypes.cast(bitmaps.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct)), y.ctypes.data, _lib.SMM_F64,
                  D + 3, 7, 0.5, _lib.APPLY_MASKED, chunk_rows)
        same_bits(np.ascontiguousarray(y[:, :D]), want, "ldy > D")
        assert (y[:, D:] == -1.0).all()


def test_a_failed_chunk_drains_and_the_next_bm_call_succeeds(hip):
    name, buf, rows, bitmaps, field = host_case()
    op = operator(name)[0]
    want = expected_bm(name, field)
    _lib.call("smm_debug_fail_at_chunk", 1)
    try:
        with pytest.raises(_lib.SmmError, match="injected failure"):
            op.apply_host_grib(buf, rows, chunk_rows=3, bitmaps=bitmaps)
    finally:
        _lib.call("smm_debug_fail_at_chunk", -1)
    same_bits(op.apply_host_grib(buf, rows, chunk_rows=3, bitmaps=bitmaps), want, "after the injected failure")


# ---------------------------------------------------------------------------------------------- 5: both instantiations

def test_both_division_instantiations_with_a_bitmap(hip):
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(50)
    S = operator(name)[0].n_src
    specs = random_bitmaps(rng, grib_cases.row_specs(rng, S, 6, (16, 12, 25), D=(0,)), S)
    buf, rows, bitmaps, field = build_bm(specs, rng)
    assert (rows["ddiv"] == 1.0).all()
    nodiv = run_bm(name, buf, rows, bitmaps)
    same_bits(nodiv, expected_bm(name, field), "DIV = false")
    mixed = [dict(s, D=(0, 2, 0, -1, 0, 0)[i]) for i, s in enumerate(specs)]
    buf2, rows2, bitmaps2, field2 = build_bm(mixed, rng)
    assert set(rows2["ddiv"].tolist()) == {1.0, 100.0, 0.1}
    div = run_bm(name, buf2, rows2, bitmaps2)
    same_bits(div, expected_bm(name, field2), "DIV = true")
    same_bits(div[[0, 2, 4, 5]], nodiv[[0, 2, 4, 5]], "rows with D = 0 under either instantiation")


# ---------------------------------------------------------------------------------------------- 6: refusals

def test_bm_refusals_that_need_the_operator(hip):
    op = operator("tiny")[0]
    S = op.n_src
    rng = np.random.default_rng(60)
    specs = random_bitmaps(rng, grib_cases.row_specs(rng, S, 2, (12,)), S)
    lib = _lib.load()

    def case(last):
        """the buffer with the piece of kind `last` laid last: it ends exactly at x_bytes"""
        for seed in range(200):
            buf, rows, bitmaps, field = build_bm(specs, np.random.default_rng(seed), tail_residue=1)
            ends = {"bitmap": (bitmaps["bitmap_off"] + (S + 7) // 8).max(),
                    "data": (rows["byte_off"] + (bitmaps["n_values"] * 12 + 7) // 8).max()}
            if ends[last] == buf.size and ends["bitmap" if last == "data" else "data"] < buf.size:
                return buf, rows, bitmaps, field
        raise AssertionError("no layout found")

    for last, word in (("bitmap", b"bitmap bytes"), ("data", b"]: bytes [")):
        buf, rows, bitmaps, field = case(last)
        x, y = device_bytes(buf), np.zeros((2, op.n_dst))
        yd = to_device(y)
        rp = ctypes.cast(rows.ctypes.data, ctypes.POINTER(_lib.GribRowStruct))

        def bp(b):
            return ctypes.cast(b.ctypes.data, ctypes.POINTER(_lib.GribBitmapStruct))

        def device(x_bytes, ldy, handle=op.handle, b=bitmaps):
            return lib.smm_apply_grib_bm(handle, ctypes.c_void_p(x.ptr), x_bytes, rp, bp(b), ctypes.c_void_p(yd.ptr),
                                         _lib.SMM_F64, ldy, 2, 0.0, 0, None)

        def host(x_bytes, ldy, handle=op.handle, b=bitmaps):
            return lib.smm_apply_host_grib_bm(handle, buf.ctypes.data, x_bytes, rp, bp(b), y.ctypes.data, _lib.SMM_F64, ldy,
                                              2, 0.0, 0, 0)

        too_many = bitmaps.copy()
        too_many["n_values"][1] = S + 1
        for fn in (device, host):
            # the piece laid last ends exactly at x_bytes: one byte less and it leaves the buffer
            assert fn(buf.size - 1, op.n_dst) == _lib.SMM_ERR_INVALID
            assert b"leave the buffer" in lib.smm_last_error() and word in lib.smm_last_error(), lib.smm_last_error()
            assert fn(buf.size, op.n_dst, b=too_many) == _lib.SMM_ERR_INVALID and b"n_values" in lib.smm_last_error()
            assert fn(buf.size, op.n_dst - 1) == _lib.SMM_ERR_INVALID and b"ldy" in lib.smm_last_error()
            assert fn(buf.size, op.n_dst, None) == _lib.SMM_ERR_INVALID and b"null operator" in lib.smm_last_error()
            assert fn(buf.size, op.n_dst) == _lib.SMM_OK
        same_bits(y, yd.to_host(), "host and device entry")
        same_bits(y, expected_bm("tiny", field), "the good call")


# ---------------------------------------------------------------------------------------------- 7: Regridder

def grib1_sst(tmp_path, rng):
    ni, nj = 36, 18
    grid = (0, ni, nj, 85, 0, -85, 350, 10000)
    lat = 85.0 - 10.0 * np.arange(nj)
    sea = rng.random((nj, ni)) > 0.3
    msgs = []
    for day in (1, 2, 3):
        sst = 285.0 + 10.0 * np.cos(np.radians(lat))[:, None] + rng.standard_normal((nj, ni)) + day
        msgs.append(encode(sst, *grid, param=34, date=(2021, 3, day, 12), nbits=12, bitmap=sea))
        msgs.append(encode(sst - 10.0, *grid, param=167, date=(2021, 3, day, 12), nbits=16))
    path = tmp_path / "sst.grib"
    path.write_bytes(b"".join(msgs))
    return str(path), "sst", "t2m"


def grib2_sst(tmp_path, rng):
    ni, nj = 36, 18
    grid = dict(template=0, ni=ni, nj=nj, la1=85.0, lo1=0.0, la2=-85.0, lo2=350.0, n_or_dj=10000000)
    sea = rng.random((nj, ni)) > 0.3
    msgs = []
    for step in (0, 6):
        msgs.append(encode2([dict(values=285.0 + 5 * rng.random((nj, ni)), category=3, number=0, bitmap=sea, nbits=14,
                                  decimal=1, step=step)], discipline=10, **grid))
        msgs.append(encode2([dict(values=280.0 + rng.standard_normal((nj, ni)), category=0, number=0, surface=(103, 2),
                                  nbits=17, step=step)], **grid))
    path = tmp_path / "sst.grib2"
    path.write_bytes(b"".join(msgs))
    return str(path), "sst", "t2m"


@pytest.mark.parametrize("make", [grib1_sst, grib2_sst])
def test_regridder_ships_a_bitmapped_variable_raw(hip, tmp_path, caplog, monkeypatch, make):
    path, var, plain = make(tmp_path, np.random.default_rng(70))
    dec, raw = open_dataset(path), open_dataset(path, decode=False, bitmaps=True)
    f = raw[var].data
    assert isinstance(f, GribField) and f.bitmaps is not None and isinstance(raw[plain].data, GribField)
    assert raw[plain].data.bitmaps is None and np.isnan(dec[var].values).any()
    S = 36 * 18
    # conservative weights on the decoded field: the source mask follows the NaNs
    w = CdoGenerate(dec[var], "r12x6").weights(method="con")
    want = Regridder(weights=w).regrid(dec)
    caplog.clear()
    assert want[var].dtype == np.float64 and np.isfinite(want[var].values).any()
    names = []
    real = _lib.call
    monkeypatch.setattr(_lib, "call", lambda name, *a: names.append(name) or real(name, *a))
    _lib.host_stats(reset=True)
    with caplog.at_level("INFO"):
        got = Regridder(weights=w, packed=True, loglevel="INFO").regrid(raw)
    st = _lib.host_stats(reset=True)
    assert not any("decoded on the host" in r.getMessage() or r.levelname == "WARNING" for r in caplog.records)
    assert names.count("smm_apply_host_grib_bm") == 1 and names.count("smm_apply_host_grib") == 1      # one per variable
    rows_plain = raw[plain].data.rows
    plain_bytes = int(sum(40 + ((S * int(n) + 7) // 8 + 3) // 4 * 4 for n in rows_plain["nbits"]))
    assert st["calls"] == 2 and st["h2d_bytes"] == staged_bytes_bm(f.rows, f.bitmaps, S) + plain_bytes
    assert list(got.data_vars) == list(want.data_vars) and got.attrs == want.attrs
    same_arrays(got[var], want[var], "packed=True on the bitmapped variable")
    same_arrays(got[plain], want[plain], "packed=True on the plain variable beside it")
    # bilinear weights without a mask: the missing cells poison their neighbours, as on the decoded road
    wb = CdoGenerate(dec[plain], "r12x6").weights(method="bil")
    want_b = Regridder(weights=wb).regrid(dec[var])
    got_b = Regridder(weights=wb, packed=True).regrid(raw[var])
    assert np.isnan(want_b.values).any() and np.isfinite(want_b.values).any()
    same_arrays(got_b, want_b, "bilinear, NaN-poisoned")
    # the fallbacks decode on the host with one INFO line each and give the bits of the decoded road
    for kw, word in ((dict(skipna=True), "skipna"), (dict(out_dtype=np.float32), "out_dtype float32")):
        caplog.clear()
        with caplog.at_level("INFO"):
            fb = Regridder(weights=w, packed=True, loglevel="INFO", **kw).regrid(raw[var])
        lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
        assert len(lines) == 1 and word in lines[0], lines
        ref = Regridder(weights=w, **kw).regrid(dec[var])
        assert fb.dtype == ref.dtype and np.array_equal(fb.values.view(np.uint8), ref.values.view(np.uint8)), word


def test_regridder_masked_levels_decode_a_bitmapped_variable_on_the_host(hip, tmp_path, caplog):
    ni, nj = 36, 18
    rng = np.random.default_rng(71)
    grid = dict(template=0, ni=ni, nj=nj, la1=85.0, lo1=0.0, la2=-85.0, lo2=350.0, n_or_dj=10000000)
    msgs = [encode2([dict(values=220.0 + 30 * rng.random((nj, ni)) + lev / 1e4, category=0, number=0, surface=(100, lev),
                          nbits=12, decimal=1, step=step, bitmap=rng.random((nj, ni)) > (0.2 if lev == 85000 else 0.4))
                     for lev in (85000, 50000)], **grid) for step in (0, 6)]
    path = tmp_path / "t.grib2"
    path.write_bytes(b"".join(msgs))
    dec, raw = open_dataset(str(path)), open_dataset(str(path), decode=False, bitmaps=True)
    assert isinstance(raw["t"].data, GribField) and raw["t"].data.bitmaps is not None
    w3 = CdoGenerate(dec["t"], "r12x6").weights(method="con", mask_dim="isobaricInhPa")
    want = Regridder(weights=w3).regrid(dec["t"])
    caplog.clear()
    with caplog.at_level("INFO"):
        got = Regridder(weights=w3, packed=True, loglevel="INFO").regrid(raw["t"])
    lines = [r.getMessage() for r in caplog.records if "is decoded on the host" in r.getMessage()]
    assert len(lines) == 1 and "masked levels" in lines[0]
    same_arrays(got, want, "masked levels")


# ---------------------------------------------------------------------------------------------- 8: no cross-talk

def test_the_old_entry_keeps_its_bits_between_bm_calls(hip):
    from smmregrid_amd.device import Stream
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(80)
    op = operator(name)[0]
    S = op.n_src
    pbuf, prows, pfield = grib_cases.build(grib_cases.row_specs(rng, S, 9, (16, 12, 7)), rng)
    specs = random_bitmaps(rng, grib_cases.row_specs(rng, S, 5, (12, 16, 25)), S)
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=3)
    want_plain, want_bm = expected(name, pfield), expected_bm(name, field)
    px, x = device_bytes(pbuf), device_bytes(buf)
    stream = Stream()
    ys = []
    for _ in range(2):
        ys.append((op.apply_grib(px, prows, x_bytes=pbuf.size, stream=stream), want_plain))
        ys.append((op.apply_grib(x, rows, x_bytes=buf.size, stream=stream, bitmaps=bitmaps), want_bm))
    ys.append((op.apply_grib(px, prows, x_bytes=pbuf.size, stream=stream), want_plain))
    stream.synchronize()
    for i, (y, want) in enumerate(ys):
        same_bits(y.to_host(), want, f"interleaved call {i}")


# ---------------------------------------------------------------------------------------------- 9: the batch split

def test_a_small_grid_limit_cuts_the_batch(hip):
    """4050 destination cells are 16 destination blocks, 9 rows at 4 rows per thread 3 batch tiles: 48 workgroups.  A limit
    of 20 cuts the 9 rows into parts of 2, 1, 2 and 4 rows, 16 leaves one batch tile per launch, and 15 is below the 16
    destination blocks of a single row.  The host entry cuts each chunk's launch alike: chunk_rows=4 gives chunks that
    fit as they are, chunk_rows=0 one chunk of all 9 rows.  Once with bitmaps (the BM gather and its rank tables, whose
    records move with the parts), once without (the plain gather)."""
    name = "bil_r180x90_r90x45"
    rng = np.random.default_rng(90)
    op = operator(name)[0]
    S = op.n_src
    assert (op.n_dst + 255) // 256 == 16
    specs = random_bitmaps(rng, grib_cases.row_specs(rng, S, 9, (16, 12, 7, 25, 0, 32, 17), D=(0, 1)), S)
    for b in (1, 4, 6):
        specs[b]["bitmap"] = None
    buf, rows, bitmaps, field = build_bm(specs, rng, tail_residue=3)
    pbuf, prows, pfield = grib_cases.build(grib_cases.row_specs(rng, S, 9, (16, 12, 7, 24), D=(0, 2)), rng)
    assert sorted(np.flatnonzero(bitmaps["bitmap_off"] == GRIB_NO_BITMAP).tolist()) == [1, 4, 6]
    kw = dict(masked=True, remap_area_min=0.5)
    cases = []
    for b, r, bm, f in ((buf, rows, bitmaps, field), (pbuf, prows, None, pfield)):
        x = device_bytes(b)
        want = op.apply_grib(x, r, x_bytes=b.size, bitmaps=bm, **kw).to_host()   # the unlimited run of the same call
        same_bits(want, expected_bm(name, f, True, 0.5), "no limit")
        cases.append((b, x, r, bm, want))
    try:
        for limit in (20, 16):
            _lib.call("smm_debug_set_grid_limit", limit)
            for b, x, r, bm, want in cases:
                what = f"grid limit {limit}, bitmaps={bm is not None}"
                same_bits(op.apply_grib(x, r, x_bytes=b.size, bitmaps=bm, **kw).to_host(), want, what)
                for chunk_rows in (4, 0):
                    same_bits(op.apply_host_grib(b, r, chunk_rows=chunk_rows, bitmaps=bm, **kw), want,
                              f"{what}, host chunk_rows={chunk_rows}")
        _lib.call("smm_debug_set_grid_limit", 15)
        for b, x, r, bm, want in cases:
            with pytest.raises(_lib.SmmError, match="launch grid beyond 15 workgroups") as err:
                op.apply_grib(x, r, x_bytes=b.size, bitmaps=bm, **kw)
            assert err.value.code == _lib.SMM_ERR_INVALID
    finally:
        _lib.call("smm_debug_set_grid_limit", 0)
    for b, x, r, bm, want in cases:
        same_bits(op.apply_grib(x, r, x_bytes=b.size, bitmaps=bm, **kw).to_host(), want, "limit restored")
