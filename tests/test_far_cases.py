"""tests/far_cases.py catches what it is for: at modulus 2^12 a numpy stand-in for an apply has its read offsets, or
its write offsets, narrowed in each of the four ways, in every layout the GPU test uses; the decoy / sentinel checks
must fail for each of them and pass for the stand-in that narrows nothing.  The byte-stream section does the same for
the GRIB transcoders' buffers: the library's host decoders read every row at each narrowed byte offset, and a stand-in
writes slots at narrowed output offsets."""
import numpy as np
import pytest

from tests import far_cases as fc

M, G = 1 << 12, 8
DTYPES = {"f16": np.float16, "f32": np.float32, "f64": np.float64}
B, S = 3, 25                                   # the stand-in's batch rows and source cells; D = S - 1


def _layouts(name):
    """(X layout, Y layout, x_off (B, S), y_off (B, D)): element offsets of every cell the stand-in touches."""
    D = S - 1
    b, s, d = np.arange(B)[:, None], np.arange(S)[None, :], np.arange(D)[None, :]
    if name == "row-major":                    # 5 batch rows on a far pitch, X and Y
        lx, ly = fc.rows_layout(5, S, M, G)[0], fc.rows_layout(5, D, M, G)[0]
        bb = np.arange(5)[:, None]
        return lx, ly, np.asarray(lx.offsets)[bb] + s, np.asarray(ly.offsets)[bb] + d
    if name == "batch-fastest":                # X (S, ldx), Y (D, ldy): the batch entries of a cell are contiguous
        lx, ly = fc.rows_layout(S, B, M, G)[0], fc.rows_layout(D, B, M, G)[0]
        return lx, ly, np.asarray(lx.offsets)[s] + b, np.asarray(ly.offsets)[d] + b
    if name == "batch-fastest-x":              # X (S, ldx), Y (B, ldy) as smm_apply_sb writes it by default
        lx, ly = fc.rows_layout(S, B, M, G)[0], fc.rows_layout(B, D, M, G)[0]
        return lx, ly, np.asarray(lx.offsets)[s] + b, np.asarray(ly.offsets)[b] + d
    if name == "levels":                       # 3 far levels of 2 near rows each
        lx, ly = fc.rows_layout(3, S, M, G, inner=2)[0], fc.rows_layout(3, D, M, G, inner=2)[0]
        bb = np.arange(6)[:, None]
        return lx, ly, np.asarray(lx.offsets)[bb] + s, np.asarray(ly.offsets)[bb] + d
    if name == "grad-rows":                    # G of smm_gradients: 3 far batch rows of 3 near planes each
        lx, ly = fc.rows_layout(3, S, M, G, inner=3)[0], fc.rows_layout(3, D, M, G, inner=3)[0]
        bb = np.arange(9)[:, None]
        return lx, ly, np.asarray(lx.offsets)[bb] + s, np.asarray(ly.offsets)[bb] + d
    if name == "grad-planes":                  # ... and one batch row whose 3 planes lie far apart
        lx, ly = fc.rows_layout(3, S, M, G)[0], fc.rows_layout(3, D, M, G)[0]
        bb = np.arange(3)[:, None]
        return lx, ly, np.asarray(lx.offsets)[bb] + s, np.asarray(ly.offsets)[bb] + d
    raise KeyError(name)


LAYOUTS = ("row-major", "batch-fastest", "batch-fastest-x", "levels", "grad-rows", "grad-planes")


def _row_starts(layout, off):
    """For every touched cell the start of the true row it belongs to."""
    starts = np.asarray(layout.offsets)
    return starts[np.searchsorted(starts, off, side="right") - 1]


def _standin(xbuf, lx, x_off, ybuf, ly, y_off, read=None, write=None):
    """y[b, d] = x[b, d] + 2 x[b, d + 1] through explicit element offsets.  `read` / `write` name a truncation applied
    to the ROW START of every access (the `b * ldx`, `c * ldx`, `l * xs_lev` of a kernel); an access that leaves the
    buffer -- a fault on the device -- reads 0 / writes nothing."""
    isz = xbuf.dtype.itemsize

    def narrowed(layout, off, kind):
        if kind is None:
            return off
        starts = _row_starts(layout, off)
        cut = np.vectorize(lambda o: fc.truncate(o, isz, kind, M))(starts)
        return cut + (off - starts)

    xo, yo = narrowed(lx, x_off, read), narrowed(ly, y_off, write)
    ok = (xo >= 0) & (xo < xbuf.size)
    xv = np.where(ok, xbuf[np.where(ok, xo, 0)], 0).astype(np.float64)
    y = (xv[:, :-1] + 2.0 * xv[:, 1:]).astype(ybuf.dtype)
    ok = (yo >= 0) & (yo < ybuf.size)
    ybuf[yo[ok]] = y[ok]


def _run(name, dt, read=None, write=None):
    """The pattern of tests/test_gpu_far_offsets.py on numpy buffers.  Returns the two checks as callables."""
    rng = np.random.default_rng(5)
    lx, ly, x_off, y_off = _layouts(name)
    dtype = np.dtype(DTYPES[dt])
    xbuf = (1000.0 + 50.0 * rng.standard_normal(lx.size)).astype(dtype)          # decoys
    true = (250.0 + 30.0 * rng.standard_normal(x_off.shape)).astype(dtype)
    xbuf[x_off] = true
    ybuf = np.frombuffer(bytes([fc.SENTINEL]) * (ly.size * dtype.itemsize), dtype=dtype).copy()
    _standin(xbuf, lx, x_off, ybuf, ly, y_off, read, write)
    want = (true.astype(np.float64)[:, :-1] + 2.0 * true.astype(np.float64)[:, 1:]).astype(dtype)
    return (lambda: fc.check_rows(ybuf[y_off], want, name),
            lambda: fc.check_windows(lambda s, e: ybuf[s:e], ly, dtype.itemsize, name))


@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_the_unwrapped_standin_passes(name, dt):
    rows, wins = _run(name, dt)
    rows()
    wins()


@pytest.mark.parametrize("kind", fc.TRUNCATIONS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_a_wrapped_read_is_caught(name, dt, kind):
    rows, wins = _run(name, dt, read=kind)
    with pytest.raises(AssertionError, match="differ in their bits"):
        rows()
    wins()                                      # nothing was written elsewhere


@pytest.mark.parametrize("kind", fc.TRUNCATIONS)
@pytest.mark.parametrize("dt", DTYPES)
@pytest.mark.parametrize("name", LAYOUTS)
def test_a_wrapped_write_is_caught(name, dt, kind):
    rows, wins = _run(name, dt, write=kind)
    with pytest.raises(AssertionError, match="differ in their bits"):
        rows()                                  # the true row kept its sentinel bytes
    with pytest.raises(AssertionError, match=kind):
        wins()                                  # and the alias window names the truncation


@pytest.mark.parametrize("kind", (None,) + fc.TRUNCATIONS)
@pytest.mark.parametrize("which", ["ld_row", "ld_plane"])
def test_a_narrowed_gradient_stride_is_caught(which, kind):
    """smm_gradients writes plane p of batch row b at g + b * ld_row + p * ld_plane from the pointer to row 0.  Here one
    of the two products alone is narrowed, in the layouts of tests/test_gpu_gradients_far_offsets.py: 3 rows of 3 near
    planes on a far `ld_row`; one row of 3 planes on a far `ld_plane`."""
    n_planes = 3
    if which == "ld_row":
        n_batch = 3
        lay, ld_row = fc.rows_layout(n_batch, S, M, G, inner=n_planes)
        ld_plane = lay.offsets[1] - lay.offsets[0]
    else:
        n_batch = 1
        lay, ld_plane = fc.rows_layout(n_planes, S, M, G)
        ld_row = n_planes * ld_plane
    rng = np.random.default_rng(6)
    want = rng.standard_normal((n_batch * n_planes, S))
    ybuf = np.frombuffer(bytes([fc.SENTINEL]) * (lay.size * 8), dtype=np.float64).copy()
    for b in range(n_batch):
        for p in range(n_planes):
            far_part, near_part = (b * ld_row, p * ld_plane) if which == "ld_row" else (p * ld_plane, b * ld_row)
            assert lay.offsets[0] + far_part + near_part == lay.offsets[b * n_planes + p]
            at = lay.offsets[0] + (far_part if kind is None else fc.truncate(far_part, 8, kind, M)) + near_part
            if 0 <= at and at + S <= lay.size:             # elsewhere: a fault on the device
                ybuf[at:at + S] = want[b * n_planes + p]

    def rows():
        fc.check_rows(np.stack([ybuf[o:o + S] for o in lay.offsets]), want, which)

    def wins():
        fc.check_windows(lambda s, e: ybuf[s:e], lay, 8, which)

    if kind is None:
        rows()
        wins()
    else:
        with pytest.raises(AssertionError, match="differ in their bits"):
            rows()
        with pytest.raises(AssertionError, match=kind):
            wins()


SMALL = [(M, G, s) for s in ((5, 25, 1), (5, 24, 1), (9, 25, 1), (25, 3, 1), (24, 3, 1), (3, 24, 1), (3, 25, 2))]
FULL = [(fc.MODULUS, fc.GUARD, s) for s in ((5, 1040, 1), (9, 4000, 1), (36, 131, 1), (3, 805, 1), (131, 36, 1),
                                            (3, 1040, 2), (3, 36 * 136, 1),
                                            # the gradient cases: 257 x 33 cells, planes of 2 and 3, results of 300
                                            (5, 8481, 1), (3, 8481, 1), (3, 8481, 2), (3, 8481, 3), (5, 300, 1))]
GRAD_SMALL = [(M, G, (3, 25, 3))]              # appended last: the ids of the cases above keep their numbers


@pytest.mark.parametrize("itemsize", (1, 2, 4, 8))
@pytest.mark.parametrize("modulus,guard,shape", SMALL + FULL + GRAD_SMALL)
def test_windows_never_overlap_a_true_row(shape, itemsize, modulus, guard):
    n_rows, row_len, inner = shape
    lay, ld = fc.rows_layout(n_rows, row_len, modulus, guard, inner=inner)
    assert ld % 4 == 0 and all(o % 4 == 0 for o in lay.offsets)
    wins = fc.windows(lay, itemsize)           # raises if a window overlaps a true row
    for s, e in wins:
        assert 0 <= s < e <= lay.size
        for o in lay.offsets:
            assert e <= o or s >= o + lay.row_len
    for (s0, e0), (s1, e1) in zip(wins, wins[1:]):
        assert e0 < s1
    # every row past a threshold has an alias window of its own truncations
    for o in lay.offsets:
        if o >= modulus:
            assert fc.aliases(o, itemsize, lay.size, modulus), o


def test_the_standard_layouts_cross_where_the_issue_says():
    lay, ld = fc.rows_layout(5, 1040)
    assert ld == (1 << 30) + 1040 + 8192 and lay.crossed() == (3, 1)
    assert [o >= 1 << 31 for o in lay.offsets] == [False, False, True, True, True] and lay.offsets[4] >= 1 << 32
    lay, ld = fc.rows_layout(36, 131)
    assert ld == (1 << 27) + fc._round4(131 + 8192) and lay.offsets[16] >= 1 << 31 and lay.offsets[32] >= 1 << 32
    assert lay.offsets[15] < 1 << 31 and lay.offsets[31] < 1 << 32


@pytest.mark.parametrize("itemsize", (2, 4))
def test_the_host_layout_crosses_2_32_bytes_and_2_31_elements(itemsize):
    lay, ld = fc.host_rows_layout(5, 4000)
    assert ld == (1 << 29) + 4000 + 8192 and lay.nbytes(4) < 9e9
    assert lay.offsets[2] * 4 >= 1 << 32 and lay.offsets[4] >= 1 << 31 and lay.offsets[4] * 2 >= 1 << 32
    wins = fc.windows(lay, itemsize)
    assert all(e <= o or s >= o + lay.row_len for s, e in wins for o in lay.offsets)
    assert fc.aliases(lay.offsets[4], itemsize, lay.size) and (itemsize == 2 or fc.aliases(lay.offsets[2], 4, lay.size))


# ------------------------------------------------------------------ byte streams at far byte offsets

def _cpx_rows():
    """Short complex-packed rows (the streams must fit below modulus / 4 = 1024 bytes): orders 2, 1 and 0 far, the alias
    of the second, one near row."""
    from tests import complex_cases as xc
    rng = np.random.default_rng(21)
    smooth = (2000 + 900 * np.sin(np.arange(60) / 7.0)).astype(np.int64) + rng.integers(0, 9, 60)
    far = [xc.Case("far_order2", smooth, 2, xc.even(60, 5)), xc.Case("far_order1", smooth[::-1] + 3, 1, xc.even(60, 4)),
           xc.Case("far_order0", rng.integers(0, 4096, 48), 0, xc.even(48, 6))]
    return far + [fc.cpx_alias(far[1]), xc.case("n3_order2")]


def _aec_rows():
    from tests import ccsds_cases as cc
    far = [cc.fixture("edge_n43_w12_pp1"), cc.fixture("edge_n43_w32_pp0"), cc.fixture("edge_n9_w16_pp0")]
    return far + [fc.aec_alias(far[1]), cc.fixture("edge_n16_w17_pp0")]


def _cpx_decode(buf, row, off):
    from smmregrid_amd.griblite import cpx_decode
    return cpx_decode(buf, row.record(off)), np.asarray(row.X, dtype=np.uint32)


def _aec_decode(buf, row, off):
    from smmregrid_amd.griblite import aec_decode
    from tests.ccsds_cases import record
    rec = record(off, row.stream.size, row.n_values, row.nbits, row.block, row.rsi, row.flags)
    return aec_decode(buf, rec), np.asarray(row.values, dtype=np.uint32)


@pytest.mark.parametrize("codec", ["cpx", "aec"])
def test_a_stream_read_at_a_narrowed_byte_offset_is_caught(codec):
    """The buffer of the GPU test's input-far cases at modulus 2^12, through the library's host decoders: every true row
    decodes to its integers with its record; with its byte_off narrowed in each way that keeps it inside the buffer it
    is refused or decodes to other integers -- and the row whose narrowed offset is the alias row's decodes CLEANLY to
    the alias row's integers, the case that noise in the decoys cannot stand for."""
    rows, decode = (_cpx_rows(), _cpx_decode) if codec == "cpx" else (_aec_rows(), _aec_decode)
    lay = fc.stream_layout([r.stream.size for r in rows[:3]], [r.stream.size for r in rows[4:]], M, G)
    assert lay.far[0] > M and lay.far[1] > 2 * M and lay.far[1] % 2 == 1 and lay.far[2] > 8 * M
    assert lay.alias == lay.far[1] % (2 * M) and lay.x_bytes == lay.far[2] + rows[2].stream.size
    buf = fc.stream_buffer(lay, [r.stream for r in rows], seed=3)
    seen, clean = set(), set()
    for off, row in zip(lay.offsets(), rows):
        got, want = decode(buf, row, off)
        assert np.array_equal(got, want), row
        for kind, at in fc.stream_images(off, lay.x_bytes, M).items():
            seen.add(kind)
            try:
                got, _ = decode(buf, row, at)
            except ValueError:
                continue
            assert not np.array_equal(got, want), (row, kind, at)
            if at == lay.alias:
                assert np.array_equal(got, np.asarray(rows[3].X, dtype=np.uint32)), (row, kind)
                clean.add(kind)
    assert seen == set(fc.STREAM_TRUNCATIONS), seen
    assert clean == {"elems31", "elems32", "bytes32", "sext32", "bits32"}, clean      # far[1] under all that move it


def test_stream_images_by_hand():
    big = 1 << 40
    assert fc.stream_images((1 << 31) + 77, big) == {"elems31": 77, "bits32": 77}
    assert fc.stream_images((1 << 32) + 77, big) == {k: 77 for k in ("elems31", "elems32", "bytes32", "sext32", "bits32")}
    assert fc.stream_images((1 << 34) + 77, big) == {k: 77 for k in fc.STREAM_TRUNCATIONS}
    assert fc.stream_images((1 << 29) + 77, big) == {"bits32": 77} and fc.stream_images(77, big) == {}
    lay = fc.stream_layout([4100, 8200, 3001], [4100, 9])
    assert [o >> 31 for o in lay.far] == [1, 2, 8] and lay.far[1] % 2 == 1 and lay.alias == lay.far[1] - (1 << 32)
    assert (1 << 34) < lay.x_bytes < (1 << 34) + (1 << 20) and all(o < 1 << 20 for o in lay.near)


def _slots(kind=None):
    """[A, spacer, B, spacer, C] laid back to back, 4-byte aligned, as the packers lay their streams: B begins past
    modulus bytes, C past twice that.  A stand-in writes every row at its offset narrowed by `kind`; a write that
    leaves the buffer -- a fault on the device -- writes nothing."""
    rng = np.random.default_rng(8)
    rows = [rng.integers(0, 0x40, n, dtype=np.uint8) for n in (41, M + 50, 43, M + 10, 37)]
    offs = np.concatenate([[0], np.cumsum([fc._round4(r.size) for r in rows])])
    used, size = int(offs[-1]), int(offs[-1]) + 64
    assert offs[2] >= M and offs[4] >= 2 * M
    buf = np.full(size, fc.SENTINEL, np.uint8)
    for off, r in zip(offs, rows):
        at = int(off) if kind is None else fc.truncate(int(off), 1, kind, M)
        if 0 <= at and at + r.size <= size:
            buf[at:at + r.size] = r
    checked = [(int(offs[i]), rows[i]) for i in (0, 2, 4)] + [(int(offs[i]), rows[i][:16]) for i in (1, 3)] + \
        [(int(offs[i]) + rows[i].size - 16, rows[i][-16:]) for i in (1, 3)]
    return lambda: fc.check_slots(lambda s, e: buf[s:e], checked, used, size, "slots")


def test_a_slot_written_at_a_narrowed_offset_is_caught():
    _slots()()
    for kind in fc.TRUNCATIONS:
        with pytest.raises(AssertionError, match="bytes differ"):
            _slots(kind)()
    buf = np.full(64, fc.SENTINEL, np.uint8)
    buf[40] = 0
    with pytest.raises(AssertionError, match="byte 40 behind the 32 bytes used"):
        fc.check_slots(lambda s, e: buf[s:e], [], 32, 64)


def test_aliases_by_hand():
    big = 1 << 40
    assert fc.aliases((1 << 32) + 20, 4, big) == [20]                         # 20 under every truncation
    assert fc.aliases((1 << 31) + 20, 2, big) == [20]                         # sign-extended: negative, not in the buffer
    assert fc.aliases((1 << 30) + 20, 8, big) == [20]                         # only the byte offset wraps: 2^33 + 160
    assert fc.aliases((1 << 30) + 20, 4, big) == [20]
    assert fc.aliases(3 * (1 << 30) + 20, 4, big) == [20, (1 << 30) + 20]     # bytes32 and elems31
    assert fc.aliases(100, 8, big) == []
    assert fc.truncate((1 << 31) + 20, 4, "sext32") == 20 - (1 << 31)
