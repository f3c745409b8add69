"""tests/far_cases.py catches what it is for: at modulus 2^12 a numpy stand-in for an apply has its read offsets, or
its write offsets, narrowed in each of the four ways, in every layout the GPU test uses; the decoy / sentinel checks
must fail for each of them and pass for the stand-in that narrows nothing."""
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
    raise KeyError(name)


LAYOUTS = ("row-major", "batch-fastest", "batch-fastest-x", "levels")


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


SMALL = [(M, G, s) for s in ((5, 25, 1), (5, 24, 1), (9, 25, 1), (25, 3, 1), (24, 3, 1), (3, 24, 1), (3, 25, 2))]
FULL = [(fc.MODULUS, fc.GUARD, s) for s in ((5, 1040, 1), (9, 4000, 1), (36, 131, 1), (3, 805, 1), (131, 36, 1),
                                            (3, 1040, 2), (3, 36 * 136, 1))]


@pytest.mark.parametrize("itemsize", (1, 2, 4, 8))
@pytest.mark.parametrize("modulus,guard,shape", SMALL + FULL)
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


def test_aliases_by_hand():
    big = 1 << 40
    assert fc.aliases((1 << 32) + 20, 4, big) == [20]                         # 20 under every truncation
    assert fc.aliases((1 << 31) + 20, 2, big) == [20]                         # sign-extended: negative, not in the buffer
    assert fc.aliases((1 << 30) + 20, 8, big) == [20]                         # only the byte offset wraps: 2^33 + 160
    assert fc.aliases((1 << 30) + 20, 4, big) == [20]
    assert fc.aliases(3 * (1 << 30) + 20, 4, big) == [20, (1 << 30) + 20]     # bytes32 and elems31
    assert fc.aliases(100, 8, big) == []
    assert fc.truncate((1 << 31) + 20, 4, "sext32") == 20 - (1 << 31)
