"""The host builder of operators with weight columns (smm_operator_create_cols: csrc/smm_build.cpp's build_csr_cols,
prune_zero_links_cols, build_sell_cols) under AddressSanitizer + UBSan on the CPU, through a stand-alone program:
every column follows the permutation and the sequential duplicate summing of the one-column builder, column 0 IS that
builder's output, a link is pruned only when all its columns are zero, and 0 or 5 columns are refused."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "build_cols_harness_asan")
SOURCES = [os.path.join(ROOT, "tests", "cpp", "build_cols_harness.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_build.cpp"),
           os.path.join(ROOT, "smmregrid_amd", "csrc", "smm_hostpool.cpp")]


@pytest.fixture(scope="module")
def harness():
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-pthread", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", EXE] + SOURCES)
    yield EXE
    os.remove(EXE)


def run(exe, n_src, n_dst, src, dst, w, n_cols, prune=False, threads=1):
    w = np.asarray(w, dtype=np.float64).reshape(len(src), -1)
    text = f"{n_src} {n_dst} {len(src)} {n_cols} {int(prune)}\n" + "".join(
        f"{int(s)} {int(d)} " + " ".join(repr(float(v)) for v in row) + "\n" for s, d, row in zip(src, dst, w))
    out = subprocess.run([exe, str(threads)], input=text, capture_output=True, text=True, timeout=120,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, out.stderr[-3000:]
    return out.stdout.splitlines()


def statement(n_dst, src, dst, w):
    """(rowptr, col, val (nnz, K)): links ordered by (dst, src) with the link index as tie-break, duplicate coordinates
    summed one after the other in that order -- written per column, with Python floats."""
    order = np.lexsort((np.arange(len(src)), src, dst))
    rowptr, col, val = np.zeros(n_dst + 1, dtype=np.int64), [], []
    for k in order:
        if col and last == (dst[k], src[k]):
            val[-1] = [a + float(b) for a, b in zip(val[-1], w[k])]
        else:
            col.append(int(src[k]) - 1)
            val.append([float(b) for b in w[k]])
            rowptr[dst[k]] += 1
        last = (dst[k], src[k])
    # rowptr[d] counted the links of row d - 1 (1-based addresses): its running sum is the CSR's rowptr
    return np.cumsum(rowptr), np.array(col, dtype=np.int64), np.array(val, dtype=np.float64).reshape(len(col), w.shape[1])


def parse(lines, at, nnz, n_cols):
    """(col, val (nnz, K)) from the col line at `at` and the VAL lines behind it."""
    col = np.array(lines[at].split(), dtype=np.int64)
    val = np.empty((nnz, n_cols))
    for k in range(n_cols):
        head, *nums = lines[at + 1 + k].split()
        assert head == "VAL" and int(nums[0]) == k
        val[:, k] = [float(v) for v in nums[1:]]
    return col, val


def links(rng, n_src, n_dst, nnz, n_cols, dup_frac=0.4):
    src = rng.integers(1, n_src + 1, size=nnz).astype(np.int32)
    dst = rng.integers(1, n_dst + 1, size=nnz).astype(np.int32)
    n_dup = int(nnz * dup_frac)
    pick = rng.integers(0, nnz, size=n_dup)
    src[:n_dup], dst[:n_dup] = src[pick], dst[pick]          # duplicates, spread by the shuffle below
    perm = rng.permutation(nnz)
    src, dst = src[perm], dst[perm]
    w = rng.standard_normal((nnz, n_cols)) * 10.0 ** rng.integers(-6, 6, size=(nnz, n_cols))
    return src, dst, w


@pytest.mark.parametrize("threads", [1, 3])
@pytest.mark.parametrize("n_cols", [1, 2, 3, 4])
def test_every_column_follows_the_one_column_builder(harness, rng, n_cols, threads):
    n_src, n_dst = 57, 131                                   # rows without links, more than two SELL slices
    src, dst, w = links(rng, n_src, n_dst, 1500, n_cols)
    lines = run(harness, n_src, n_dst, src, dst, w, n_cols, threads=threads)
    nnz = int(lines[0].split()[1])
    rowptr, col, val = statement(n_dst, src, dst, w)
    assert nnz == col.size
    assert np.array_equal(np.array(lines[1].split(), dtype=np.int64), rowptr)
    got_col, got_val = parse(lines, 2, nnz, n_cols)
    assert np.array_equal(got_col, col)
    assert np.array_equal(got_val.view(np.uint64), val.view(np.uint64))      # the same sums in the same order, every column
    assert "COL0BAD 0" in lines and "SELLBAD 0" in lines


def test_links_already_in_cdo_order_take_the_sort_free_path(harness, rng):
    n_src, n_dst = 40, 70
    src, dst, w = links(rng, n_src, n_dst, 900, 4)
    order = np.lexsort((src, dst))
    src, dst, w = src[order], dst[order], w[order]
    lines = run(harness, n_src, n_dst, src, dst, w, 4, threads=3)
    nnz = int(lines[0].split()[1])
    rowptr, col, val = statement(n_dst, src, dst, w)
    got_col, got_val = parse(lines, 2, nnz, 4)
    assert np.array_equal(got_col, col) and np.array_equal(got_val.view(np.uint64), val.view(np.uint64))
    assert "COL0BAD 0" in lines and "SELLBAD 0" in lines


def test_pruning_needs_all_columns_zero(harness, rng):
    n_src, n_dst = 30, 20
    _, _, w = links(rng, n_src, n_dst, 300, 3, dup_frac=0.0)
    cells = rng.permutation(n_src * n_dst)[:300]         # distinct coordinates: no sum hides a zero
    src, dst = (cells % n_src + 1).astype(np.int32), (cells // n_src + 1).astype(np.int32)
    w[::5] = 0.0                       # every column zero: these go
    w[1::5, 0] = 0.0                   # column 0 zero alone: these stay
    w[2::5, 1:] = 0.0                  # only column 0 set: these stay
    w[3, :] = [0.0, -0.0, 0.0]         # signed zeros are zeros
    lines = run(harness, n_src, n_dst, src, dst, w, 3, prune=True)
    rowptr, col, val = statement(n_dst, src, dst, w)
    keep = (val != 0.0).any(axis=1)
    at = next(i for i, ln in enumerate(lines) if ln.startswith("PRUNED"))
    dropped, nnz = (int(v) for v in lines[at].split()[1:])
    assert dropped == int((~keep).sum()) and dropped >= 60 and nnz == int(keep.sum())
    rows = np.repeat(np.arange(n_dst), np.diff(rowptr))[keep]
    assert np.array_equal(np.array(lines[at + 1].split(), dtype=np.int64),
                          np.concatenate(([0], np.cumsum(np.bincount(rows, minlength=n_dst)))))
    got_col, got_val = parse(lines, at + 2, nnz, 3)
    assert np.array_equal(got_col, col[keep]) and np.array_equal(got_val.view(np.uint64), val[keep].view(np.uint64))
    assert (got_val[:, 0] == 0.0).any()                      # a link whose column 0 is zero survived


@pytest.mark.parametrize("n_cols", [0, 5])
def test_column_counts_outside_1_to_4_are_refused(harness, n_cols):
    width = max(n_cols, 1)
    lines = run(harness, 3, 2, [1, 2], [1, 2], np.ones((2, width)), n_cols)
    assert lines[0].startswith("ERROR n_cols") and "outside 1..4" in lines[0]


def test_bad_addresses_are_refused_with_columns_too(harness):
    lines = run(harness, 3, 2, [4], [1], np.ones((1, 3)), 3)
    assert lines[0].startswith("ERROR src_address")
