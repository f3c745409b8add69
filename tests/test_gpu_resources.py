"""Handles release what they own: HBM usage returns to its level after operators, groups and
their cached host-pipeline buffers are destroyed; buffers replaced or built on demand inside a live
handle (epilogue vectors, tile plans, the batch-fastest CSR, level configurations) are the ones the
kernels read afterwards."""
import gc

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import OperatorGroup, SparseOperator, _lib, gridgen, to_device
from smmregrid_amd.device import mem_info, synchronize
from tests.helpers import assert_same, field, ragged_links, random_links

pytestmark = pytest.mark.gpu


def test_no_device_memory_leak_over_handle_lifecycles(hip, rng):
    w = gridgen.conservative_weights("r144x72", "r48x24")
    S, D = w.sizes["src_grid_size"], w.sizes["dst_grid_size"]
    x = field(rng, 8, S)

    def cycle():
        ops = [SparseOperator(S, D, w["src_address"].values, w["dst_address"].values, w["remap_matrix"].values,
                              device=0) for _ in range(3)]
        for op in ops:
            op.set_epilogue(w["dst_grid_imask"].values, w["dst_grid_frac"].values)
        grp = OperatorGroup(ops)
        dx = to_device(x)
        ops[0].apply(dx, remap_area_min=0.5).free()
        ops[0].apply_host(x, remap_area_min=0.5)                       # allocates the cached pipeline
        grp.apply_host(x.reshape(2, 2, 2, S), [0, 1], masked=True, remap_area_min=0.5)
        ops[1].mask_apply(w["src_grid_imask"].values)
        dx.free()
        grp.close()
        for op in ops:
            op.close()

    cycle()                                                            # warm-up: runtime pools settle
    gc.collect()
    synchronize()
    free0, _ = mem_info()
    for _ in range(40):
        cycle()
    gc.collect()
    synchronize()
    free1, _ = mem_info()
    assert free0 - free1 < (8 << 20), f"device memory shrank by {(free0 - free1) / 2**20:.1f} MiB over 40 cycles"


# ---- operators large enough for a leaked array to show in mem_info()

BIG_S, BIG_D, BIG_LINKS, BIG_B = 40000, 20000, 600_000, 4


def _epilogue_vectors(rng, n_dst):
    return rng.integers(0, 2, size=n_dst).astype(np.int32), rng.random(n_dst)


@pytest.fixture(scope="module")
def big(hip):
    """Two operators of ~600 000 links each (SELL / CSR values ~4.8 MB, columns ~2.4 MB per array), two epilogues per
    operator, one field, and the oracle's results under the SECOND epilogue: per operator (B, D) and per group call."""
    rng = np.random.default_rng(20261019)
    links = [random_links(rng, BIG_S, BIG_D, BIG_LINKS) for _ in range(2)]
    csrs = [oracle.coo_to_csr_c(BIG_S, BIG_D, *ln) for ln in links]
    first = [_epilogue_vectors(rng, BIG_D) for _ in range(2)]
    second = [_epilogue_vectors(rng, BIG_D) for _ in range(2)]
    x = field(rng, BIG_B, BIG_S)
    src_imask = rng.integers(0, 2, size=BIG_S).astype(np.int32)
    imask2, frac2 = np.stack([e[0] for e in second]), np.stack([e[1] for e in second])
    x4 = x.reshape(2, 2, 1, BIG_S)                                    # (n_outer, n_lev, n_inner, S)
    ref = {"op": [oracle.apply_c(csrs[i], x, masked=True, dst_imask=imask2[i], dst_frac=frac2[i], area_min=0.5)
                  for i in range(2)],
           "mask": oracle.mask_apply_c(csrs[1], src_imask)}
    for name, lev in (("g01", [0, 1]), ("g10", [1, 0])):
        ref[name] = oracle.apply_levels(csrs, x4, 1, lev, [True, True], imask2, frac2, 0.5, True)
    for v in [*ref["op"], ref["mask"], ref["g01"], ref["g10"]]:
        v.setflags(write=False)
    return dict(links=links, first=first, second=second, x=x, x4=x4, src_imask=src_imask, ref=ref)


def _big_cycle(big, check):
    """Everything that allocates inside a handle, then everything closed.  check: compare each result with the oracle."""
    x, x4, ref = big["x"], big["x4"], big["ref"]
    same = assert_same if check else (lambda *a, **k: None)
    ops = [SparseOperator(BIG_S, BIG_D, *big["links"][i], device=0) for i in range(2)]
    for i, op in enumerate(ops):                                      # the second pair replaces the first
        op.set_epilogue(*big["first"][i])
        op.set_epilogue(*big["second"][i])
    dx, dx_sb, dx4 = to_device(x), to_device(np.ascontiguousarray(x.T), layout="sb"), to_device(x4)
    dx4_sb = to_device(np.ascontiguousarray(x4[:, :, 0, :].transpose(1, 2, 0)), layout="sb")   # (n_lev, S, n_outer)
    kw = dict(masked=True, remap_area_min=0.5)
    for y in (ops[0].apply(dx, **kw), ops[0].apply_sb(dx_sb, **kw)):  # apply_sb uploads the batch-fastest CSR
        same(y.to_host(), ref["op"][0], exact=True)
        y.free()
    same(ops[0].apply_host(x, chunk_rows=2, **kw), ref["op"][0], exact=True)          # two chunks: both pipe buffers
    if check:
        assert np.array_equal(ops[1].mask_apply(big["src_imask"]), ref["mask"])
    else:
        ops[1].mask_apply(big["src_imask"])
    grp = OperatorGroup(ops)
    for name, lev in (("g01", [0, 1]), ("g10", [1, 0])):              # two level configurations: two cache entries
        y = grp.apply(dx4, lev, **kw)
        same(y.to_host(), ref[name], exact=True)
        y.free()
    y = grp.apply_sb(dx4_sb, [0, 1], **kw)                            # (B, n_lev, D)
    same(y.to_host(), ref["g01"][:, 0], exact=True)
    y.free()
    same(grp.apply_host(x4, [0, 1], chunk_outer=1, **kw), ref["g01"], exact=True)     # two chunks
    for d in (dx, dx_sb, dx4, dx4_sb):
        d.free()
    grp.close()
    for op in ops:
        op.close()


def test_no_leak_of_megabyte_sized_arrays_over_handle_lifecycles(big):
    """12 cycles of create / set_epilogue twice / apply / apply_sb / apply_host / mask_apply / group of two with two
    level configurations, apply_sb and apply_host / close: one leaked column array (2.4 MB) per cycle would cost ~29 MB,
    the bound is the 8 MiB of the test above.  Blocks of D elements (epilogue vectors: 20 KB and 160 KB here),
    descriptors and level configurations are below this test's resolution: their ownership is covered on the CPU by
    tests/cpp/devmem_harness.cpp."""
    _big_cycle(big, check=True)                                       # warm-up: runtime pools settle; results checked
    gc.collect()
    synchronize()
    free0, _ = mem_info()
    for _ in range(12):
        _big_cycle(big, check=False)
    gc.collect()
    synchronize()
    free1, _ = mem_info()
    print(f"device memory shrank by {(free0 - free1) / 2**20:.2f} MiB over 12 cycles")
    assert free0 - free1 < (8 << 20), f"device memory shrank by {(free0 - free1) / 2**20:.1f} MiB over 12 cycles"


# ---- buffers replaced or built inside a live handle

def test_second_epilogue_replaces_the_first(hip):
    rng = np.random.default_rng(20261020)
    S, D = 5000, 1300
    src, dst, w = random_links(rng, S, D, 9000)
    csr = oracle.coo_to_csr_c(S, D, src, dst, w)
    (im1, fr1), (im2, fr2) = _epilogue_vectors(rng, D), _epilogue_vectors(rng, D)
    x = field(rng, 5, S)
    ref1, ref2 = (oracle.apply_c(csr, x, masked=True, dst_imask=im, dst_frac=fr, area_min=0.5)
                  for im, fr in ((im1, fr1), (im2, fr2)))
    assert not np.array_equal(np.isnan(ref1), np.isnan(ref2))        # the two epilogues can be told apart
    op = SparseOperator(S, D, src, dst, w, device=0)
    dx = to_device(x)
    op.set_epilogue(im1, fr1)
    assert_same(op.apply(dx, masked=True, remap_area_min=0.5).to_host(), ref1, exact=True)
    op.set_epilogue(im2, fr2)
    assert_same(op.apply(dx, masked=True, remap_area_min=0.5).to_host(), ref2, exact=True)
    grp = OperatorGroup([op])
    with pytest.raises(_lib.SmmError) as e:                           # a group's descriptors hold the vectors' addresses
        op.set_epilogue(im1, fr1)
    assert e.value.code == _lib.SMM_ERR_INVALID
    assert "operator belongs to a group: set the epilogue vectors before smm_group_create" in str(e.value)
    y = grp.apply(to_device(x.reshape(5, 1, 1, S)), [0], masked=True, remap_area_min=0.5).to_host()
    assert_same(y.reshape(5, D), ref2, exact=True)                    # the refused call changed nothing
    grp.close()
    op.close()


def test_plans_built_and_dropped_on_demand(hip):
    """A long-row operator tries several plan shapes at create and keeps one; grouped with a short-row operator (own
    shape: 256 rows per block) the group takes the long-row shape, which the short-row member then builds on demand."""
    rng = np.random.default_rng(20261021)
    S, D, B = 3000, 800, 6
    links = [ragged_links(rng, S, D, max_len=60), ragged_links(rng, S, D, max_len=16)]
    csrs = [oracle.coo_to_csr_c(S, D, *ln) for ln in links]
    ops = [SparseOperator(S, D, *ln, device=0) for ln in links]
    assert ops[0].max_row_nnz > 16 >= ops[1].max_row_nnz
    assert ops[0].plan_info()["rows_per_block"] <= 64 and ops[1].plan_info()["rows_per_block"] == 256
    x = field(rng, 2 * B, S, nan_frac=0.01)
    x4 = x.reshape(B, 2, 1, S)
    ref_op = [oracle.apply_c(c, x) for c in csrs]
    ref_grp = oracle.apply_levels(csrs, x4, 1, [0, 1], [False, False], None, None, 0.0, True)
    dx, dx4 = to_device(x), to_device(x4)
    grp = OperatorGroup(ops)
    forms = [0, _lib.APPLY_KERNEL_SELL] + ([_lib.APPLY_KERNEL_TILE] if grp.plan_info()["tile_plan"] else [])
    print(f"long rows: {ops[0].max_row_nnz} links, {ops[0].plan_info()}; group: {grp.plan_info()}")
    for flags in forms:
        assert_same(grp.apply(dx4, [0, 1], flags=flags).to_host(), ref_grp, exact=True)
    for op in ops:                                                    # the group's descriptors name the member's buffers
        with pytest.raises(_lib.SmmError) as e:
            _lib.call("smm_operator_destroy", op.handle)
        assert e.value.code == _lib.SMM_ERR_INVALID and "operator still belongs to a group" in str(e.value)
    grp.close()
    for op, ref in zip(ops, ref_op):
        assert_same(op.apply(dx).to_host(), ref, exact=True)
        op.close()


def test_double_close_is_harmless(hip):
    rng = np.random.default_rng(20261022)
    src, dst, w = random_links(rng, 300, 200, 900)
    op = SparseOperator(300, 200, src, dst, w, device=0)
    grp = OperatorGroup([op])
    grp.close()
    grp.close()
    op.close()
    op.close()
    assert op.handle is None and grp.handle is None
