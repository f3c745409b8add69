"""One validator (check_levels, smm_device.hip) serves every level-group entry: smm_group_apply, smm_group_apply_sb and
smm_group_apply_host -- packed outer blocks, whole rows and level-major chunks -- refuse the same bad calls with
SMM_ERR_INVALID before anything is launched, and the next valid call is bit-equal to the oracle.  The chunk plan's
byte counts (smm::plan_group_chunks) reach the pipeline's copies intact."""
import ctypes

import numpy as np
import pytest

from oracle import oracle
from smmregrid_amd import OperatorGroup, _lib, gridgen, to_device
from smmregrid_amd.weights import compute_weights_matrix3d
from tests.helpers import assert_same, bits_equal

pytestmark = pytest.mark.gpu

N_OUTER, L = 40, 3          # 40 batch entries per level (n_inner = 1): at least the 32 a packed outer block needs
SENTINEL = -12345.678
LEV = np.arange(L, dtype=np.int32)
# host_chunk_kb: 0 = the default rule (one packed block of all 40 outer indices); 1 = a 4-KiB cap holds fewer than 32
# outer indices of the widest level, so the planner falls back to whole rows; 16 = level-major (see the stats test)
HOST_MODES = (("packed", 0, 0), ("whole rows", _lib.APPLY_HOST_NO_PACK, 0), ("budget 1 KiB", 0, 1), ("level-major", 0, 16))
# what is wrong with the call: (level_index, masked, remap_area_min, group, the valid call that follows)
BAD_CALLS = {
    "level_index 3": (np.array([0, 3, 1], np.int32), True, 0.5, "full", "full"),
    "level_index -1": (np.array([-1, 1, 2], np.int32), True, 0.5, "full", "full"),
    "a level without dst_imask": (LEV, True, 0.5, "no_imask", "unmasked"),
    "last level without dst_frac": (LEV, True, 0.5, "no_frac", "no_area_min"),
    "remap_area_min 1.5": (LEV, True, 1.5, "full", "full"),
}
# the valid calls: (masked, remap_area_min)
VALID = {"full": (True, 0.5), "unmasked": (False, 0.5), "no_area_min": (True, 0.0)}


@pytest.fixture(scope="module")
def case(hip):
    rng = np.random.default_rng(20261018)
    nx, ny = 24, 12
    src = gridgen.regular_grid(nx, ny)
    masks = gridgen.synthetic_ocean_masks(nx, ny, L, top=0.45, bottom=0.06)
    w3 = gridgen.ConservativeLevels(src, "r8x4").stack(masks, np.arange(L, dtype=np.float64))
    frac = w3["dst_grid_frac"].values
    groups, imask = {}, None
    for name in ("full", "no_imask", "no_frac"):
        ops = compute_weights_matrix3d(w3, "lev", device=0)
        if imask is None:
            imask = np.stack([op.mask_apply(masks[i]) for i, op in enumerate(ops)])
        for i, op in enumerate(ops):
            op.set_epilogue(None if (name == "no_imask" and i == 1) else imask[i],
                            None if (name == "no_frac" and i == L - 1) else frac[i])
        groups[name] = OperatorGroup(ops)
    ops = groups["full"].operators
    S, D = ops[0].n_src, ops[0].n_dst
    used = [op.n_used_src for op in ops]
    assert 0 < sum(used) * 5 <= L * S * 4                        # the packing variant applies
    x = 10.0 + 5.0 * rng.standard_normal((N_OUTER, L, 1, S))
    for l in range(L):
        x[:, l][:, :, masks[l] == 0] = np.nan
    csrs = [op.export_csr() for op in ops]
    refs = {}
    for name, (masked, area_min) in VALID.items():
        refs[name] = oracle.apply_levels(csrs, x, 1, LEV, np.full(L, masked), imask, frac if area_min > 0 else None,
                                         area_min, True)
        refs[name].setflags(write=False)
    group_of_valid = {"full": "full", "unmasked": "no_imask", "no_area_min": "no_frac"}
    x_dev = to_device(x)
    x_sb = to_device(np.ascontiguousarray(x.reshape(N_OUTER, L, S).transpose(1, 2, 0)), layout="sb")
    yield dict(groups=groups, S=S, D=D, used=used, x=x, x_dev=x_dev, x_sb=x_sb, refs=refs, group_of_valid=group_of_valid)
    for g in groups.values():
        g.close()


def _host_call(grp, x, out, lev, masked, area_min, flags):
    """smm_group_apply_host into a result buffer of the caller's (transpose order)."""
    n_outer, n_lev, n_inner, _ = x.shape
    _lib.call("smm_group_apply_host", grp.handle, x.ctypes.data_as(ctypes.c_void_p), 1, out.ctypes.data_as(ctypes.c_void_p),
              1, n_outer, n_lev, n_inner, 1, lev.ctypes.data_as(ctypes.c_void_p), None, float(area_min),
              flags | (_lib.APPLY_MASKED if masked else 0), 0)


def _entries(case):
    """name -> f(group, level_index, masked, area_min, y or None) -> the result on the host; y: a prefilled result buffer
    of that entry (device array / numpy array), made by `fresh(name)`."""
    D = case["D"]

    def dev(grp, lev, masked, area_min, y):
        return grp.apply(case["x_dev"], lev, y=y, masked=masked, remap_area_min=area_min).to_host().reshape(N_OUTER, 1, L, D)

    def sb(grp, lev, masked, area_min, y):
        return grp.apply_sb(case["x_sb"], lev, y=y, masked=masked, remap_area_min=area_min).to_host().reshape(N_OUTER, 1, L, D)

    def host(flags, kb):
        def run(grp, lev, masked, area_min, y):
            out = np.empty((N_OUTER, 1, L, D)) if y is None else y
            with _lib.tuning(host_chunk_kb=kb):
                _host_call(grp, case["x"], out, lev, masked, area_min, flags)
            return out
        return run

    entries = {"smm_group_apply": dev, "smm_group_apply_sb": sb}
    for label, flags, kb in HOST_MODES:
        entries[f"smm_group_apply_host, {label}"] = host(flags, kb)
    return entries


def _fresh(case, name):
    D = case["D"]
    if name == "smm_group_apply":
        return to_device(np.full((N_OUTER, 1, L, D), SENTINEL))
    if name == "smm_group_apply_sb":
        return to_device(np.full((N_OUTER, L, D), SENTINEL))
    return np.full((N_OUTER, 1, L, D), SENTINEL)


@pytest.mark.parametrize("bad", list(BAD_CALLS))
def test_every_group_entry_refuses_the_same_calls_before_any_launch(case, bad):
    lev, masked, area_min, group, valid = BAD_CALLS[bad]
    sentinel = np.full(N_OUTER * L * case["D"], SENTINEL)
    for name, entry in _entries(case).items():
        y = _fresh(case, name)
        with pytest.raises(_lib.SmmError) as e:
            entry(case["groups"][group], lev, masked, area_min, y)
        assert e.value.code == _lib.SMM_ERR_INVALID, (name, str(e.value))
        after = y if isinstance(y, np.ndarray) else y.to_host()
        bits_equal(after.ravel(), sentinel)                # Y untouched: nothing was launched for the refused call
        # the refusal leaves no state behind: a valid call on the same group, straight after
        v_masked, v_area_min = VALID[valid]
        got = entry(case["groups"][case["group_of_valid"][valid]], LEV, v_masked, v_area_min, None)
        assert_same(got, case["refs"][valid], exact=True)


@pytest.mark.parametrize("kb", [0, 1, 16])
def test_the_plans_byte_counts_reach_the_copies(case, kb):
    """The packed plans ship each level's used cells and nothing else: h2d_bytes = sum_l U_l * 40 * 8, in one block of all
    40 outer indices (kb = 0) or level-major.  Level-major needs 32 outer indices of the widest level within the cap of
    four budgets: 4 * 16 KiB / (U_max * 8 B) >= 32 holds for 16 KiB (the levels together exceed the 16-KiB target: more
    than one chunk), while the 4 KiB of kb = 1 hold fewer than 32, so that call ships whole rows: 3 * 40 * S * 8, one
    block as for kb = 0.  Y comes back once, 3 * 40 * D * 8 bytes, whatever the plan."""
    S, D, used = case["S"], case["D"], case["used"]
    assert 4 * 16 * 1024 // (max(used) * 8) >= 32 > 4 * 1024 // (max(used) * 8) and sum(used) * N_OUTER * 8 > 16 * 1024
    grp = case["groups"]["full"]
    out = np.empty((N_OUTER, 1, L, D))
    with _lib.tuning(host_chunk_kb=kb):
        _lib.host_stats(reset=True)
        _host_call(grp, case["x"], out, LEV, True, 0.5, 0)
        st = _lib.host_stats(reset=True)
    assert_same(out, case["refs"]["full"], exact=True)
    print(f"host_chunk_kb={kb}: chunks {st['chunks']}, h2d_bytes {st['h2d_bytes']}, d2h_bytes {st['d2h_bytes']}")
    assert st["h2d_bytes"] == (L * S if kb == 1 else sum(used)) * N_OUTER * 8
    assert st["d2h_bytes"] == L * N_OUTER * D * 8
    assert 1 < st["chunks"] <= L if kb == 16 else st["chunks"] == 1
