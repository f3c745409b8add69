"""The entries behind `gradients=True` at the ABI: declared, exported and bound, the version unchanged, and every refusal
that needs no device -- of smm_grad_plan_create, smm_gradients, smm_apply_cols, smm_apply_cols_scratch and of
`Regridder(gradients=True)`."""
import ctypes
import os
import re

import numpy as np
import pytest

from smmregrid_amd import Regridder, _lib, gridgen

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smmregrid_amd.h")
NEW = ("smm_operator_create_cols", "smm_operator_cols", "smm_operator_export_cols", "smm_grad_plan_create",
       "smm_grad_plan_destroy", "smm_gradients", "smm_apply_cols", "smm_apply_cols_scratch")


def test_new_symbols_are_declared_exported_and_bound():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(smm_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", text) and lib.smm_abi_version() == 6      # entries are only added
    assert re.search(r"SMM_GRAD_I\s*=\s*0,\s*SMM_GRAD_J\s*=\s*1,\s*SMM_GRAD_IJ\s*=\s*2", text)


def status(name, *args):
    return getattr(_lib.load(), name)(*args), (_lib.load().smm_last_error() or b"").decode()


def plan_args(nx=4, ny=3, n_planes=3, kinds=(0, 1, 2), si=True, sj=True, ci=True, out=True):
    """(what must stay alive, the argument tuple) of one smm_grad_plan_create call; a refused call reads no table."""
    tx, ty = min(max(nx, 1), 64), min(max(ny, 1), 64)
    keep = [np.ones(3 * tx), np.ones(3 * ty), np.ones(ty), (ctypes.c_int * max(len(kinds), 1))(*kinds), ctypes.c_void_p()]
    ptr = lambda a, on: a.ctypes.data_as(ctypes.c_void_p) if on else None
    return keep, (nx, ny, 1, n_planes, keep[3], ptr(keep[0], si), ptr(keep[1], sj), ptr(keep[2], ci), 0,
                  ctypes.byref(keep[4]) if out else None)


def test_grad_plan_create_refuses_bad_tables_before_any_device():
    for kw, word in ((dict(n_planes=0), "n_planes=0"), (dict(n_planes=4, kinds=(0, 1, 2, 2)), "n_planes=4"),
                     (dict(si=False), "null table"), (dict(sj=False), "null table"), (dict(ci=False), "null table"),
                     (dict(n_planes=2, kinds=(0, 2)), "IJ plane needs a J plane"),
                     (dict(n_planes=1, kinds=(2,)), "IJ plane needs a J plane"),
                     (dict(n_planes=2, kinds=(0, 7)), "plane_kind[1]=7"), (dict(nx=0), "at least 1"),
                     (dict(nx=1 << 20, ny=1 << 20), "int32")):
        keep, args = plan_args(**kw)
        rc, msg = status("smm_grad_plan_create", *args)
        assert rc == _lib.SMM_ERR_INVALID and word in msg, (kw, rc, msg)
        assert keep[4].value is None
    keep, args = plan_args(out=False)
    assert status("smm_grad_plan_create", *args)[0] == _lib.SMM_ERR_INVALID
    assert _lib.load().smm_grad_plan_destroy(None) == _lib.SMM_OK
    if _lib.device_count() == 0:      # valid tables: the device is the next thing looked for
        keep, args = plan_args()
        assert status("smm_grad_plan_create", *args)[0] == _lib.SMM_ERR_NO_DEVICE


def test_gradients_refuses_dtypes_and_a_null_plan():
    for dt in (_lib.SMM_I16, _lib.SMM_U16, _lib.SMM_F16, _lib.SMM_BF16, 17):
        rc, msg = status("smm_gradients", None, None, dt, 12, None, 12, 36, 1, None)
        assert rc == _lib.SMM_ERR_UNSUPPORTED, (dt, msg)
    rc, msg = status("smm_gradients", None, None, _lib.SMM_F32, 12, None, 12, 36, 1, None)
    assert rc == _lib.SMM_ERR_INVALID and "null gradient plan" in msg


def apply_cols(x_dtype=_lib.SMM_F64, y_dtype=_lib.SMM_F64, flags=0):
    return status("smm_apply_cols", None, None, None, x_dtype, 12, None, y_dtype, 6, 1, 0.0, flags, None, 0, None)


def test_apply_cols_refuses_what_is_not_built_before_the_handles():
    unsupported = [dict(flags=_lib.APPLY_SKIPNA), dict(flags=_lib.APPLY_KERNEL_TILE), dict(flags=_lib.APPLY_SB_PACKED),
                   dict(flags=_lib.APPLY_SB_Y_SB), dict(flags=_lib.APPLY_HOST_NO_PACK), dict(x_dtype=_lib.SMM_I16),
                   dict(x_dtype=_lib.SMM_U16), dict(x_dtype=_lib.SMM_F16), dict(x_dtype=_lib.SMM_BF16),
                   dict(y_dtype=_lib.SMM_F32), dict(y_dtype=_lib.SMM_I16), dict(y_dtype=_lib.SMM_F16),
                   dict(y_dtype=_lib.SMM_BF16)]
    seen = set()
    for kw in unsupported:
        rc, msg = apply_cols(**kw)
        assert rc == _lib.SMM_ERR_UNSUPPORTED and msg, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 6                                  # one sentence per kind of refusal
    rc, msg = apply_cols(flags=1 << 20)
    assert rc == _lib.SMM_ERR_INVALID and "unknown apply flag" in msg
    rc, msg = apply_cols(flags=_lib.APPLY_SKIPNA | _lib.APPLY_NO_FILL)
    assert rc == _lib.SMM_ERR_INVALID
    for fl in (0, _lib.APPLY_MASKED, _lib.APPLY_KERNEL_SELL, _lib.APPLY_NO_FILL):      # built: the handle is looked at next
        rc, msg = apply_cols(flags=fl)
        assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg
    rc, msg = apply_cols(x_dtype=_lib.SMM_F32)
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg


def test_apply_cols_scratch_refuses_a_null_operator():
    n = ctypes.c_size_t(7)
    rc, msg = status("smm_apply_cols_scratch", None, 4, ctypes.byref(n))
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg and n.value == 7
    n_cols = ctypes.c_int(0)
    assert status("smm_operator_cols", None, ctypes.byref(n_cols))[0] == _lib.SMM_ERR_INVALID
    assert status("smm_operator_export_cols", None, None)[0] == _lib.SMM_ERR_INVALID


def test_create_cols_refuses_column_counts_outside_1_to_4():
    """On a host without a device the refusal of the device comes first (as for smm_operator_create); with one, the
    column count is refused by the host builder."""
    src, dst, w = np.array([1], np.int32), np.array([1], np.int32), np.ones(5)
    ptr = lambda a: a.ctypes.data_as(ctypes.c_void_p)
    for n_cols in (0, 5):
        h = ctypes.c_void_p()
        rc, msg = status("smm_operator_create_cols", 2, 2, 1, ptr(src), ptr(dst), ptr(w), n_cols, 0, 0, ctypes.byref(h))
        if _lib.device_count() == 0:
            assert rc == _lib.SMM_ERR_NO_DEVICE
        else:
            assert rc == _lib.SMM_ERR_INVALID and "outside 1..4" in msg
        assert h.value is None


# ------------------------------------------------------------------ Regridder(gradients=True): refused before any device work

@pytest.fixture(scope="module")
def bic_weights():
    return gridgen.generate_weights("r12x6", "r8x4", method="bic")


@pytest.mark.parametrize("kw, word", [(dict(skipna=True), "skipna"), (dict(packed=True), "packed"),
                                      (dict(half=True), "half"), (dict(keep_batch_fastest=True), "keep_batch_fastest"),
                                      (dict(out_dtype=np.float32), "out_dtype=float32"),
                                      (dict(out_dtype=np.float16), "out_dtype=float16")])
def test_regridder_names_what_gradients_does_not_go_with(bic_weights, kw, word):
    with pytest.raises(ValueError) as err:
        Regridder(weights=bic_weights, gradients=True, **kw)
    text = str(err.value)
    assert "gradients=True does not go with" in text and word in text and "it goes with" in text


def test_regridder_refuses_weights_without_gradient_columns(bic_weights):
    for method in ("bil", "con", "nn"):
        with pytest.raises(ValueError, match="num_wgts = 1"):
            Regridder(weights=gridgen.generate_weights("r12x6", "r8x4", method=method), gradients=True)


def test_regridder_refuses_masked_level_weights():
    masks = gridgen.synthetic_ocean_masks(12, 6, 2)
    levels = [gridgen.generate_weights("r12x6", "r8x4", method="bic", src_mask=m) for m in masks]
    w3d = gridgen.stack_level_weights(levels, [5.0, 50.0], method="bic")
    with pytest.raises(ValueError, match="masked-level"):
        Regridder(weights=w3d, gradients=True)


def test_regridder_refuses_a_source_that_is_no_regular_grid(bic_weights):
    from smmregrid_amd.xrlite import Dataset
    bent = Dataset(attrs=bic_weights.attrs, coords=bic_weights.coords)
    for k, v in bic_weights.data_vars.items():
        bent[k] = v
    lat = bic_weights["src_grid_center_lat"].values.copy()
    lat[3] += 1e-3
    bent["src_grid_center_lat"] = (bic_weights["src_grid_center_lat"].dims, lat, bic_weights["src_grid_center_lat"].attrs)
    with pytest.raises(ValueError, match="regular lon/lat source"):
        Regridder(weights=bent, gradients=True)


def test_without_the_keyword_nothing_changes_in_the_constructor(bic_weights):
    """gradients defaults to False: on a host without a device the constructor fails where it always did."""
    if _lib.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(_lib.SmmNoDeviceError):
        Regridder(weights=bic_weights)
    with pytest.raises(_lib.SmmNoDeviceError):          # valid gradients=True: refused by the device, not by a check
        Regridder(weights=bic_weights, gradients=True)
