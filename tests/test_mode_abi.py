"""The categorical apply at the ABI: declared, exported and bound, the version unchanged, every refusal that needs no
device -- of smm_apply_mode and smm_mode_launch_info on null handles -- and the clashes of `Regridder(categorical=...)` and
of a class variable's road, by name."""
import ctypes
import os
import re

import numpy as np
import pytest

from smmregrid_amd import Regridder, _lib, gridgen, road

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "smmregrid_amd.h")
NEW = ("smm_apply_mode", "smm_mode_launch_info")


def test_new_symbols_are_declared_exported_and_bound():
    raw = open(HEADER).read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    declared = set(re.findall(r"\b(smm_[a-z0-9_]+)\s*\(", text))
    lib = _lib.load()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", text) and lib.smm_abi_version() == 6      # entries are only added
    struct = re.search(r"typedef struct smm_mode_rule_t \{(.*?)\} smm_mode_rule_t;", text, re.S).group(1)
    assert re.findall(r"int32_t (\w+)", struct) == [n for n, _ in _lib.ModeRuleStruct._fields_]
    assert ctypes.sizeof(_lib.ModeRuleStruct) == 20
    assert "categorical fields" in raw and "remaplaf as recalled" in raw      # the rule has a heading of its own


def status(name, *args):
    return getattr(_lib.load(), name)(*args), (_lib.load().smm_last_error() or b"").decode()


def rule(n_fill=1, fill=(-1, 0), fill_out=-1, reserved=0):
    return _lib.ModeRuleStruct(n_fill, (ctypes.c_int32 * 2)(*fill), fill_out, reserved)


def apply_mode(x_dtype=_lib.SMM_F32, flags=0, rule=None, n_batch=1, x=None, y=None, share=None):
    return status("smm_apply_mode", None, x, x_dtype, 12, y, 6, share, 6, n_batch, 0.0, flags,
                  None if rule is None else ctypes.byref(rule), None)


def test_apply_mode_refuses_what_is_not_built_before_the_handles():
    unsupported = [dict(flags=_lib.APPLY_SKIPNA), dict(flags=_lib.APPLY_NO_FILL), dict(flags=_lib.APPLY_KERNEL_TILE),
                   dict(flags=_lib.APPLY_SB_PACKED), dict(flags=_lib.APPLY_SB_Y_SB), dict(flags=_lib.APPLY_HOST_NO_PACK),
                   dict(x_dtype=_lib.SMM_F16), dict(x_dtype=_lib.SMM_BF16), dict(x_dtype=17)]
    seen = set()
    for kw in unsupported:
        rc, msg = apply_mode(**kw)
        assert rc == _lib.SMM_ERR_UNSUPPORTED and msg, (kw, rc, msg)
        seen.add(msg)
    assert len(seen) >= 6                                  # one sentence per kind of refusal
    rc, msg = apply_mode(flags=1 << 20)
    assert rc == _lib.SMM_ERR_INVALID and "unknown apply flag" in msg
    for fl in (0, _lib.APPLY_MASKED, _lib.APPLY_KERNEL_SELL, _lib.APPLY_MASKED | _lib.APPLY_KERNEL_SELL):
        rc, msg = apply_mode(flags=fl)                     # built: the handle is looked at next
        assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg
    for dt in (_lib.SMM_I16, _lib.SMM_U16):
        rc, msg = apply_mode(x_dtype=dt, rule=rule(fill=(5, 0), fill_out=5))
        assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg
    rc, msg = apply_mode(x_dtype=_lib.SMM_F64)
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg


def test_apply_mode_refuses_a_bad_rule_before_the_handles():
    I16, U16, F32 = _lib.SMM_I16, _lib.SMM_U16, _lib.SMM_F32
    for kw, word in ((dict(x_dtype=F32, rule=rule()), "takes no smm_mode_rule_t"),
                     (dict(x_dtype=_lib.SMM_F64, rule=rule()), "takes no smm_mode_rule_t"),
                     (dict(x_dtype=I16), "needs a smm_mode_rule_t"), (dict(x_dtype=U16), "needs a smm_mode_rule_t"),
                     (dict(x_dtype=I16, rule=rule(n_fill=3)), "n_fill=3"), (dict(x_dtype=I16, rule=rule(n_fill=-1)), "n_fill=-1"),
                     (dict(x_dtype=I16, rule=rule(fill=(40000, 0))), "fill[0]=40000"),
                     (dict(x_dtype=U16, rule=rule(fill=(-1, 0), fill_out=0)), "fill[0]=-1"),
                     (dict(x_dtype=U16, rule=rule(n_fill=2, fill=(1, 65536), fill_out=0)), "fill[1]=65536"),
                     (dict(x_dtype=I16, rule=rule(fill_out=-32769)), "fill_out=-32769"),
                     (dict(x_dtype=U16, rule=rule(n_fill=0, fill_out=-1)), "fill_out=-1"),
                     (dict(x_dtype=I16, rule=rule(reserved=1)), "reserved")):
        rc, msg = apply_mode(**kw)
        assert rc == _lib.SMM_ERR_INVALID and word in msg, (kw, rc, msg)
    # only the first n_fill entries are looked at
    rc, msg = apply_mode(x_dtype=U16, rule=rule(n_fill=1, fill=(1, -7), fill_out=0))
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg


def test_apply_mode_refuses_a_negative_batch_and_misaligned_pointers_before_the_handles():
    rc, msg = apply_mode(n_batch=-1)
    assert rc == _lib.SMM_ERR_INVALID and "negative batch" in msg
    for kw in (dict(x=2), dict(y=6), dict(share=4), dict(x_dtype=_lib.SMM_F64, x=4),
               dict(x_dtype=_lib.SMM_U16, rule=rule(fill=(1, 0), fill_out=1), y=1)):
        kw = {k: ctypes.c_void_p(v) if k in ("x", "y", "share") else v for k, v in kw.items()}
        rc, msg = apply_mode(**kw)
        assert rc == _lib.SMM_ERR_INVALID and "not element aligned" in msg, (kw, rc, msg)
    rc, msg = apply_mode(x_dtype=_lib.SMM_U16, rule=rule(fill=(1, 0), fill_out=1), x=ctypes.c_void_p(2), y=ctypes.c_void_p(6))
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg      # 2-byte cells: aligned


def test_mode_launch_info_reports_the_capacity_without_an_operator():
    cap = ctypes.c_int(0)
    for dt, want in ((_lib.SMM_F32, 64), (_lib.SMM_I16, 64), (_lib.SMM_U16, 64), (_lib.SMM_F64, 32)):
        assert status("smm_mode_launch_info", None, dt, ctypes.byref(cap), None, None, None, None)[0] == _lib.SMM_OK
        assert cap.value == want
    slots = ctypes.c_int(0)
    rc, msg = status("smm_mode_launch_info", None, _lib.SMM_F32, None, ctypes.byref(slots), None, None, None)
    assert rc == _lib.SMM_ERR_INVALID and "null operator" in msg
    assert status("smm_mode_launch_info", None, _lib.SMM_F16, None, None, None, None, None)[0] == _lib.SMM_ERR_UNSUPPORTED


# ------------------------------------------------------------------ Regridder(categorical=...): refused before any device work

@pytest.fixture(scope="module")
def con_weights():
    return gridgen.generate_weights("r12x6", "r8x4", method="con")


@pytest.mark.parametrize("kw, word", [
    (dict(skipna=True), "skipna"), (dict(packed=True), "packed"), (dict(packed=True, packed_levels=True), "packed_levels"),
    (dict(packed=True, packed_out=True), "packed_out"), (dict(packed=True, packed_out=True, packed_out_levels=True), "packed_out_levels"),
    (dict(half=True), "half"), (dict(keep_batch_fastest=True), "keep_batch_fastest"), (dict(lazy=True), "lazy"),
    (dict(packed=True, grib_out=True), "grib_out"), (dict(packed=True, grib_out=True, grib_out_ccsds=True), "grib_out_ccsds"),
    (dict(packed=True, grib_out=True, grib_out_cpx=True), "grib_out_cpx"),
    (dict(packed=True, packed_levels=True, grib_out=True, grib_out_levels=True), "grib_out_levels"),
    (dict(packed=True, skipna=True, packed_skipna=True), "packed_skipna"),
    (dict(out_dtype=np.float32), "out_dtype=float32"), (dict(out_dtype=np.float64), "out_dtype=float64")])
@pytest.mark.parametrize("categorical", [True, ["lc"]])
def test_regridder_names_what_categorical_does_not_go_with(con_weights, kw, word, categorical):
    with pytest.raises(ValueError) as err:
        Regridder(weights=con_weights, categorical=categorical, **kw)
    text = str(err.value)
    assert "categorical does not go with" in text and word in text.split(":")[0] and "it goes with" in text


def test_regridder_refuses_gradients_beside_categorical():
    w = gridgen.generate_weights("r12x6", "r8x4", method="bic")
    with pytest.raises(ValueError, match="categorical does not go with gradients"):
        Regridder(weights=w, categorical=True, gradients=True)


def test_regridder_refuses_masked_level_weights():
    masks = gridgen.synthetic_ocean_masks(12, 6, 2)
    levels = [gridgen.generate_weights("r12x6", "r8x4", method="con", src_mask=m) for m in masks]
    w3d = gridgen.stack_level_weights(levels, [5.0, 50.0], method="con")
    with pytest.raises(ValueError, match=r"categorical does not go with masked-level \(3-D\) weights"):
        Regridder(weights=w3d, categorical=True)


def test_a_class_variables_road_refuses_raw_grib_batch_fastest_and_levels():
    s = road.Switches.of(categorical=True)
    dims = ("time", "lat", "lon")
    ok = road.decide(s, road.Facts("lc", road.HOST, np.uint8, dims, ("lat", "lon"), None, categorical=True))
    assert ok.refusal is None and ok.source == road.CLASS_CODES and ok.result == road.MODE and ok.out_dtype == np.uint8
    assert not ok.lines and not ok.after and not ok.gradients
    assert road.decide(s, road.Facts("lc", road.BS, np.int16, dims, ("lat", "lon"), None, categorical=True)).refusal is None
    for facts, word in ((road.Facts("lc", road.GRIB, np.float32, dims, ("lat", "lon"), None, categorical=True), "GribField"),
                        (road.Facts("lc", road.SB, np.float32, ("lat", "lon", "time"), ("lat", "lon"), None, categorical=True),
                         "layout='sb'"),
                        (road.Facts("lc", road.HOST, np.uint8, ("time", "lev", "lat", "lon"), ("lat", "lon"), "lev",
                                    categorical=True), "masked-level (3-D) weights")):
        stage, message = road.decide(s, facts).refusal
        assert stage == road.VARIABLE and "categorical does not go with" in message and word in message and "lc" in message


def test_the_switch_is_off_by_default_and_changes_no_other_road():
    assert road.Switches.of().categorical is False and road.refusal(road.Switches.of(categorical=True)) is None
    plain = road.Facts("tas", road.HOST, np.float32, ("time", "lat", "lon"), ("lat", "lon"), None)
    assert plain.categorical is False
    assert road.decide(road.Switches.of(categorical=True), plain) == road.decide(road.Switches.of(), plain)


def test_without_the_keyword_nothing_changes_in_the_constructor(con_weights):
    """categorical defaults to False: on a host without a device the constructor fails where it always did."""
    if _lib.device_count() > 0:
        pytest.skip("a device is present")
    with pytest.raises(_lib.SmmNoDeviceError):
        Regridder(weights=con_weights)
    for categorical in (True, ["lc"], (), False, None):      # valid: refused by the device, not by a check
        with pytest.raises(_lib.SmmNoDeviceError):
            Regridder(weights=con_weights, categorical=categorical)
