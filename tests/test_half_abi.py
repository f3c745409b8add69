"""Half-precision fields and results on the host side (no device needed): the header's dtype codes and their ctypes /
numpy twins, `bfloat16` / `to_bfloat16` / `from_bfloat16`, the test suite's own rounding against exact rational
arithmetic, and the keywords."""
import inspect
import os
import re

import numpy as np
import pytest

from tests import half_cases as hc
import smmregrid_amd
from smmregrid_amd import DeviceArray, Regridder, SparseOperator, OperatorGroup, _lib, bfloat16, from_bfloat16, to_bfloat16
from smmregrid_amd import device

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        return f.read()


def test_header_ctypes_table_and_numpy_names_agree_on_the_half_codes():
    text = _header()
    u16 = int(re.search(r"\bSMM_U16\s*=\s*(\d+)", text).group(1))
    codes = {m.group(1): u16 + int(m.group(2)) for m in re.finditer(r"\b(SMM_B?F16)\s*=\s*SMM_U16\s*\+\s*(\d+)", text)}
    assert codes == {"SMM_F16": 4, "SMM_BF16": 5}                # the two codes after SMM_U16
    assert (_lib.SMM_F16, _lib.SMM_BF16) == (4, 5)
    assert device.dtype_code(np.float16) == _lib.SMM_F16 and device.dtype_code(bfloat16) == _lib.SMM_BF16
    assert device.dtype_code(np.float32) == _lib.SMM_F32 and device.dtype_code(np.float64) == _lib.SMM_F64
    assert re.search(r"#define\s+SMM_ABI_VERSION\s+6\b", text)   # codes are only added: no new entry, no new struct
    with pytest.raises(TypeError):
        device.dtype_code(np.int32)


def test_bfloat16_is_a_two_byte_numpy_dtype():
    assert isinstance(bfloat16, np.dtype) and bfloat16.itemsize == 2 and bfloat16 != np.dtype(np.uint16)
    a = np.empty((3, 5), bfloat16)
    assert a.nbytes == 30
    bits = np.arange(6, dtype=np.uint16).reshape(2, 3)
    assert np.array_equal(bits.view(bfloat16).view(np.uint16), bits)
    assert device.is_half_dtype(bfloat16) and device.is_half_dtype(np.float16) and not device.is_half_dtype(np.float32)
    for name in ("bfloat16", "to_bfloat16", "from_bfloat16"):
        assert name in smmregrid_amd.__all__


def test_bfloat16_round_trip_of_every_pattern():
    bits = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    f = from_bfloat16(bits.view(bfloat16))
    assert f.dtype == np.float32
    assert np.array_equal(f.view(np.uint32), bits.astype(np.uint32) << 16)           # exact: the upper half of a float32
    nan = np.isnan(f)
    assert nan.sum() == 2 * 127
    for src in (f, f.astype(np.float64)):                                            # from float32 and from float64
        back = to_bfloat16(src)
        assert back.dtype == bfloat16 and back.shape == src.shape
        back = back.view(np.uint16)
        assert np.array_equal(back[~nan], bits[~nan])
        assert np.isnan(from_bfloat16(back[nan])).all()                              # NaN by class


@pytest.mark.parametrize("kind", ["f16", "bf16"])
def test_the_tests_own_rounding_is_exact(kind):
    """`half_cases.round_bits` (integer arithmetic on the float64 bits) against Fraction arithmetic; for float16 numpy's
    own conversion agrees too."""
    vals = hc.adversarial(kind)
    got = hc.round_bits(vals, kind)
    want = np.array([hc.exact_bits(float(v), kind) for v in vals], dtype=np.uint16)
    assert np.array_equal(got, want), [(float(v), hex(g), hex(w)) for v, g, w in zip(vals, got, want) if g != w][:5]
    if kind == "f16":
        with np.errstate(over="ignore"):
            np16 = vals.astype(np.float16).view(np.uint16)
        ok = ~np.isnan(vals)
        assert np.array_equal(got[ok], np16[ok])
    one = {"f16": (1 + 2.0 ** -11 + 2.0 ** -40, 0x3C01), "bf16": (1 + 2.0 ** -8 + 2.0 ** -40, 0x3F81)}[kind]
    assert int(hc.round_bits(np.array([one[0]]), kind)[0]) == one[1]
    # the float32 detour this guards against really gives 1.0
    detour = hc.round_bits(np.array([one[0]], np.float64).astype(np.float32).astype(np.float64), kind)[0]
    assert int(detour) == {"f16": 0x3C00, "bf16": 0x3F80}[kind]


def test_to_bfloat16_rounds_to_nearest_even_from_the_inputs_own_precision():
    vals = hc.adversarial("bf16")
    want = np.array([hc.exact_bits(float(v), "bf16") for v in vals], dtype=np.uint16)
    got = to_bfloat16(vals).view(np.uint16)
    nan = np.isnan(vals)
    assert np.array_equal(got[~nan], want[~nan])
    assert np.isnan(from_bfloat16(got[nan])).all()
    with np.errstate(over="ignore"):
        v32 = vals.astype(np.float32)                 # from float32: exact for what float32 holds
    want32 = np.array([hc.exact_bits(float(v), "bf16") for v in v32], dtype=np.uint16)
    got32 = to_bfloat16(v32).view(np.uint16)
    assert np.array_equal(got32[~nan], want32[~nan])
    rng = np.random.default_rng(7)
    r = rng.standard_normal(20000) * 10.0 ** rng.integers(-45, 39, size=20000)
    assert np.array_equal(to_bfloat16(r).view(np.uint16), hc.round_bits(r, "bf16"))
    assert np.array_equal(to_bfloat16(np.float16([1.5, -2.0])).view(np.uint16), np.array([0x3FC0, 0xC000], np.uint16))
    with pytest.raises(TypeError):
        to_bfloat16(np.arange(3))
    with pytest.raises(TypeError):
        from_bfloat16(np.zeros(3, np.float32))


def test_keywords_and_refusals_that_need_no_device():
    assert inspect.signature(Regridder.__init__).parameters["half"].default is False
    for fn in (SparseOperator.apply_host, OperatorGroup.apply_host):
        assert inspect.signature(fn).parameters["half"].default is False
    assert hasattr(DeviceArray, "from_interface")
    with pytest.raises(ValueError, match="out_dtype must be float32 or float64"):
        Regridder(weights=None, source_grid="x", target_grid="y", out_dtype=np.int16)
    with pytest.raises(TypeError) as err:
        device.check_half_pair(np.float16, bfloat16)
    for pair in ("float16 -> float64", "float16 -> float16", "bfloat16 -> float64", "bfloat16 -> bfloat16",
                 "float32 -> float16", "float64 -> float16", "float32 -> bfloat16", "float64 -> bfloat16"):
        assert pair in str(err.value)
    with pytest.raises(TypeError):
        device.check_half_pair(np.float16, np.float32)
    for x, y in device.HALF_PAIRS:
        device.check_half_pair(x, y)
    assert len(device.HALF_PAIRS) == 8

    class Fake:
        __cuda_array_interface__ = {"shape": (2, 3), "typestr": "<i4", "data": (4096, False), "version": 2}
    with pytest.raises(TypeError):
        DeviceArray.from_interface(Fake())
    with pytest.raises(TypeError):
        DeviceArray.from_interface(object())
    Fake.__cuda_array_interface__ = {"shape": (2, 3), "typestr": "<f2", "data": (4096, False), "version": 2,
                                     "strides": (2, 4)}
    with pytest.raises(ValueError):
        DeviceArray.from_interface(Fake())
    Fake.__cuda_array_interface__["strides"] = (6, 2)
    obj = Fake()
    view = DeviceArray.from_interface(obj)
    assert view.shape == (2, 3) and view.dtype == np.float16 and view.ptr == 4096 and view.base is obj
    view.free()                                       # a view: nothing is released
