"""SMM_APPLY_SKIPNA on the host side: the header's bit, its Python twin and the keyword on every apply entry
(no device needed)."""
import inspect
import os
import re

from smmregrid_amd import OperatorGroup, Regridder, SparseOperator, _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _header_flags():
    with open(os.path.join(ROOT, "include", "smmregrid_amd.h")) as f:
        text = f.read()
    return {m.group(1): int(m.group(2)) for m in re.finditer(r"(SMM_APPLY_\w+)\s*=\s*1u\s*<<\s*(\d+)", text)}


def test_header_defines_skipna_at_bit_6():
    flags = _header_flags()
    assert flags["SMM_APPLY_SKIPNA"] == 6
    bits = list(flags.values())
    assert len(bits) == len(set(bits)), "two apply flags share a bit"
    assert 5 not in bits


def test_python_flag_matches_header():
    assert _lib.APPLY_SKIPNA == 1 << _header_flags()["SMM_APPLY_SKIPNA"] == 64


def test_apply_entries_take_skipna():
    for cls in (SparseOperator, OperatorGroup):
        for name in ("apply", "apply_sb", "apply_host"):
            p = inspect.signature(getattr(cls, name)).parameters
            assert "skipna" in p and p["skipna"].default is False, f"{cls.__name__}.{name}"
    p = inspect.signature(Regridder.__init__).parameters
    assert "skipna" in p and p["skipna"].default is False
