"""The row rule of the categorical apply that needs no device, in a stand-alone program under AddressSanitizer + UBSan
(tests/cpp/mode_harness.cpp): `mode_row` of smm_mode.hpp -- the function both forms of the kernel run -- compiled with
plain g++ -ffp-contract=off, against `categorical.ModeRule` on the cases of tests/mode_cases.py.  y and the share must be
identical bit for bit."""
import os
import subprocess

import numpy as np
import pytest

from tests import mode_cases as mc

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SOURCE = os.path.join(ROOT, "tests", "cpp", "mode_harness.cpp")
CODES = {"f32": 0, "f64": 1, "i16": 2, "u16": 3}


@pytest.fixture(scope="module")
def harness(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("mode") / "mode_harness_asan")
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-o", exe, SOURCE])
    return exe


def run(exe, tmp_path, op, x, kind, rule, masked, area_min):
    rowptr, col, val = op.csr
    fill = (list(rule.fill) + [0, 0])[:2]
    head = [op.n_dst, op.n_src, x.shape[0], x.shape[1], CODES[kind], len(rule.fill), fill[0], fill[1],
            rule.fill_out or 0, int(masked)]
    src, dst = str(tmp_path / "case.bin"), str(tmp_path / "out.bin")
    with open(src, "wb") as fh:
        fh.write(np.array(head, dtype=np.int64).tobytes())
        fh.write(np.array([area_min], dtype=np.float64).tobytes())
        for a, t in ((rowptr, np.int64), (col, np.int32), (val, np.float64), (op.imask, np.uint8), (op.frac, np.float64)):
            fh.write(np.ascontiguousarray(a, dtype=t).tobytes())
        fh.write(np.ascontiguousarray(x).tobytes())
    out = subprocess.run([exe, src, dst], capture_output=True, text=True, timeout=300,
                         env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1"))
    assert out.returncode == 0, (out.stdout + out.stderr)[-3000:]
    raw = open(dst, "rb").read()
    n = x.shape[0] * op.n_dst
    y = np.frombuffer(raw, dtype=x.dtype, count=n).reshape(x.shape[0], op.n_dst)
    share = np.frombuffer(raw, dtype=np.float64, count=n, offset=n * x.dtype.itemsize).reshape(x.shape[0], op.n_dst)
    return y, share


@pytest.mark.parametrize("kind", mc.DTYPES)
@pytest.mark.parametrize("D", [1, 65, 257])
def test_the_header_rule_matches_numpy_bit_for_bit(harness, tmp_path, D, kind):
    op = mc.operator(D, seed=7)
    x, rule = mc.checked_field(op, 3, kind, n_classes=5, n_fill=2, seed=8, pitch=4)
    for masked, area_min in ((False, 0.0), (True, 0.3), (True, 0.9)):
        y, share = run(harness, tmp_path, op, x, kind, rule, masked, area_min)
        want_y, want_share = rule.apply(op.csr, x, masked=masked, dst_imask=op.imask, dst_frac=op.frac,
                                        remap_area_min=area_min)
        mc.assert_bits(y, want_y, f"y masked={masked} area_min={area_min}")
        mc.assert_bits(share, want_share, f"share masked={masked} area_min={area_min}")


@pytest.mark.parametrize("n_classes, n_fill", [(1, 1), (2, 0), ("own", 1)])
def test_one_class_no_fill_and_every_cell_its_own_class(harness, tmp_path, n_classes, n_fill):
    op = mc.operator(65, seed=9)
    for kind in ("i16", "f32"):
        x, rule = mc.checked_field(op, 2, kind, n_classes=n_classes, n_fill=n_fill, seed=10)
        y, share = run(harness, tmp_path, op, x, kind, rule, True, 0.3)
        want_y, want_share = rule.apply(op.csr, x, masked=True, dst_imask=op.imask, dst_frac=op.frac, remap_area_min=0.3)
        mc.assert_bits(y, want_y, f"{kind} y")
        mc.assert_bits(share, want_share, f"{kind} share")
