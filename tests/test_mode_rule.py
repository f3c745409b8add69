"""`categorical.ModeRule` -- the numpy statement of largest-area-fraction regridding -- against an independent statement
built from the C oracle's plain apply on indicator fields (tests/mode_cases.py: shares bit for bit, the winner by argmax
with the first-link tie-break taken from the CSR), against answers written out by hand, and the coverage of the cases
the GPU tests use.  No device."""
import numpy as np
import pytest

from smmregrid_amd import ModeRule
from tests import mode_cases as mc


def one_row(weights, values, **kw):
    """(y, share) of a single destination row whose links go to source cells 0 .. n-1."""
    w = np.asarray(weights, dtype=np.float64)
    csr = (np.array([0, w.size]), np.arange(w.size, dtype=np.int32), w)
    x = np.asarray(values)[None, :]
    rule = kw.pop("rule", ModeRule())
    y, share = rule.apply(csr, x, **kw)
    return y[0, 0], share[0, 0]


# ------------------------------------------------------------------ known answers

def test_ten_links_of_nine_percent_beat_one_of_ten():
    y, share = one_row([0.10] + [0.09] * 10, np.array([7.0] + [3.0] * 10, dtype=np.float32))
    want = 0.0
    for _ in range(10):
        want += 0.09
    assert y == 3.0 and y.dtype == np.float32 and share == want


def test_a_two_against_two_tie_goes_to_the_first_links_class():
    assert one_row([0.25] * 4, np.array([5, 9, 5, 9], dtype=np.float64)) == (5.0, 0.5)
    assert one_row([0.25] * 4, np.array([9, 5, 5, 9], dtype=np.float64)) == (9.0, 0.5)
    assert one_row([0.25] * 4, np.array([9, 5, 5, 9], dtype=np.int16), rule=ModeRule((), -1)) == (9, 0.5)


def test_a_class_reached_through_zero_weight_links_cannot_win():
    assert one_row([0.0, 0.0, 0.3], np.array([4.0, 4.0, 6.0])) == (6.0, 0.3)
    y, share = one_row([0.0, 0.0], np.array([4.0, 4.0]))
    assert np.isnan(y) and share == 0.0 and not np.signbit(share)
    y, share = one_row([0.0, -0.5], np.array([4, 6], dtype=np.uint16), rule=ModeRule((), 65535))
    assert y == 65535 and share == 0.0


def test_signed_zeros_are_one_class_and_the_first_links_sign_is_kept():
    y, share = one_row([0.2, 0.3, 0.4], np.array([-0.0, 1.0, 0.0]))
    assert y == 0.0 and np.signbit(y) and share == 0.2 + 0.4
    y, share = one_row([0.2, 0.3, 0.4], np.array([0.0, 1.0, -0.0], dtype=np.float32))
    assert y == 0.0 and not np.signbit(y)


def test_non_finite_floats_and_integer_fills_drop_out():
    y, share = one_row([0.5, 0.5, 0.5, 0.1], np.array([np.nan, np.inf, -np.inf, 2.0]))
    assert (y, share) == (2.0, 0.1)
    y, share = one_row([0.4, 0.4, 0.1], np.array([np.inf, np.inf, 2.0]))      # inf == inf, and still no class
    assert (y, share) == (2.0, 0.1)
    rule = ModeRule((-32768, -1), -32768)
    assert one_row([0.5, 0.5, 0.1], np.array([-32768, -1, 2], dtype=np.int16), rule=rule) == (2, 0.1)
    assert one_row([0.5, 0.5], np.array([-32768, -1], dtype=np.int16), rule=rule) == (-32768, 0.0)
    one = ModeRule((-32768,))                                                 # only the first n_fill entries count
    assert one_row([0.5, 0.3, 0.1], np.array([-32768, -1, 2], dtype=np.int16), rule=one) == (-1, 0.3)
    assert one.checked(np.int16) == ((-32768,), -32768)                       # fill_out: the first fill


def test_the_area_test_uses_the_valid_fraction_of_the_weight():
    kw = dict(dst_frac=np.array([0.5]), remap_area_min=0.3)
    assert one_row([0.5, 0.5], np.array([1.0, 1.0]), **kw)[0] == 1.0          # 0.5 * (1 / 1) >= 0.3
    y, share = one_row([0.5, 0.25, 0.25], np.array([np.nan, 1.0, 1.0]), **kw)  # 0.5 * (0.5 / 1) < 0.3
    assert np.isnan(y) and share == 0.0
    assert one_row([0.5, 0.25, 0.25], np.array([np.nan, 1.0, 1.0]), dst_frac=np.array([0.5]))[0] == 1.0
    y, _ = one_row([1.0, -1.0, 0.5], np.array([1.0, 2.0, 1.0]), **kw)         # tot 0.5, val 0.5
    assert y == 1.0
    assert one_row([1.0, -1.0], np.array([1.0, 2.0]), **kw)[0] == 1.0         # 0 / 0: NaN compares false, the row lives


def test_a_masked_row_is_dead_and_a_row_without_links_too():
    kw = dict(masked=True, dst_imask=np.array([0]))
    y, share = one_row([0.5], np.array([1.0]), **kw)
    assert np.isnan(y) and share == 0.0
    assert one_row([0.5], np.array([1.0]), masked=True, dst_imask=np.array([1])) == (1.0, 0.5)
    y, share = one_row([], np.zeros(0))
    assert np.isnan(y) and share == 0.0


def test_the_rule_refuses_what_does_not_fit():
    with pytest.raises(ValueError, match="at most two"):
        ModeRule((1, 2, 3))
    with pytest.raises(ValueError, match="no value of uint16"):
        ModeRule((-1,)).checked(np.uint16)
    with pytest.raises(ValueError, match="no value of int16"):
        ModeRule((1,), 40000).checked(np.int16)
    with pytest.raises(ValueError, match="needs fill_out"):
        ModeRule().checked(np.int16)
    with pytest.raises(ValueError, match="float class field takes no fill"):
        ModeRule((1,)).checked(np.float32)
    with pytest.raises(TypeError, match="int16"):
        ModeRule((1,)).checked(np.dtype("U4"))
    with pytest.raises(ValueError, match="dst_frac"):
        one_row([1.0], np.array([1.0]), remap_area_min=0.3)
    with pytest.raises(ValueError, match="dst_imask"):
        one_row([1.0], np.array([1.0]), masked=True)


def test_from_attrs_takes_fill_value_then_missing_value():
    rule, found = ModeRule.from_attrs({"_FillValue": np.uint8(255), "missing_value": np.uint8(0)}, np.uint8)
    assert found and rule.fill == (255, 0) and rule.fill_out == 255
    rule, found = ModeRule.from_attrs({"missing_value": -9, "_FillValue": -9}, np.int16)
    assert found and rule.fill == (-9,) and rule.fill_out == -9
    rule, found = ModeRule.from_attrs({}, np.int16)
    assert not found and rule.fill == (-32768,) and rule.fill_out == -32768
    rule, found = ModeRule.from_attrs({}, np.uint8)
    assert not found and rule.fill_out == 255
    rule, found = ModeRule.from_attrs({"_FillValue": np.nan}, np.float32)
    assert found and rule.fill == () and rule.fill_out is None


# ------------------------------------------------------------------ against the indicator statement

@pytest.mark.parametrize("area_min", mc.AREA_MINS)
@pytest.mark.parametrize("masked", [False, True])
@pytest.mark.parametrize("kind", mc.DTYPES)
def test_the_rule_equals_the_indicator_statement(kind, masked, area_min):
    op = mc.operator(65, seed=1)
    x, rule = mc.checked_field(op, 3, kind, n_classes=5, n_fill=2, seed=2)
    y, share = rule.apply(op.csr, x, masked=masked, dst_imask=op.imask, dst_frac=op.frac, remap_area_min=area_min)
    want_y, want_share = mc.indicator_statement(op, x, rule, masked, area_min)
    mc.assert_bits(y, want_y, "y")
    mc.assert_bits(share, want_share, "share")
    assert y.dtype == x.dtype and share.dtype == np.float64


@pytest.mark.parametrize("n_classes, n_fill", [(1, 1), (2, 0), (2, 1), (5, 2), ("own", 1)])
def test_fields_of_few_many_and_all_distinct_classes(n_classes, n_fill):
    op = mc.operator(63, seed=3)
    for kind in ("u16", "f32"):
        x, rule = mc.checked_field(op, 2, kind, n_classes=n_classes, n_fill=n_fill, seed=4, pitch=5)
        y, share = rule.apply(op.csr, x, masked=True, dst_imask=op.imask, dst_frac=op.frac, remap_area_min=0.3)
        want_y, want_share = mc.indicator_statement(op, x, rule, True, 0.3)
        mc.assert_bits(y, want_y, f"{kind} y")
        mc.assert_bits(share, want_share, f"{kind} share")


def test_planted_rows_give_their_written_answers():
    op = mc.operator(16, seed=0)
    x, rule = mc.field(op, 2, "u16", n_classes=5, n_fill=1)
    classes = mc.CLASSES["u16"]
    for area_min, masked in ((0.0, False), (0.3, True)):
        y, share = rule.apply(op.csr, x, masked=masked, dst_imask=op.imask, dst_frac=op.frac, remap_area_min=area_min)
        for b in range(2):
            a = classes[b % 5]
            dead = rule.fill_out
            hard = area_min > 0
            assert y[b, 0] == a and share[b, 0] == 0.5
            assert (y[b, 1], share[b, 1]) == ((dead, 0.0) if hard else (a, 0.5))
            assert y[b, 2] == a and share[b, 2] > 0.89
            assert [y[b, d] for d in (3, 4, 5)] == [dead] * 3 and not share[b, 3:6].any()
            assert y[b, 6] == (dead if masked else a)
            assert y[b, 7] == (dead if hard else a)
            assert (y[b, 8], share[b, 8]) == (a, 0.3)


# ------------------------------------------------------------------ the cases of the GPU tests cover what they must

def test_the_gpu_cases_cover_ties_missing_links_dead_rows_and_light_winners():
    from tests import test_gpu_mode as tg
    n = 0
    for D, B, kind, kw in tg.host_cases():
        op = mc.operator(D, seed=tg.SEED)
        x, rule = mc.field(op, B, kind, **kw)
        got = mc.coverage(op, x, rule)
        need = mc.required(op, x, rule)
        assert all(got[k] >= 1 for k in need), (D, B, kind, kw, got)
        if D >= mc.N_PLANTED and kw.get("n_classes", 5) != 1 and (kind[0] == "f" or kw.get("n_fill", 1)):
            assert set(need) == set(got), (D, kind, kw)      # nothing is excused in an ordinary case
        n += 1
    assert n >= 20
