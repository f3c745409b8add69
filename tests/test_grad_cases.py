"""tests/grad_cases.py catches what it is for.  The numpy stand-in for the gradient stencil, in the kernel's own order,
equals `GradientRule` bit for bit on every seam case; with each named defect it differs on the grids where that defect
can show, on the very fields the GPU test hands the kernel; `GradientRule` equals the closed-form planes of a bilinear
field; and the gather fuzz's seed list reaches all 18 instantiations of smm_apply_cols_kernel."""
import numpy as np
import pytest

from smmregrid_amd.gradients import GRAD_I, GRAD_IJ, GRAD_J
from tests import grad_cases as gc
from tests.helpers import bits_equal

CASES = [(nx, ny, periodic, num_wgts) for nx, ny in gc.SEAM_GRIDS for periodic in (True, False) for num_wgts in (3, 4)]
IDS = [f"{nx}x{ny}-{'periodic' if p else 'regional'}-{k}" for nx, ny, p, k in CASES]


def fields(nx, ny):
    """The rows the GPU test uses at B = 3 (a NaN row and a NaN column on the seams among them), float32 and float64."""
    return [row for dt in (np.float32, np.float64) for row in gc.seam_batch(nx, ny, 3, dt)]


def differs(a, b):
    return not np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.mark.parametrize("nx,ny,periodic,num_wgts", CASES, ids=IDS)
def test_the_clean_standin_is_the_rule_and_every_defect_shows_where_it_can(nx, ny, periodic, num_wgts):
    for descending in (False, True):
        rule = gc.stretched_rule(nx, ny, periodic, num_wgts, descending)
        assert rule.periodic == periodic and rule.kind == ("sphere" if num_wgts == 3 else "index")
        t = rule.tables()
        if rule.kind == "sphere":      # every column and every row has a table entry of its own
            assert np.unique(t["si"][0, 1:-1]).size == nx - 2 and np.unique(t["sj"][0, 1:-1]).size == ny - 2
            assert t["ci"][0] == 0.0 and t["ci"][-1] == 0.0 and np.unique(t["ci"][1:-1]).size == ny - 2
        shown = {d: False for d in gc.DEFECTS}
        for f in fields(nx, ny):
            ref = rule.gradients(f)
            assert np.isfinite(ref).all()
            bits_equal(gc.standin(rule, f), ref)
            for d in gc.DEFECTS:
                got = differs(gc.standin(rule, f, d), ref)
                assert got <= gc.defect_shows(d, nx, ny, periodic, rule.kind), (d, "shows where it should not")
                shown[d] |= got
        for d in gc.DEFECTS:
            assert shown[d] == gc.defect_shows(d, nx, ny, periodic, rule.kind), d


def test_every_defect_is_caught_by_some_grid():
    for d in gc.DEFECTS:
        assert any(gc.defect_shows(d, nx, ny, p, "sphere" if k == 3 else "index") for nx, ny, p, k in CASES), d
    # the table of the issue, spelt out
    assert [nx for nx, ny in gc.SEAM_GRIDS if gc.defect_shows("body_no_wrap", nx, ny, True, "index")] == [255, 257, 258, 513, 257]
    assert not gc.defect_shows("ci_band_local", 513, 33, True, "sphere") and gc.defect_shows("ci_band_local", 258, 34, True, "sphere")
    assert not gc.defect_shows("si_tile_local", 513, 33, True, "index")


def test_the_seam_fields_put_finite_and_absent_cells_on_every_seam():
    for nx, ny in gc.SEAM_GRIDS:
        x = gc.seam_batch(nx, ny, 3, np.float32).reshape(3, ny, nx)
        plain = x[2] if ny > gc.BAND_ROWS else x[0]                      # no whole NaN row
        for r in {r for r in gc.SEAM_ROWS + (ny - 1,) if r < ny}:
            assert np.isfinite(plain[r]).sum() >= nx // 2 - 2
        plain = x[1] if nx > gc.TILE_X else x[0]                          # no whole NaN column
        for c in {c for c in gc.SEAM_COLS + (nx - 1,) if c < nx}:
            assert np.isfinite(plain[:, c]).sum() >= ny // 2 - 2
        assert not np.isfinite(x).all() and np.isinf(x).any() and np.isnan(x).any()
        if ny > gc.BAND_ROWS:
            assert np.isnan(x[0, gc.BAND_ROWS]).all() and np.isnan(x[1, gc.BAND_ROWS]).all()
        if nx > gc.TILE_X:
            assert np.isnan(x[0, :, gc.TILE_X]).all() and np.isnan(x[2, :, gc.TILE_X]).all()
    assert np.array_equal(gc.seam_batch(257, 33, 2, np.float64), gc.seam_batch(257, 33, 2, np.float64), equal_nan=True)


@pytest.mark.parametrize("nx,ny", gc.SEAM_GRIDS)
def test_the_rule_equals_the_closed_form_planes(nx, ny):
    for periodic in (True, False):
        for descending in (False, True):
            rule = gc.stretched_rule(nx, ny, periodic, 4, descending)
            assert rule.plane_kind == (GRAD_I, GRAD_J, GRAD_IJ)
            for a, b, c in ((3, 5, 2), (1, 1, 1)):
                want = gc.known_answer(nx, ny, periodic, descending, a, b, c)
                for dt in (np.float32, np.float64):
                    f = gc.known_field(nx, ny, a, b, c, dt)
                    assert np.array_equal(f.astype(np.float64), gc.known_field(nx, ny, a, b, c))      # exact
                    bits_equal(rule.gradients(f), want)
                    bits_equal(gc.standin(rule, f), want)


def test_known_answer_by_hand():
    g = gc.known_answer(4, 3, True, True, 3, 5, 2)        # f[j, i] = 3 i + 5 j + 2 i j
    assert g[0, 1].tolist() == [-5.0, 5.0, 5.0, -5.0]     # j = 1: a + c j = 5; the wrapped ends (0 - 3)/2 * 5 ... twice
    assert g[1, :, 2].tolist() == [-9.0, -9.0, -9.0] and g[2, 0].tolist() == [2.0, -2.0, -2.0, 2.0]
    g = gc.known_answer(4, 3, False, False, 3, 5, 2)
    assert g[0, 2].tolist() == [7.0] * 4 and g[1, 0].tolist() == [5.0, 7.0, 9.0, 11.0] and (g[2] == 2.0).all()


def test_one_plane_rule_picks_its_plane():
    rng = np.random.default_rng(3)
    for num_wgts in (3, 4):
        rule = gc.stretched_rule(12, 7, True, num_wgts)
        x = gc.seam_field(rng, 12, 7, np.float32).reshape(1, -1).repeat(2, axis=0)
        full, stacked = rule.gradients_rows(x), rule.stacked(x).reshape(2, rule.size, num_wgts)
        for kind in (GRAD_I, GRAD_J):
            one = gc.OnePlaneRule(rule, kind)
            at = rule.plane_kind.index(kind)
            assert (one.size, one.nx, one.ny, one.n_planes, one.plane_kind) == (84, 12, 7, 1, (kind,))
            bits_equal(one.gradients_rows(x), full[:, at:at + 1])
            bits_equal(one.gradients(x[0]), rule.gradients(x[0])[at:at + 1])
            s = one.stacked(x).reshape(2, rule.size, 2)
            bits_equal(s[:, :, 0], stacked[:, :, 0])
            bits_equal(s[:, :, 1], full[:, at])
    with pytest.raises(AssertionError):
        gc.OnePlaneRule(rule, GRAD_IJ)


def test_the_fuzz_seeds_reach_all_18_instantiations():
    draws = [gc.fuzz_draw(s) for s in gc.FUZZ_SEEDS]
    assert len(draws) == 24 and draws[5] == gc.fuzz_draw(5)
    by = {}
    for p in draws:
        for inst in sorted(gc.fuzz_instantiations(p)):
            by.setdefault(inst, p["seed"])
    assert sorted(by) == sorted(gc.INSTANTIATIONS) and len(gc.INSTANTIATIONS) == 18
    print({f"K={k} {dt} BT={bt}": s for (k, dt, bt), s in sorted(by.items())})
    # and every K with every field type in every batch class, as drawn
    classes = {(p["K"], p["dtype"], next(i for i, c in enumerate(gc.BATCH_CLASSES) if p["B"] in c)) for p in draws}
    assert len(classes) == 18
    for key, values in (("grid", gc.FUZZ_GRIDS), ("D", gc.FUZZ_D), ("links", ("random", "ragged")), ("masked", (False, True)),
                        ("area_min", (0.0, 0.25, 0.5, 0.9)), ("scratch_rows", (None, 1, 2, 3)), ("B", range(1, 10))):
        assert {p[key] for p in draws} >= set(values), key
    assert gc.fuzz_instantiations(dict(K=3, dtype="f32", B=7, scratch_rows=None)) == {(3, "f32", 4)}
    assert gc.fuzz_instantiations(dict(K=3, dtype="f32", B=7, scratch_rows=3)) == {(3, "f32", 2), (3, "f32", 1)}
