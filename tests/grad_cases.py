"""Inputs that put the gradient stencil (smm_gradients_kernel) and the K-column gather (smm_apply_cols_kernel) on their
seams, for tests/test_gpu_gradients_seams.py and tests/test_gpu_gradients_far_offsets.py, and a numpy stand-in for the
stencil in the kernel's own order, with which tests/test_grad_cases.py shows that these inputs catch what they are for.
Plain numpy, no GPU (only `OnePlaneRule.plan` touches the library).

The stencil walks tiles of 256 columns and bands of 32 rows; a workgroup fills a window of (rows + 2) x 258 cells -- slot x
of a window row holds column i0 + x - 1, slots 1 .. 256 filled by the lanes, slots 0 and 257 by two halo lanes -- and takes
five differences on it.  `SEAM_GRIDS` lie just around one and two tiles and bands; `stretched_rule` gives every column
and every row a table entry of its own, so that an index taken within the tile or the band reads another value."""
import ctypes

import numpy as np

from smmregrid_amd.gradients import GRAD_I, GRAD_IJ, GRAD_J, GradientRule

TILE_X, BAND_ROWS = 256, 32
SEAM_GRIDS = ((255, 31), (256, 32), (257, 33), (258, 34), (513, 33), (257, 65), (512, 64))
SEAM_COLS = (0, 255, 256, 257, 511, 512)
SEAM_ROWS = (0, 31, 32, 33, 63, 64)
SEED = 20261021

DEFECTS = ("halo_no_wrap", "body_no_wrap", "seam_halo_absent", "band_top_absent", "band_bottom_absent", "si_tile_local",
           "sj_band_local", "ci_band_local", "cross_presence_on_gj")


# ------------------------------------------------------------------ grids and fields

def stretched_rule(nx, ny, periodic, num_wgts, descending=False):
    """A rule on a stretched grid: cell widths drawn from [0.6, 1.4], normalised to the circle (70 degrees when
    regional) in longitude and to pole-to-pole in latitude; the first and last row on the poles when ny > 2.  The
    seed is fixed per (nx, ny)."""
    rng = np.random.default_rng([SEED, nx, ny])
    wx, wy = rng.uniform(0.6, 1.4, nx), rng.uniform(0.6, 1.4, ny)
    wx *= (2.0 * np.pi if periodic else np.radians(70.0)) / wx.sum()
    wy *= np.pi / wy.sum()
    lon = np.cumsum(wx) - 0.5 * wx
    lat = -0.5 * np.pi + np.cumsum(wy) - 0.5 * wy
    if ny > 2:
        lat[0], lat[-1] = -0.5 * np.pi, 0.5 * np.pi
    return GradientRule(lon, lat[::-1].copy() if descending else lat, num_wgts, periodic=periodic)


def seam_field(rng, nx, ny, dtype):
    """(ny, nx): a rough field with 4 % NaN / +inf / -inf; every second cell of the seam columns and seam rows is
    redrawn finite, so that finite and absent neighbours both sit on every seam."""
    x = (250.0 + 30.0 * rng.standard_normal((ny, nx))).astype(dtype)
    bad = rng.random(x.shape) < 0.04
    x[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf]), size=int(bad.sum())).astype(dtype)
    for c in sorted({c for c in SEAM_COLS + (nx - 1,) if c < nx}):
        x[c % 2::2, c] = (250.0 + 30.0 * rng.standard_normal(x[c % 2::2, c].shape)).astype(dtype)
    for r in sorted({r for r in SEAM_ROWS + (ny - 1,) if r < ny}):
        x[r, r % 2::2] = (250.0 + 30.0 * rng.standard_normal(x[r, r % 2::2].shape)).astype(dtype)
    return x


def seam_batch(nx, ny, n_batch, dtype):
    """(n_batch, ny * nx): the batch the GPU test hands the stencil, the same on every call.  Row 0 carries a whole NaN
    row 32 and a whole NaN column 256 where the grid has them, row 1 the NaN row alone, row 2 the NaN column alone."""
    rng = np.random.default_rng([SEED, nx, ny, n_batch, np.dtype(dtype).itemsize])
    x = np.stack([seam_field(rng, nx, ny, dtype) for _ in range(n_batch)])
    for b in range(n_batch):
        if b % 3 != 2 and ny > BAND_ROWS:
            x[b, BAND_ROWS, :] = np.nan
        if b % 3 != 1 and nx > TILE_X:
            x[b, :, TILE_X] = np.nan
    return x.reshape(n_batch, -1)


# ------------------------------------------------------------------ the stencil restated in the kernel's order

def _window(f, nx, ny, periodic, j0, j1, i0, defect):
    """The (j1 - j0 + 2) x 258 cells a workgroup stages: rows j0 - 1 .. j1, columns i0 - 1 .. i0 + 256, by the kernel's
    rule for one cell -- the load index clamped into the grid, a periodic grid wrapping column -1 and column nx, NaN for
    everything else outside."""
    j = np.arange(j0 - 1, j1 + 1)[:, None]
    gc = np.arange(i0 - 1, i0 + TILE_X + 1)[None, :]
    halo = np.zeros(gc.shape, bool)
    halo[0, 0] = halo[0, -1] = True
    inside = (j >= 0) & (j < ny)
    out = (gc < 0) | (gc >= nx)
    wraps = bool(periodic) & ((gc == -1) | (gc == nx))
    if defect == "halo_no_wrap":
        wraps = wraps & ~halo
    if defect == "body_no_wrap":
        wraps = wraps & halo
    present = inside & (~out | wraps)
    if defect == "seam_halo_absent":
        present = present & ~(halo & ~out)
    if defect == "band_top_absent" and j0 > 0:
        present = present & (j != j0 - 1)
    if defect == "band_bottom_absent" and j1 < ny:
        present = present & (j != j1)
    c = np.where(out, np.where(gc < 0, nx - 1, 0), gc)
    jc = np.clip(j, 0, ny - 1)
    return np.where(present, f[jc, c], np.nan)


def _diff(fc, fp, fm, vc, vp, vm, s, idx, m):
    """grad_diff of the kernel: presence on f, values from v, one rounded operation a line."""
    pp, pm = np.isfinite(fp), np.isfinite(fm)
    ok = np.isfinite(fc) & (pp | pm)
    hi, lo = np.where(pp, vp, vc), np.where(pm, vm, vc)
    code = np.where(pp & pm, 0, np.where(pp, 1, 2))
    with np.errstate(invalid="ignore", over="ignore"):
        d = hi - lo
        ds = d * s[code, idx]
        dm = ds * m
    return np.where(ok, dm, 0.0)


def standin(rule, f, defect=None):
    """`rule.gradients(f)` by the kernel's road: block by block of 256 x 32 cells, the window, then the five
    differences on it.  `defect` names one way in which a kernel could be wrong (DEFECTS)."""
    assert defect is None or defect in DEFECTS, defect
    nx, ny = rule.nx, rule.ny
    t = rule.tables()
    si, sj, ci = t["si"], t["sj"], t["ci"]
    f = np.asarray(f).reshape(ny, nx).astype(np.float64)
    planes = {k: np.zeros((ny, nx)) for k in (GRAD_I, GRAD_J, GRAD_IJ)}
    for j0 in range(0, ny, BAND_ROWS):
        j1 = min(ny, j0 + BAND_ROWS)
        for i0 in range(0, nx, TILE_X):
            W = _window(f, nx, ny, rule.periodic, j0, j1, i0, defect)
            n = min(TILE_X, nx - i0)                       # lanes with i < nx
            C, P, M = W[1:-1], W[2:], W[:-2]
            mid, east, west = slice(1, 1 + n), slice(2, 2 + n), slice(0, n)
            fc, fe, fw = C[:, mid], C[:, east], C[:, west]
            i_idx = (np.arange(n) if defect == "si_tile_local" else np.arange(i0, i0 + n))[None, :]
            j_idx = (np.arange(j1 - j0) if defect == "sj_band_local" else np.arange(j0, j1))[:, None]
            cij = ci[np.arange(j1 - j0) if defect == "ci_band_local" else np.arange(j0, j1)][:, None]
            gi = _diff(fc, fe, fw, fc, fe, fw, si, i_idx, cij)
            gj = _diff(fc, P[:, mid], M[:, mid], fc, P[:, mid], M[:, mid], sj, j_idx, 1.0)
            gj_e = _diff(fe, P[:, east], M[:, east], fe, P[:, east], M[:, east], sj, j_idx, 1.0)
            gj_w = _diff(fw, P[:, west], M[:, west], fw, P[:, west], M[:, west], sj, j_idx, 1.0)
            if defect == "cross_presence_on_gj":
                gij = _diff(gj, gj_e, gj_w, gj, gj_e, gj_w, si, i_idx, cij)
            else:
                gij = _diff(fc, fe, fw, gj, gj_e, gj_w, si, i_idx, cij)
            for kind, v in ((GRAD_I, gi), (GRAD_J, gj), (GRAD_IJ, gij)):
                planes[kind][j0:j1, i0:i0 + n] = v
    return np.stack([planes[k] for k in rule.plane_kind], axis=0)


def defect_shows(defect, nx, ny, periodic, kind):
    """Whether `defect` changes a bit of the planes on a grid of SEAM_GRIDS with the fields above."""
    return {"halo_no_wrap": periodic,
            "body_no_wrap": periodic and nx % TILE_X != 0,
            "seam_halo_absent": nx > TILE_X,
            "band_top_absent": ny > BAND_ROWS,
            "band_bottom_absent": ny > BAND_ROWS,
            "si_tile_local": kind == "sphere" and nx > TILE_X,
            "sj_band_local": kind == "sphere" and ny > BAND_ROWS,
            # ny = 33: the lone row of band 1 is a pole row, ci = 0 like row 0
            "ci_band_local": kind == "sphere" and ny >= BAND_ROWS + 2,
            "cross_presence_on_gj": kind == "index"}[defect]


# ------------------------------------------------------------------ known answers

def known_field(nx, ny, a, b, c, dtype=np.float64):
    """f[j, i] = a i + b j + c i j, exact in float32 and float64 for the small integers used."""
    j, i = np.arange(ny)[:, None], np.arange(nx)[None, :]
    f = a * i + b * j + c * i * j
    assert np.abs(f).max() < 1 << 24
    return f.astype(dtype)


def known_answer(nx, ny, periodic, descending, a, b, c):
    """The index-kind planes (g_i, g_j, g_ij) of `known_field`, (3, ny, nx), written out region by region.  a, b, c
    positive, so that no entry is a zero whose sign would have to be argued."""
    assert nx >= 3 and ny >= 3 and min(a, b, c) > 0
    sign = -1.0 if descending else 1.0
    j, i = np.arange(ny, dtype=np.float64)[:, None], np.arange(nx, dtype=np.float64)[None, :]
    gi, gj, gij = np.empty((ny, nx)), np.empty((ny, nx)), np.empty((ny, nx))
    # d/di.  Interior: (f[j, i + 1] - f[j, i - 1]) / 2 = a + c j.
    gi[:, 1:-1] = np.broadcast_to(a + c * j, (ny, nx))[:, 1:-1]
    if periodic:      # both neighbours present, one of them across the seam: (f[j, 1] - f[j, nx - 1]) / 2 and its mirror
        gi[:, 0] = ((a + c * j) * (1.0 - (nx - 1.0)) * 0.5)[:, 0]
        gi[:, -1] = ((a + c * j) * (0.0 - (nx - 2.0)) * 0.5)[:, 0]
    else:             # one-sided: f[j, 1] - f[j, 0] and f[j, nx - 1] - f[j, nx - 2]
        gi[:, 0] = gi[:, -1] = (a + c * j)[:, 0]
    # d/dj, signed towards increasing latitude.  Interior: (f[j + 1, i] - f[j - 1, i]) / 2 = b + c i.
    gj[1:-1] = sign * (b + c * i)
    gj[0] = (sign * (b + c * i))[0]          # one-sided, first row: f[1, i] - f[0, i]
    gj[-1] = (sign * (b + c * i))[0]         # one-sided, last row: f[ny - 1, i] - f[ny - 2, i]
    # d/di of g_j, which is sign (b + c i) in every row
    gij[:, 1:-1] = sign * c
    if periodic:
        gij[:, 0] = sign * c * (1.0 - (nx - 1.0)) * 0.5
        gij[:, -1] = sign * c * (0.0 - (nx - 2.0)) * 0.5
    else:
        gij[:, 0] = gij[:, -1] = sign * c
    return np.stack([gi, gj, gij], axis=0)


# ------------------------------------------------------------------ one plane: the road to K = 2

class OnePlaneRule:
    """One plane (GRAD_I or GRAD_J; neither depends on another plane) of a full rule, as a rule of its own: what a
    weights matrix of two columns goes with.  Duck-typed for `SparseOperator.gradients` / `.apply(gradients=)`."""

    def __init__(self, rule, kind):
        assert kind in (GRAD_I, GRAD_J) and kind in rule.plane_kind
        self.full, self.kind_of_plane = rule, kind
        self.size, self.nx, self.ny = rule.size, rule.nx, rule.ny
        self.n_planes, self.plane_kind = 1, (kind,)
        self._at = rule.plane_kind.index(kind)
        self._plans = {}

    def tables(self):
        return self.full.tables()

    def gradients(self, field2d):
        return self.full.gradients(field2d)[self._at:self._at + 1]

    def gradients_rows(self, x):
        return np.ascontiguousarray(self.full.gradients_rows(x)[:, self._at:self._at + 1])

    def stacked(self, x):
        K = self.full.n_planes + 1
        X = self.full.stacked(x).reshape(np.asarray(x).shape[0], self.size, K)
        return np.ascontiguousarray(X[:, :, [0, 1 + self._at]]).reshape(X.shape[0], -1)

    def plan(self, device):
        device = int(device)
        if device not in self._plans:
            self._plans[device] = create_plan(self.full.tables(), (self.kind_of_plane,), device)
        return self._plans[device]

    def __del__(self):
        try:
            from smmregrid_amd import _lib
            for h in self._plans.values():
                _lib.call("smm_grad_plan_destroy", h)
            self._plans = {}
        except Exception:
            pass


def create_plan(tables, plane_kind, device):
    """smm_grad_plan_create on a rule's tables with the planes named; SmmError when the library refuses."""
    from smmregrid_amd import _lib
    kinds = (ctypes.c_int * len(plane_kind))(*plane_kind)
    h = ctypes.c_void_p()
    _lib.call("smm_grad_plan_create", tables["nx"], tables["ny"], int(tables["periodic"]), len(plane_kind), kinds,
              tables["si"].ctypes.data_as(ctypes.c_void_p), tables["sj"].ctypes.data_as(ctypes.c_void_p),
              tables["ci"].ctypes.data_as(ctypes.c_void_p), int(device), ctypes.byref(h))
    return h


# ------------------------------------------------------------------ the gather fuzz: what each seed draws

FUZZ_SEEDS = tuple(range(24))
FUZZ_GRIDS = ((12, 7), (40, 9), (257, 33))
FUZZ_D = (1, 63, 64, 65, 255, 256, 257, 600)
BATCH_CLASSES = ((1,), (2, 3), (4, 5, 6, 7, 8, 9))
INSTANTIATIONS = tuple((K, dt, bt) for K in (2, 3, 4) for dt in ("f32", "f64") for bt in (1, 2, 4))


def cols_batch_rows(n_j):
    """Batch rows per thread of one gather launch of n_j rows (smm_grad.hip)."""
    return 4 if n_j >= 4 else (2 if n_j >= 2 else 1)


def fuzz_draw(seed):
    """The parameters of fuzz case `seed`.  The first 18 seeds walk K x field type x batch class (B = 1, B in {2, 3},
    B >= 4) in turn, with a scratch that lets the first round have that many rows; the last 6 cut larger batches into
    rounds of 1, 2 and 3 rows; everything else is drawn."""
    rng = np.random.default_rng([SEED, 77, seed])
    p = {"seed": seed}
    if seed < 18:
        p["K"], p["dtype"] = (2, 3, 4)[seed % 3], ("f32", "f64")[(seed // 3) % 2]
        cls = BATCH_CLASSES[seed // 6]
        p["B"] = int(rng.choice(cls))
        p["scratch_rows"] = (None, 1, 2, 3)[int(rng.integers(4))] if len(cls) == 1 else \
            ((None, 2, 3)[int(rng.integers(3))] if len(cls) == 2 else None)
    else:
        p["K"], p["dtype"] = int(rng.integers(2, 5)), ("f32", "f64")[int(rng.integers(2))]
        p["B"] = (9, 5, 7, 4, 6, 8)[seed - 18]                      # several rounds, most with a shorter tail
        p["scratch_rows"] = (1, 2, 3)[seed % 3]
    p["grid"] = FUZZ_GRIDS[int(rng.integers(3))]
    p["D"] = FUZZ_D[(seed + int(rng.integers(2)) * 3) % len(FUZZ_D)]
    p["periodic"] = bool(rng.integers(2))
    p["plane"] = (GRAD_I, GRAD_J)[int(rng.integers(2))]             # K = 2: which plane the second column weighs
    p["num_wgts"] = {2: (3, 4)[int(rng.integers(2))], 3: 3, 4: 4}[p["K"]]
    p["links"] = ("random", "ragged")[int(rng.integers(2))]
    p["masked"] = bool(rng.integers(2))
    p["area_min"] = (0.0, 0.25, 0.5, 0.9)[int(rng.integers(4))]
    return p


def fuzz_instantiations(p):
    """The (K, field type, batch rows per thread) kernels case p launches: one per round of the scratch."""
    rows = p["B"] if p["scratch_rows"] is None else min(p["scratch_rows"], p["B"])
    sizes = {rows} | ({p["B"] % rows} - {0})
    return {(p["K"], p["dtype"], cols_batch_rows(n)) for n in sizes}
