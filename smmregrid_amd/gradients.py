"""The source-gradient rule of `gradients=True`, stated once in numpy.

Bicubic weights (`method="bic"`, `cdo genbic`: `num_wgts` = 4) and second-order conservative weights (`method="con2"`,
SCRIP-style: `num_wgts` = 3) carry, beside the value weight of column 0, weights of the source field's gradients.
`GradientRule` says which gradients those are and how they are taken on a regular lon/lat source; its `gradients` is the
definition the device kernel (smm_gradients) is tested against bit for bit, as `CFEncode.encode` and `GribEncode.encode`
are for their kernels.  Host only: numpy, no device.

Per batch row, with f widened to float64, i the column (longitude) and j the row (latitude) of a cell, i+ / i- the
east / west and j+ / j- the next / previous row in the order the field is stored:

* A neighbour is ABSENT when it lies outside the grid (j beyond the first or last row; i beyond the ends unless the
  longitudes close the circle -- `periodic`, by the test of `gridgen._is_cyclic`) or its value is not finite.
  `src_grid_imask` is not consulted.
* ``g_i[j,i] = ((f[j,i+] - f[j,i-]) * si[c][i]) * ci[j]``; an absent side is replaced by the cell itself, and c picks
  the table: 0 both sides present, 1 the + side only, 2 the - side only.  With both sides absent, or f[j,i] itself not
  finite, the gradient is exactly +0.0.
* ``g_j[j,i] = (f[j+,i] - f[j-,i]) * sj[c][j]`` by the same presence rule.
* ``g_ij`` is the i-difference rule applied to the plane g_j, presence still judged on f.
* The tables are made here in float64; the device multiplies and never divides.
  Index kind (`num_wgts` = 4): si = {0.5, 1, 1}, ci = 1, sj = +-{0.5, 1, 1} -- derivatives per grid index, which is what
  the cubic Hermite basis of `gridgen.bicubic_weights` multiplies; the sign makes the j derivative point towards
  increasing latitude (the generator works south to north and only renumbers the cells of a north-to-south grid).
  Planes in column order: g_i, g_j, g_ij.
  Sphere kind (`num_wgts` = 3): sj[c][j] = 1 / (lat[a] - lat[b]) in radians for the two rows actually used,
  si[c][i] = 1 / dlon in radians with the east-minus-west difference unwrapped into (0, 2 pi], ci[j] = 1 / cos(lat_j)
  and 0 where cos(lat_j) < 1e-9 (a pole row).  Planes in column order: g_j, g_i -- d/dlat and (1 / cos lat) d/dlon, the
  two gradients `gridgen.conservative2_weights` integrates against.
* A non-finite cell still enters a regrid through column 0 as ever (the 1e20 fill, then > 1e19 -> NaN); its gradients
  are finite, so the NaN footprint of a result is the footprint of the column-0 result.  This is SCRIP's
  masked-neighbour convention as recalled; it is not pinned against a CDO `remapbic` / `remapcon2` run.
"""
import ctypes
import math
import types

import numpy as np

GRAD_I, GRAD_J, GRAD_IJ = 0, 1, 2      # SMM_GRAD_*
_POLE_COS = 1e-9


def _unwrapped(d):
    """A longitude difference in radians brought into (0, 2 pi]."""
    d = np.mod(d, 2.0 * math.pi)
    return np.where(d <= 0.0, d + 2.0 * math.pi, d)


class GradientRule:
    """The gradients of one regular lon/lat source grid for weights of `num_wgts` columns.

    lon: the nx column longitudes, lat: the ny row latitudes (radians, in the order the field is stored: ascending,
    descending and Gaussian latitudes are fine).  `from_weights` reads them from a weights Dataset."""

    def __init__(self, lon, lat, num_wgts, periodic=None):
        self.lon = np.ascontiguousarray(lon, dtype=np.float64).ravel()
        self.lat = np.ascontiguousarray(lat, dtype=np.float64).ravel()
        self.nx, self.ny = int(self.lon.size), int(self.lat.size)
        if self.nx < 1 or self.ny < 1:
            raise ValueError("gradients need a source grid of at least one cell")
        self.num_wgts = int(num_wgts)
        if self.num_wgts == 4:
            self.kind, self.plane_kind = "index", (GRAD_I, GRAD_J, GRAD_IJ)
        elif self.num_wgts == 3:
            self.kind, self.plane_kind = "sphere", (GRAD_J, GRAD_I)
        else:
            raise ValueError(f"gradients=True needs weights of 3 (second-order conservative) or 4 (bicubic) columns, "
                             f"these have num_wgts = {self.num_wgts}")
        if not (np.isfinite(self.lon).all() and np.isfinite(self.lat).all()):
            raise ValueError("gradients need finite source cell centres")
        step = np.diff(self.lat)
        if self.ny > 1 and not ((step > 0).all() or (step < 0).all()):
            raise ValueError("gradients need a regular lon/lat source: its latitudes are not strictly monotonic")
        if periodic is None:
            from .gridgen import _is_cyclic
            periodic = _is_cyclic(types.SimpleNamespace(lon=np.degrees(self.lon)))
        self.periodic = bool(periodic)
        self.n_planes = len(self.plane_kind)
        self.size = self.nx * self.ny
        self._tables = None
        self._plans = {}

    @classmethod
    def from_weights(cls, weights):
        """The rule of a weights Dataset: `src_grid_dims`, `src_grid_center_lat`, `src_grid_center_lon` and the
        width of `remap_matrix`.  The source must be a regular lon/lat grid -- rank 2, nx fastest, latitude constant
        along a row and longitude along a column; anything else is a ValueError naming the reason."""
        from .xrlite import from_xarray
        weights = from_xarray(weights)
        rm = weights["remap_matrix"]
        if "num_wgts" in rm.dims:
            num_wgts = int(rm.shape[rm.dims.index("num_wgts")])
        else:
            num_wgts = int(rm.shape[-1]) if len(rm.shape) >= 2 else 1
        if num_wgts not in (3, 4):
            raise ValueError(f"gradients=True needs weights of 3 (second-order conservative) or 4 (bicubic) columns, "
                             f"these have num_wgts = {num_wgts}")
        dims = np.asarray(weights["src_grid_dims"].values).astype(np.int64).ravel()
        if dims.size != 2:
            raise ValueError(f"gradients need a regular lon/lat source: src_grid_dims has rank {dims.size}, not 2 "
                             "(curvilinear and unstructured sources are out of scope)")
        nx, ny = int(dims[0]), int(dims[1])

        def centres(name):
            var = weights[name]
            v = np.asarray(var.values, dtype=np.float64)
            if v.size != nx * ny:      # weights with a mask dimension: every level has the same centres
                v = v.reshape(-1, nx * ny)[0]
            if str(var.attrs.get("units", "radians")).lower().startswith("deg"):
                v = np.radians(v)
            return v.reshape(ny, nx)

        lat, lon = centres("src_grid_center_lat"), centres("src_grid_center_lon")
        if not (lat == lat[:, :1]).all():
            raise ValueError("gradients need a regular lon/lat source: the latitude varies along a row of the grid")
        if not (lon == lon[:1, :]).all():
            raise ValueError("gradients need a regular lon/lat source: the longitude varies along a column of the grid")
        return cls(lon[0], lat[:, 0], num_wgts)

    # ------------------------------------------------------------------ tables
    def tables(self):
        """{"si": (3, nx), "sj": (3, ny), "ci": (ny,)} float64 and "plane_kind", "periodic", "nx", "ny": what
        smm_grad_plan_create takes.  Row c of si / sj: 0 both neighbours present, 1 the + one only, 2 the - one only;
        entries no cell can use (the + side of the last row, ...) are 0."""
        if self._tables is not None:
            return self._tables
        nx, ny = self.nx, self.ny
        si, sj, ci = np.zeros((3, nx)), np.zeros((3, ny)), np.ones(ny)
        if self.kind == "index":
            sign = -1.0 if (ny > 1 and self.lat[1] < self.lat[0]) else 1.0
            si[0], si[1], si[2] = 0.5, 1.0, 1.0
            sj[0], sj[1], sj[2] = sign * 0.5, sign, sign
        else:
            lat, lon = self.lat, self.lon
            if ny > 2:
                sj[0, 1:-1] = 1.0 / (lat[2:] - lat[:-2])
            if ny > 1:
                sj[1, :-1] = 1.0 / (lat[1:] - lat[:-1])
                sj[2, 1:] = 1.0 / (lat[1:] - lat[:-1])
            if self.periodic:
                east, west = np.roll(lon, -1), np.roll(lon, 1)
                si[0] = 1.0 / _unwrapped(east - west)
                si[1] = 1.0 / _unwrapped(east - lon)
                si[2] = 1.0 / _unwrapped(lon - west)
            else:
                if nx > 2:
                    si[0, 1:-1] = 1.0 / _unwrapped(lon[2:] - lon[:-2])
                if nx > 1:
                    si[1, :-1] = 1.0 / _unwrapped(lon[1:] - lon[:-1])
                    si[2, 1:] = 1.0 / _unwrapped(lon[1:] - lon[:-1])
            cos = np.cos(lat)
            pole = cos < _POLE_COS
            ci = np.where(pole, 0.0, 1.0 / np.where(pole, 1.0, cos))
        self._tables = {"si": np.ascontiguousarray(si), "sj": np.ascontiguousarray(sj), "ci": np.ascontiguousarray(ci),
                        "plane_kind": self.plane_kind, "periodic": self.periodic, "nx": nx, "ny": ny}
        return self._tables

    # ------------------------------------------------------------------ the rule
    def _neighbours(self, a, axis):
        """(a at the + neighbour, a at the - neighbour) along axis 0 (j) or 1 (i); NaN outside the grid."""
        if axis == 1 and self.periodic:
            return np.roll(a, -1, axis=1), np.roll(a, 1, axis=1)
        plus, minus = np.full_like(a, np.nan), np.full_like(a, np.nan)
        if axis == 1:
            plus[:, :-1], minus[:, 1:] = a[:, 1:], a[:, :-1]
        else:
            plus[:-1], minus[1:] = a[1:], a[:-1]
        return plus, minus

    def _difference(self, f, v, axis, scale, row_factor=None):
        """The difference rule along one axis: presence judged on f, the values differenced are v."""
        fp, fm = self._neighbours(f, axis)
        vp, vm = (fp, fm) if v is f else self._neighbours(v, axis)
        pp, pm = np.isfinite(fp), np.isfinite(fm)
        ok = np.isfinite(f) & (pp | pm)
        hi, lo = np.where(pp, vp, v), np.where(pm, vm, v)
        code = np.where(pp & pm, 0, np.where(pp, 1, 2))
        n = f.shape[axis]
        idx = np.arange(n)[None, :] if axis == 1 else np.arange(n)[:, None]
        with np.errstate(invalid="ignore", over="ignore"):
            d = (hi - lo) * scale[code, idx]
            if row_factor is not None:
                d = d * row_factor[:, None]
        return np.where(ok, d, 0.0)

    def gradients(self, field2d):
        """The planes of one field of shape (ny, nx) (or flat, nx fastest), in column order: (n_planes, ny, nx)
        float64."""
        f = np.asarray(field2d)
        if f.size != self.size:
            raise ValueError(f"the field has {f.size} cells, the source grid {self.nx} x {self.ny}")
        f = f.reshape(self.ny, self.nx).astype(np.float64)
        t = self.tables()
        g_j = self._difference(f, f, 0, t["sj"])
        planes = []
        for kind in self.plane_kind:
            if kind == GRAD_I:
                planes.append(self._difference(f, f, 1, t["si"], t["ci"]))
            elif kind == GRAD_J:
                planes.append(g_j)
            else:
                planes.append(self._difference(f, g_j, 1, t["si"], t["ci"]))
        return np.stack(planes, axis=0)

    def gradients_rows(self, x):
        """`gradients` of every row of a (B, S) batch: (B, n_planes, S) float64."""
        x = np.asarray(x)
        out = np.empty((x.shape[0], self.n_planes, self.size), dtype=np.float64)
        for b in range(x.shape[0]):
            out[b] = self.gradients(x[b, :self.size]).reshape(self.n_planes, self.size)
        return out

    def stacked(self, x):
        """The "stacked" float64 field the K-column apply is defined by: (B, S * K) with entry s * K + 0 the value
        f[s] filled with its own dtype's 1e20 and widened, entry s * K + k plane k of the row."""
        x = np.asarray(x)
        x = x[:, :self.size]
        filled = np.where(np.isfinite(x), x, x.dtype.type(1e20)).astype(np.float64)
        g = self.gradients_rows(x)
        return np.ascontiguousarray(np.concatenate([filled[:, None, :], g], axis=1).transpose(0, 2, 1)).reshape(
            x.shape[0], -1)

    # ------------------------------------------------------------------ the device side of the tables
    def plan(self, device):
        """The smm_grad_plan_t of these tables on `device` (made once, kept with the rule)."""
        device = int(device)
        p = self._plans.get(device)
        if p is None:
            p = self._plans[device] = _DevicePlan(self, device)
        return p.handle

    def __repr__(self):
        return (f"GradientRule({self.kind}, nx={self.nx}, ny={self.ny}, periodic={self.periodic}, "
                f"planes={self.n_planes})")


class _DevicePlan:
    def __init__(self, rule, device):
        from . import _lib
        t = rule.tables()
        kinds = (ctypes.c_int * rule.n_planes)(*rule.plane_kind)
        h = ctypes.c_void_p()
        _lib.call("smm_grad_plan_create", rule.nx, rule.ny, int(rule.periodic), rule.n_planes, kinds,
                  t["si"].ctypes.data_as(ctypes.c_void_p), t["sj"].ctypes.data_as(ctypes.c_void_p),
                  t["ci"].ctypes.data_as(ctypes.c_void_p), device, ctypes.byref(h))
        self.handle = h

    def __del__(self):
        try:
            from . import _lib
            if self.handle:
                _lib.call("smm_grad_plan_destroy", self.handle)
                self.handle = None
        except Exception:
            pass
