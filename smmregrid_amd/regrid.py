"""Regridder facade -- drop-in for smmregrid.regrid.Regridder on the apply path.

Same constructor keywords, methods and exceptions as the reference
(regrid.py:55-59, :233, :273, :339, :429, :458, :656); the arithmetic that the
reference hands to dask/sparse (regrid.py:545-570) runs in the HIP library.
Inputs may be xarray objects (when xarray is importable) or the lite
containers of `smmregrid_amd.xrlite`; the result has the type of the input.
A field whose ``data`` is a `DeviceArray` stays in HBM (no host copies).

By default the result is eager (numpy- or HBM-backed).  ``Regridder(..., lazy=True)`` gives the
reference's contract (regrid.py:29-30): nothing is launched before ``.values`` / ``.compute()``;
a dask-backed field comes back dask-backed with the chunking of its kept dimensions preserved
(`lazy.map_batch_blocks`), any other field as a `lazy.LazyArray`.
"""
import logging
import math
import os

import numpy as np

from . import road
from .device import CFDecode, CFEncode, DeviceArray, is_packed_dtype, to_device
from .griblite import GribEncode, GribField
from .gridtype import GridType, tolist
from .lazy import LazyArray, is_dask, map_batch_blocks
from .operator import OperatorGroup, _host_field
from .weights import (_level_slice, check_mask, compute_weights_matrix, compute_weights_matrix3d,
                      mask_weights)
from .xrlite import DataArray, Dataset, from_xarray, is_xarray, to_xarray

DEFAULT_AREA_MIN = 0.5  # default minimum area for conservative remapping (regrid.py:49)


def _logger(level):
    log = logging.getLogger("smmregrid.Regrid")
    log.setLevel(getattr(logging, str(level).upper(), logging.WARNING))
    return log


def _remove_degenerate_axes(a):
    """dimension.py:22-37 of the reference: collapse axes along which a 2-D
    coordinate array does not vary."""
    a = np.asarray(a)
    if a.ndim != 2:
        return a
    if (a == a[0:1, :]).all():
        return a[0, :]
    if (a == a[:, 0:1]).all():
        return a[:, 0]
    return a


class Regridder(object):
    """Main regridding class (reference: regrid.py:52)."""

    def __init__(self, source_grid=None, target_grid=None, weights=None,
                 method='con', remap_area_min=DEFAULT_AREA_MIN, transpose=True, mask_dim=None,
                 vertical_dim=None, horizontal_dims=None, cdo_extra=None, cdo_options=None,
                 check_nan=False, cdo='cdo', loglevel='WARNING', device=None, out_dtype=None,
                 lazy=False, prune_zero_weights=False, keep_batch_fastest=False, skipna=False, packed=False,
                 packed_levels=False, packed_out=False, packed_out_levels=False, half=False, packed_skipna=False, grib_out=False,
                 grib_out_levels=False, grib_out_ccsds=False, grib_out_cpx=False, gradients=False, categorical=False):
        if (source_grid is None or target_grid is None) and (weights is None):
            raise ValueError("Either weights or source_grid/target_grid must be supplied")

        if vertical_dim is not None:  # deprecated_argument (util.py:23-40)
            import warnings
            warnings.warn("'vertical_dim' is deprecated, use 'mask_dim'", DeprecationWarning)
            if mask_dim is None:
                mask_dim = vertical_dim

        self.loggy = _logger(loglevel)
        self.loglevel = loglevel
        self.device = device
        # opt-in: links of weight exactly 0 (3 of 4 bilinear links between aligned grids) are dropped when
        # the operators are built; results are bit-identical (SMM_CREATE_PRUNE_ZEROS)
        self.prune_zero_weights = bool(prune_zero_weights)
        # categorical: True -- every variable is a class variable; a name or a collection of names -- those are
        if isinstance(categorical, (bool, type(None))):
            self.categorical_names = None
        else:
            self.categorical_names = frozenset([categorical] if isinstance(categorical, str) else categorical)
        # the switches (`road.Switches` says what each one does) live as attributes, read again at every call
        switches = road.Switches.of(
            out_dtype=out_dtype, transpose=transpose, lazy=lazy, skipna=skipna, keep_batch_fastest=keep_batch_fastest,
            packed=packed, packed_levels=packed_levels, packed_skipna=packed_skipna, packed_out=packed_out,
            packed_out_levels=packed_out_levels, half=half, grib_out=grib_out, grib_out_levels=grib_out_levels,
            grib_out_ccsds=grib_out_ccsds, grib_out_cpx=grib_out_cpx, gradients=gradients,
            categorical=bool(categorical) if self.categorical_names is None else bool(self.categorical_names))
        for name, value in switches._asdict().items():
            setattr(self, name, value)
        refused = road.refusal(switches)
        if refused is not None:
            raise ValueError(refused)
        mask_dim = tolist(mask_dim)
        horizontal_dims = tolist(horizontal_dims)
        self.extra_dims = {'mask': mask_dim, 'horizontal': horizontal_dims}

        self.remap_area_min = float(remap_area_min)
        if self.remap_area_min < 0.0 or self.remap_area_min > 1.0:
            raise ValueError('The remap_area_min provided must be between 0.0 and 1.0')

        if weights is not None:
            self.init_mode = 'weights'
            self.grids = self._gridtype_from_weights(weights)
        else:
            self.init_mode = 'grids'
            from .cdogenerate import CdoGenerate
            if isinstance(source_grid, str) and not os.path.isfile(source_grid):
                raise FileNotFoundError(f'Cannot find grid file {source_grid}')      # regrid.py:133-138
            if isinstance(source_grid, str) and os.path.isfile(source_grid):
                from .io import open_dataset       # regrid.py:133-136: a data file as source grid
                source_grid = open_dataset(source_grid)
            source_grid_array = from_xarray(source_grid)
            self.grids = self._gridtype_from_data(source_grid_array)
            if len(self.grids) == 0:
                raise ValueError('Cannot find any gridtype in your data, aborting!')
            for index, gridtype in enumerate(self.grids):
                if check_nan:
                    # NaN pattern varying along a non-time dimension -> that dimension is masked
                    gridtype = self._check_nan_variation(source_grid_array, gridtype)
                    self.grids[index] = gridtype
                # weights are generated from one variable of this gridtype (regrid.py:171-177)
                sample = next(iter(gridtype.variables.values()), source_grid_array)
                if isinstance(source_grid_array, Dataset) and isinstance(sample, DataArray):
                    # ... together with the grid's bounds variables, as the reference stores them (regrid.py:173-175;
                    # a file name goes to cdo whole, :168-169): the native generator takes a lon/lat grid's cell edges
                    # and a mesh's cell polygons from them, as CDO does.  Bounds are the variables the reference's name
                    # rule finds plus those the horizontal coordinates name in their CF `bounds` attribute
                    # (`bounds_nav_lon` of a CMOR ocean file does not end in `_bounds`)
                    named = [c.attrs.get("bounds") for k, c in sample.coords.items() if "time" not in str(k)]
                    wanted = [b for b in dict.fromkeys(list(gridtype.bounds) + named)
                              if b and b in source_grid_array and "time" not in b]
                    if wanted:
                        picked = Dataset({sample.name: sample}, attrs=source_grid_array.attrs)
                        for bname in wanted:
                            picked[bname] = source_grid_array[bname]
                        sample = picked
                generator = CdoGenerate(sample, target_grid, cdo=cdo,
                                        cdo_options=cdo_options, cdo_extra=cdo_extra,
                                        loglevel=loglevel)
                gridtype.weights = generator.weights(method=method, mask_dim=gridtype.mask_dim)

        if self.categorical:      # refused before any device work
            for gridtype in self.grids:
                if gridtype.mask_dim:
                    raise ValueError("categorical does not go with masked-level (3-D) weights: it goes with 2-D weights")
        if self.gradients:      # refused before any device work: masked levels, a source that is no regular lon/lat grid
            from .gradients import GradientRule
            for gridtype in self.grids:
                if gridtype.mask_dim:
                    raise ValueError("gradients=True does not go with masked-level (3-D) weights: it goes with 2-D weights")
                gridtype.grad_rule = GradientRule.from_weights(gridtype.weights)
        for gridtype in self.grids:
            self._setup_operators(gridtype)

    # ------------------------------------------------------------------ init helpers
    def _setup_operators(self, gridtype):
        """regrid.py:189-203: operators, destination mask, `masked` flags; then the
        epilogue vectors are placed next to the operators in HBM."""
        w = gridtype.weights
        if gridtype.mask_dim:
            gridtype.weights_matrix = compute_weights_matrix3d(w, gridtype.mask_dim, device=self.device,
                                                               prune_zeros=self.prune_zero_weights)
        else:
            gridtype.weights_matrix = compute_weights_matrix(w, device=self.device,
                                                             prune_zeros=self.prune_zero_weights, columns=self.gradients)

        if "dst_grid_masked" in w.variables:
            gridtype.masked = np.asarray(w["dst_grid_masked"].values)
            if gridtype.masked.ndim == 0:
                gridtype.masked = bool(gridtype.masked)
        else:
            gridtype.weights = mask_weights(w, gridtype.weights_matrix, gridtype.mask_dim)
            gridtype.masked = check_mask(gridtype.weights, gridtype.mask_dim)
        w = gridtype.weights

        if gridtype.mask_dim:
            for i, op in enumerate(gridtype.weights_matrix):
                op.set_epilogue(_level_slice(w["dst_grid_imask"], gridtype.mask_dim, i),
                                _level_slice(w["dst_grid_frac"], gridtype.mask_dim, i)
                                if "dst_grid_frac" in w else None)
            gridtype.group = OperatorGroup(gridtype.weights_matrix)
        else:
            gridtype.weights_matrix.set_epilogue(
                w["dst_grid_imask"].values,
                w["dst_grid_frac"].values if "dst_grid_frac" in w else None)

    def _gridtype_from_weights(self, weights):
        """regrid.py:205-223 + gridinspector.py:79-92."""
        if isinstance(weights, str):
            from .io import open_weights
            weights = open_weights(weights)
        weights = from_xarray(weights)
        if not isinstance(weights, Dataset):
            raise TypeError('weights must be a Dataset or a path to a weights file')
        gridtype = GridType(dims=[], weights=weights)
        if weights.coords:
            gridtype.mask_dim = list(weights.coords)[0]
        self.extra_dims['mask'] = [gridtype.mask_dim]
        return [gridtype]

    def _check_nan_variation(self, source_grid, gridtype):
        """regrid.py:630-653 + util.py:56-85: if the NaN mask of the first variable (first time
        step) changes along one of the unclassified dimensions, treat it as the masked dimension."""
        if gridtype.mask_dim:
            return gridtype
        arrays = list(source_grid.data_vars.values()) if isinstance(source_grid, Dataset) else [source_grid]
        arr = next((a for a in arrays if isinstance(a, DataArray)
                    and GridType(a.dims, extra_dims=self.extra_dims) == gridtype), None)
        if arr is None or not gridtype.other_dims:
            return gridtype
        if gridtype.time_dims and gridtype.time_dims[0] in arr.dims:
            arr = arr.isel(**{gridtype.time_dims[0]: 0})
        vals = arr.values
        if not np.issubdtype(vals.dtype, np.floating):
            return gridtype
        nan_mask = np.isnan(vals)
        nan_dims = [d for d in gridtype.other_dims if d in arr.dims
                    and np.diff(nan_mask.astype(np.int8), axis=arr.dims.index(d)).astype(bool).any()]
        if not nan_dims:
            return gridtype
        self.loggy.warning('Found NaN variation in dimensions: %s', nan_dims)
        self.extra_dims['mask'] = nan_dims
        new = GridType(dims=gridtype.dims + gridtype.other_dims + (gridtype.time_dims or []),
                       extra_dims=self.extra_dims)
        new.variables = gridtype.variables
        return new

    def _gridtype_from_data(self, data):
        grids = []
        arrays = data.data_vars.values() if isinstance(data, Dataset) else [data]
        for arr in arrays:
            if not isinstance(arr, DataArray):
                continue
            name = arr.name or ''
            if any(s in name for s in ("bnds", "bounds", "vertices")):
                continue
            gt = GridType(dims=arr.dims, extra_dims=self.extra_dims)
            if not gt.horizontal_dims:
                continue
            known = next((g for g in grids if g == gt), None)
            if known is None:
                grids.append(gt)
                known = gt
            known.variables[name] = arr          # gridinspector.py: variables living on this grid
        if isinstance(data, Dataset):            # gridinspector.py:183-221: spatial bounds variables go with the grid
            for name, arr in data.data_vars.items():
                spatial = (name.endswith("_bnds") or name.endswith("_bounds") or name == "vertices") and "time" not in name
                for gt in grids:
                    if spatial and set(gt.dims) & set(arr.dims) and name not in gt.bounds:
                        gt.bounds.append(name)
        return grids

    # ------------------------------------------------------------------ public API
    def regrid(self, source_data):
        """regrid.py:233-271."""
        was_xarray = is_xarray(source_data)
        data = from_xarray(source_data)
        if isinstance(data, Dataset):
            datagrids = self._gridtype_from_data(data)
            if len(datagrids) > 1 and self.init_mode == 'weights':
                raise ValueError(
                    f'Cannot process data with {len(datagrids)} GridType initializing from weights')
            out = data.map(self.regrid_array, keep_attrs=True)
            degen = [k for k, v in out.data_vars.items() if v.dims == ()]
            out = out.drop_vars(degen)
            return to_xarray(out) if was_xarray else out
        if isinstance(data, DataArray):
            out = self.regrid_array(data)
            return to_xarray(out) if was_xarray else out
        raise TypeError('The object provided is not a Xarray object!')

    def regrid_array(self, source_data):
        """regrid.py:273-312."""
        source_data = from_xarray(source_data)
        scalars = [name for name, coord in source_data.coords.items() if coord.dims == ()]
        if scalars:                                   # regrid.py:288-294
            self.loggy.warning("Found scalar coordinates %s. If have selected a along a masked dimensions,"
                               "regridding might fail. Please consider subsetting with [] or with slice", scalars)
        datagridtype = GridType(dims=source_data.dims, extra_dims=self.extra_dims)
        name = source_data.name or ''
        is_bounds = (name.endswith('_bnds') or name.endswith('_bounds') or name == 'vertices') and 'time' not in name
        if not (datagridtype.horizontal_dims or datagridtype.mask_dim) or is_bounds:
            # GridInspector finds no grid in such a variable (spatial bounds are skipped, gridinspector.py:70-78; a grid
            # without horizontal or mask dimension is cleaned away, :133-143 -- time_bnds(time, bnds) is one): nothing
            # to regrid, and the empty result is dropped from a Dataset (regrid.py:308-312, :262-264)
            return DataArray(data=None)
        if self.categorical and (self.categorical_names is None or name in self.categorical_names):
            return self._regrid_categorical(source_data, datagridtype)
        # the facts: the rules its attributes give (one WARNING each when they give none), its grid's gradient rule
        cf = self._packed_rule(source_data) if self.packed else None
        enc = self._packed_out_rule(source_data) if (self.packed_out and cf is not None) else None
        packing = {k: source_data.attrs[k] for k in road.CF_PACKING_ATTRS if k in source_data.attrs}
        grad_rule = getattr(self._get_gridtype(datagridtype), "grad_rule", None)
        way = road.decide(self.switches, self._facts(source_data, datagridtype.horizontal_dims, datagridtype.mask_dim,
                                                     cf=cf, cf_out=enc, grad_rule=grad_rule))
        self._emit(way.lines)
        if way.refusal is not None and way.refusal[0] == road.VARIABLE:
            raise ValueError(way.refusal[1])
        if way.source == road.DECODED:      # what np.asarray would do anyway; regridded as before
            source_data = self._decode_on_host(source_data, cf)
        if way.source != road.RAW_CF:
            cf = None
        cf_out = enc if way.result == road.CF_KERNEL else None
        if datagridtype.mask_dim:
            out = self.regrid3d(source_data, datagridtype, cf=cf, cf_out=cf_out, way=way)
            if out.data is not None:
                self._emit(way.after)
                if way.result == road.CF_HOST:
                    self._encode_on_host(out, enc)
        else:
            out = self.regrid2d(source_data, datagridtype, cf=cf, cf_out=cf_out, way=way)
        # an empty result (no grid of this Regridder, a bounds variable) keeps the attributes it was given before
        encoded = way.result in (road.CF_KERNEL, road.CF_HOST) if out.data is not None else \
            enc is not None and not (datagridtype.mask_dim and self.packed_out_levels)
        if encoded:
            out.attrs.update(packing)      # the result is raw again: it keeps the rule it was encoded with
        elif cf is not None:
            for k in road.CF_PACKING_ATTRS:
                out.attrs.pop(k, None)
        return out

    def _regrid_categorical(self, source_data, datagridtype):
        """A class variable (categorical): regridded by largest area fraction through `apply_mode` / `apply_mode_host`,
        in its own dtype and with its own attributes.  An integer variable's missing values are its `_FillValue` /
        `missing_value`, and dead target cells get the first of them; without either, one WARNING and the dtype's
        minimum (signed) or maximum (unsigned).  A float variable's missing value is whatever is not finite."""
        from .categorical import ModeRule
        way = road.decide(self.switches, self._facts(source_data, datagridtype.horizontal_dims, datagridtype.mask_dim,
                                                     categorical=True))
        self._emit(way.lines)
        if way.refusal is not None:
            raise ValueError(way.refusal[1])
        gridtype = self._get_gridtype(datagridtype)
        if gridtype is None:
            return DataArray(data=None)
        horizontal_dims, weights, op = gridtype.horizontal_dims, gridtype.weights, gridtype.weights_matrix
        if not any(x in source_data.dims for x in (horizontal_dims or [])):
            self.loggy.error("None of dimensions on which we can interpolate is found in the DataArray.")
            raise KeyError('Dimensions mismatch')
        kept_dims = [d for d in source_data.dims if d not in horizontal_dims]
        kept_shape = [source_data.sizes[d] for d in kept_dims]
        tgt_shape, tgt_dims = self._target_layout(weights)
        n_batch = int(np.prod(kept_shape)) if kept_shape else 1
        masked = bool(np.asarray(gridtype.masked).any()) if np.ndim(gridtype.masked) else bool(gridtype.masked)
        src = source_data.data
        rule, found = ModeRule.from_attrs(source_data.attrs, src.dtype)
        if not found:
            self.loggy.warning("categorical variable %s names no _FillValue / missing_value: %d stands for a target cell "
                               "without a class", source_data.name, rule.fill_out)
        kw = dict(masked=masked, remap_area_min=self.remap_area_min, fill=rule.fill, fill_out=rule.fill_out)
        if isinstance(src, DeviceArray):
            x = src.reshape(n_batch, -1)
            _check_cells(x.shape[1], op.n_src)
            out_data = op.apply_mode(x, **kw).reshape(*(kept_shape + tgt_shape))
        else:
            host = np.ascontiguousarray(_computed(src)).reshape(n_batch, -1)
            _check_cells(host.shape[1], op.n_src)
            out_data = op.apply_mode_host(host, **kw).reshape(kept_shape + tgt_shape)
        return self._finish(out_data, kept_dims + tgt_dims, source_data, kept_dims, weights, tgt_shape, tgt_dims)

    @property
    def switches(self):
        return road.Switches(*[getattr(self, name) for name in road.Switches._fields])

    def _emit(self, lines):
        for level, text in lines:
            getattr(self.loggy, level)(text)

    @staticmethod
    def _facts(source_data, horizontal_dims, mask_dim, cf=None, cf_out=None, grad_rule=None, **direct):
        """`road.Facts` of a variable: how it is held, its dtype and dims, the rules that stand ready for it."""
        data = source_data.data
        held = road.GRIB if isinstance(data, GribField) else data.layout if isinstance(data, DeviceArray) else \
            road.LAZY if isinstance(data, LazyArray) else road.DASK if is_dask(data) else road.HOST
        codec = None if held != road.GRIB or data.coded is None else data.coded.codec.name
        return road.Facts(source_data.name, held, getattr(data, "dtype", None), source_data.dims, horizontal_dims or (), mask_dim,
                          cf is not None, cf_out is not None, codec, grad_rule is not None, **direct)

    def _packed_out_rule(self, source_data):
        """The CFEncode of a packed variable's own attributes, or None (one WARNING) when they name no fill value."""
        try:
            return CFEncode.from_attrs(source_data.attrs, source_data.data.dtype)
        except ValueError as err:
            self.loggy.warning("packed variable %s comes back as float64, not packed: %s", source_data.name, err)
            return None

    @staticmethod
    def _encode_on_host(out, enc):
        """packed_out on masked-level (3-D) weights without packed_out_levels: a host result is encoded here with the
        same rule (the same bits as the level-group _pk entries give)."""
        data = out.data
        if isinstance(data, LazyArray):
            out.data = LazyArray(data.shape, enc.raw_dtype, lambda: enc.encode(data.compute()))
        else:
            out.data = enc.encode(np.asarray(data))

    def _packed_rule(self, source_data):
        """The CFDecode of a 2-byte integer variable that carries CF packing attributes, else None."""
        dtype = getattr(source_data.data, "dtype", None)
        if dtype is None or not is_packed_dtype(dtype) or not any(k in source_data.attrs for k in road.CF_PACKING_ATTRS):
            return None
        try:
            return CFDecode.from_attrs(source_data.attrs, raw_dtype=dtype)
        except ValueError as err:      # more than two distinct fill values: the field is regridded as it was before
            self.loggy.warning("packed variable %s is not regridded raw: %s", source_data.name, err)
            return None

    @staticmethod
    def _decode_on_host(source_data, cf):
        """The variable with its `GribField` decoded, or its raw integers decoded by `cf` (its packing attributes go)."""
        src, attrs = source_data.data, source_data.attrs
        if isinstance(src, GribField):
            data = src.decode()
        elif isinstance(src, DeviceArray):
            data = to_device(cf.decode(src.to_host()), layout=src.layout)
        else:
            data = cf.decode(_computed(src))
        if not isinstance(src, GribField):
            attrs = {k: v for k, v in attrs.items() if k not in road.CF_PACKING_ATTRS}
        return DataArray(data, dims=source_data.dims, coords=source_data.coords, attrs=attrs, name=source_data.name)

    def _get_gridtype(self, datagridtype):
        """regrid.py:324-337."""
        if self.init_mode == 'weights':
            self.grids[0].dims = datagridtype.dims
            self.grids[0].horizontal_dims = datagridtype.horizontal_dims
            self.grids[0].other_dims = datagridtype.other_dims
        return next((grid for grid in self.grids if grid == datagridtype), None)

    def regrid2d(self, source_data, datagridtype, cf=None, cf_out=None, out_dtype=None, way=None):
        """regrid.py:429-456.  way: the `road.Road` `regrid_array` decided (None: `apply_weights` decides)."""
        gridtype = self._get_gridtype(datagridtype)
        if gridtype is None:
            return DataArray(data=None)
        return self.apply_weights(source_data, gridtype.weights,
                                  weights_matrix=gridtype.weights_matrix,
                                  masked=gridtype.masked,
                                  horizontal_dims=gridtype.horizontal_dims, cf=cf, cf_out=cf_out, out_dtype=out_dtype,
                                  gradients=getattr(gridtype, "grad_rule", None), way=way)

    # ------------------------------------------------------------------ apply (2-D)
    def _target_layout(self, weights):
        """regrid.py:572-579: target shape/dims from dst_grid_dims."""
        dst_grid_shape = np.asarray(weights["dst_grid_dims"].values).astype(np.int64)
        rank = dst_grid_shape.size
        if rank == 2:
            return [int(dst_grid_shape[1]), int(dst_grid_shape[0])], ["i", "j"]
        if rank == 1:
            return [int(dst_grid_shape[0])], ['cell']
        raise ValueError('Unknown dimensional target grid')

    def _finish(self, data, dims, source_data, kept_dims, weights, tgt_shape, tgt_dims):
        """regrid.py:586-626: coordinates, lat/lon in degrees, attrs."""
        coords = {k: v for k, v in source_data.coords.items() if set(v.dims).issubset(kept_dims)}
        axis_scale = 180.0 / math.pi
        lat = _remove_degenerate_axes(
            np.asarray(weights["dst_grid_center_lat"].values).reshape(tgt_shape))
        lon = _remove_degenerate_axes(
            np.asarray(weights["dst_grid_center_lon"].values).reshape(tgt_shape))
        lat = np.round(lat * axis_scale, 10)
        lon = np.round(lon * axis_scale, 10)
        dims = list(dims)
        if tgt_dims == ["i", "j"] and lat.ndim == 1 and lon.ndim == 1:
            dims = [{"i": "lat", "j": "lon"}.get(d, d) for d in dims]
            lat_dims, lon_dims = ("lat",), ("lon",)
        else:
            lat_dims = lon_dims = tuple(tgt_dims) if lat.ndim == len(tgt_dims) else (tgt_dims[0],)
        out = DataArray(data, dims=dims, coords=coords, attrs=dict(source_data.attrs),
                        name=source_data.name)
        out.coords["lat"] = DataArray(lat, dims=lat_dims, name="lat", attrs={
            "units": "degrees_north", "standard_name": "latitude", "axis": "Y"})
        out.coords["lon"] = DataArray(lon, dims=lon_dims, name="lon", attrs={
            "units": "degrees_east", "standard_name": "longitude", "axis": "X"})
        out.attrs.pop('CDI_grid_type', None)
        return out

    def _road(self, way, source_data, horizontal_dims, mask_dim, cf, cf_out, grad_rule, **asked):
        """(the road, the field) of an apply: `way` as `regrid_array` decided it, or for a direct call -- which brings
        its own cf, cf_out, out_dtype and grib_out -- the same `road.decide`, the field decoded if it asks for that."""
        src = source_data.data
        if way is None:
            way = road.decide(self.switches, self._facts(source_data, horizontal_dims, mask_dim, cf=cf, cf_out=cf_out,
                                                         grad_rule=grad_rule, direct=True, **asked))
            if way.source == road.DECODED:      # only the raw road ships the bit streams
                src = src.decode()
        if way.refusal is not None:
            raise ValueError(way.refusal[1])
        return way, src

    def apply_weights(self, source_data, weights, weights_matrix=None, masked=True,
                      horizontal_dims=None, cf=None, cf_out=None, out_dtype=None, gradients=None, way=None):
        """regrid.py:458-628 for one 2-D operator.  cf: the CFDecode of a raw int16 / uint16 field (packed=True);
        cf_out: the CFEncode its result is stored with (packed_out=True); out_dtype: this variable's result dtype
        (None: the Regridder's, or the field's own half type under half=True); gradients: the `GradientRule` of these
        weights (Regridder(gradients=True); None there: made from `weights`); way: the `road.Road` of this variable as
        `regrid_array` decided it (None, a direct call: decided here)."""
        source_data = from_xarray(source_data)
        weights = from_xarray(weights)
        name = source_data.name or ''
        if any(s in name for s in ("bnds", "bounds", "vertices")):
            if 'time' in name:
                return source_data
            return DataArray(data=None)

        if not any(x in source_data.dims for x in (horizontal_dims or [])):
            self.loggy.error("None of dimensions on which we can interpolate is found in the DataArray.")
            raise KeyError('Dimensions mismatch')

        kept_dims = [d for d in source_data.dims if d not in horizontal_dims]
        kept_shape = [source_data.sizes[d] for d in kept_dims]
        tgt_shape, tgt_dims = self._target_layout(weights)

        rule = gradients
        if rule is None and self.gradients:
            from .gradients import GradientRule
            rule = GradientRule.from_weights(weights)
        if weights_matrix is None:
            weights_matrix = compute_weights_matrix(weights, device=self.device, columns=rule is not None)
            weights_matrix.set_epilogue(
                weights["dst_grid_imask"].values,
                weights["dst_grid_frac"].values if "dst_grid_frac" in weights else None)
        op = weights_matrix
        n_batch = int(np.prod(kept_shape)) if kept_shape else 1
        masked = bool(np.asarray(masked).any()) if np.ndim(masked) else bool(masked)

        area_min, skipna = self.remap_area_min, self.skipna
        way, src = self._road(way, source_data, horizontal_dims, None, cf, cf_out, rule, out_dtype=out_dtype)
        out_dtype, ship_half, sb_in, sb_out = way.out_dtype, way.ship_half, way.sb_in, way.sb_out
        res_dtype = out_dtype if cf_out is None else cf_out.raw_dtype
        src_dtype = getattr(src, "dtype", None)
        grad_kw = {} if rule is None else {"gradients": rule}
        out_shape = (tgt_shape + kept_shape) if sb_out else (kept_shape + tgt_shape)
        out_dims = (tgt_dims + kept_dims) if sb_out else (kept_dims + tgt_dims)

        def apply_rows(host):
            """(rows, S) host block -> (rows, D): chunks stream through the library's H2D / kernel /
            D2H pipeline."""
            host = _host_rows(host, src_dtype, cf, ship_half)
            _check_cells(host.shape[1], op.n_src)
            return op.apply_host(host, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=skipna,
                                 cf=cf, cf_out=cf_out, half=ship_half, **grad_kw)

        def compute():
            if isinstance(src, GribField):
                # GRIB simple packing regridded raw (packed=True): the file's bytes and one rule per field go to the GPU
                _check_cells(src.n_points, op.n_src)
                if src.rows.size != n_batch:
                    raise ValueError(f"{src.rows.size} GRIB fields for {n_batch} batch rows of shape {tuple(kept_shape)}")
                # (with their bitmaps, if any: smm_apply_host_grib_bm ranks them on the device)
                # (CCSDS-packed fields: their streams are decoded on the device ahead of the gather, smm_grib_aec_unpack)
                # (complex-packed fields likewise: smm_grib_cpx_unpack; those with missing values inside their groups --
                # open_dataset(..., cpx_missing=True) -- through smm_grib_cpx_unpack_mv, which hands the gather a bitmap)
                packed = {}
                if way.result in road.GRIB_RESULTS:     # the result packed on the device, each field by its source's width and D
                    # (grib_out_ccsds: and its integers coded as CCSDS streams behind the pack; a CCSDS source goes in raw.
                    # grib_out_cpx: the same with complex packing)
                    packed["grib_out"] = GribEncode.from_field(src, ccsds=True if way.result == road.GRIB_CCSDS else None,
                                                               cpx=True if way.result == road.GRIB_CPX else None)
                y = op.apply_host_grib(src.buf, src.rows, masked=masked, remap_area_min=area_min, bitmaps=src.bitmaps,
                                       skipna=skipna, coded=src.coded, **packed)
                if packed:
                    return GribField(y.buf, y.rows, out_shape, op.n_dst, bitmaps=y.bitmaps, ccsds=y.ccsds, cpx=y.cpx)
                return y.reshape(out_shape)
            if isinstance(src, DeviceArray):
                # batch-fastest, (S, B): the batch values of a cell contiguous; else (B, S)
                x = src.reshape(-1, n_batch) if sb_in else src.reshape(n_batch, -1)
                _check_cells(x.shape[0 if sb_in else 1], op.n_src)
                y = op.apply(x, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=skipna, cf=cf,
                             cf_out=cf_out, **({"keep_batch_fastest": sb_out} if sb_in else grad_kw))
                return y.reshape(*out_shape)
            return apply_rows(_computed(src).reshape(n_batch, -1)).reshape(out_shape)

        if self.lazy and is_dask(src):
            # dask in, dask out: one task per block of the kept dimensions (regrid.py:538-541)
            out_data = map_batch_blocks(src, len(source_data.dims) - len(kept_dims), tgt_shape, apply_rows,
                                        dtype=res_dtype)
        elif self.lazy:
            out_data = LazyArray(out_shape, res_dtype, compute)
        else:
            out_data = compute()

        return self._finish(out_data, out_dims, source_data, kept_dims, weights,
                            tgt_shape, tgt_dims)

    # ------------------------------------------------------------------ apply (masked levels)
    def regrid3d(self, source_data, datagridtype, cf=None, cf_out=None, out_dtype=None, grib_out=False, way=None):
        """regrid.py:339-427 as one grouped launch: per data level the nearest
        weights level (tolerance 1e-3) selects operator, mask and frac.  cf: the CFDecode of a raw int16 / uint16
        field (packed=True, packed_levels=True); cf_out: the CFEncode its result is stored with (packed_out=True,
        packed_out_levels=True); grib_out: a raw GRIB variable comes back as a `GribField` in its own field order
        (grib_out_levels=True); way: the `road.Road` of this variable as `regrid_array` decided it (None, a direct call:
        decided here from these keywords)."""
        source_data = from_xarray(source_data)
        gridtype = self._get_gridtype(datagridtype)
        if gridtype is None:
            return DataArray(data=None)
        mask_dim = gridtype.mask_dim
        weights = gridtype.weights
        horizontal_dims = gridtype.horizontal_dims
        name = source_data.name or ''
        if "bnds" in name or "bounds" in name:
            return source_data
        if not any(x in source_data.dims for x in (horizontal_dims or [])):
            raise KeyError('Dimensions mismatch')

        wlev = np.asarray(weights.coords[mask_dim].values, dtype=np.float64)
        dlev = np.asarray(source_data.coords[mask_dim].values, dtype=np.float64)
        level_index = np.empty(dlev.size, dtype=np.int32)
        for idx, lev in enumerate(dlev):
            widx = int(np.argmin(np.abs(wlev - lev)))
            if not abs(wlev[widx] - lev) <= 1e-3:
                raise ValueError(f"{lev} not found in mask_dim {mask_dim}. "
                                 f"Available levels: {list(wlev)}")
            level_index[idx] = widx

        kept_dims = [d for d in source_data.dims if d not in horizontal_dims]
        p = kept_dims.index(mask_dim)
        outer_dims, inner_dims = kept_dims[:p], kept_dims[p + 1:]
        n_outer = int(np.prod([source_data.sizes[d] for d in outer_dims])) if outer_dims else 1
        n_inner = int(np.prod([source_data.sizes[d] for d in inner_dims])) if inner_dims else 1
        n_lev = source_data.sizes[mask_dim]
        rest_dims = outer_dims + inner_dims
        rest_shape = [source_data.sizes[d] for d in rest_dims]
        tgt_shape, tgt_dims = self._target_layout(weights)
        group = gridtype.group
        masked_levels = np.broadcast_to(np.asarray(gridtype.masked, dtype=bool),
                                        (len(group),)).astype(np.uint8)
        any_masked = bool(masked_levels.any())

        S, D = group.n_src, group.n_dst
        area_min, transpose, skipna = self.remap_area_min, self.transpose, self.skipna
        way, src = self._road(way, source_data, horizontal_dims, mask_dim, cf, cf_out, None, out_dtype=out_dtype,
                              grib_out=grib_out)
        out_dtype, ship_half, sb_in, sb_out = way.out_dtype, way.ship_half, way.sb_in, way.sb_out
        grib_out = way.result in road.GRIB_RESULTS
        # a GribField: one packed field per source field, in the source's order (no transpose); batch-fastest: the other
        # dims last; else the level axis behind the other dims (transpose) or ahead of them
        lead = kept_dims if grib_out else [mask_dim] if sb_out else rest_dims + [mask_dim] if transpose else [mask_dim] + rest_dims
        out_dims = lead + tgt_dims + (rest_dims if sb_out else [])
        out_shape = [source_data.sizes[d] for d in lead] + tgt_shape + (rest_shape if sb_out else [])

        def compute():
            if isinstance(src, GribField):
                # GRIB simple packing regridded raw (packed=True, packed_levels=True): the file's bytes, one rule per
                # field and the fields' bitmaps go to the GPU, all levels of a block of the outer axis in one launch
                _check_cells(src.n_points, S)
                if src.rows.size != n_outer * n_lev * n_inner:
                    raise ValueError(f"{src.rows.size} GRIB fields for batch rows of shape {(n_outer, n_lev, n_inner)}")
                dims3 = (n_outer, n_lev, n_inner)
                # grib_out: the result packed on the device, each field by its source's width and D, in the source's order
                y = group.apply_host_grib(src.buf, src.rows.reshape(dims3), level_index, masked_levels,
                                          bitmaps=None if src.bitmaps is None else src.bitmaps.reshape(dims3),
                                          masked=any_masked, remap_area_min=area_min, skipna=skipna,
                                          **({"grib_out": GribEncode.from_field(src)} if grib_out else {"transpose": transpose}))
                return GribField(y.buf, y.rows, out_shape, D, bitmaps=y.bitmaps) if grib_out else y.reshape(out_shape)
            if sb_in:
                x = src.reshape(n_lev, -1, n_outer * n_inner)
                _check_cells(x.shape[1], S)
                y = group.apply_sb(x, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                   transpose=transpose, out_dtype=out_dtype, keep_batch_fastest=sb_out, skipna=skipna,
                                   cf=cf, cf_out=cf_out)
                return y.reshape(*out_shape)
            if isinstance(src, DeviceArray):
                x = src.reshape(n_outer, n_lev, n_inner, -1)
                y = group.apply(x, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                transpose=transpose, out_dtype=out_dtype, skipna=skipna, cf=cf, cf_out=cf_out)
                return y.reshape(*out_shape)
            # (a dask field is computed here)
            host = _host_rows(_computed(src), src.dtype, cf, ship_half).reshape(n_outer, n_lev, n_inner, -1)
            _check_cells(host.shape[3], S)
            # host field: chunks of the outer axis stream through the group's pipeline
            out = group.apply_host(host, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                   transpose=transpose, out_dtype=out_dtype, skipna=skipna, cf=cf, cf_out=cf_out,
                                   half=ship_half)
            return out.reshape(out_shape)

        res_dtype = out_dtype if cf_out is None else cf_out.raw_dtype
        out_data = LazyArray(out_shape, res_dtype, compute) if self.lazy else compute()
        return self._finish(out_data, out_dims, source_data, kept_dims, weights, tgt_shape, tgt_dims)


def _computed(src):
    return src.compute() if hasattr(src, "compute") else np.asarray(src)


def _check_cells(n_cells, n_src):
    if n_cells != n_src:
        raise ValueError(f"source grid has {n_cells} cells, weights expect {n_src}")


def _host_rows(host, src_dtype, cf, ship_half):
    """A host block as the host entries take it: contiguous, promoted to float64 unless it is float32 / float64, raw
    integers with their rule, or half cells that ship as they are (`operator._host_field`).  A lazy field promised its
    chunks' dtype -- the result dtype was fixed from it -- so a half field whose chunk has another is refused."""
    host = np.asarray(host)
    if ship_half and host.dtype != src_dtype:
        raise ValueError(f"half=True: a chunk of dtype {host.dtype} in a field of dtype {src_dtype}")
    return np.ascontiguousarray(host if cf is not None else _host_field(host, None, ship_half))


def regrid(source_data, target_grid=None, weights=None, transpose=True, cdo='cdo'):
    """One-shot helper (regrid.py:656-677)."""
    regridder = Regridder(source_data, target_grid=target_grid, weights=weights, cdo=cdo,
                          transpose=transpose)
    return regridder.regrid(source_data)
