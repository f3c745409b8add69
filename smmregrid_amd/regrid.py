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

from .device import CFDecode, CFEncode, DeviceArray, bfloat16, is_half_dtype, is_packed_dtype, to_device
from .griblite import CCSDS, CPX, GribEncode, GribField
from .gridtype import GridType, tolist
from .lazy import LazyArray, is_dask, map_batch_blocks
from .operator import OperatorGroup
from .weights import (_level_slice, check_mask, compute_weights_matrix, compute_weights_matrix3d,
                      mask_weights)
from .xrlite import DataArray, Dataset, from_xarray, is_xarray, to_xarray

_CF_PACKING_ATTRS = ("scale_factor", "add_offset", "_FillValue", "missing_value")
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
                 grib_out_levels=False, grib_out_ccsds=False, grib_out_cpx=False, gradients=False):
        if (source_grid is None or target_grid is None) and (weights is None):
            raise ValueError("Either weights or source_grid/target_grid must be supplied")

        if vertical_dim is not None:  # deprecated_argument (util.py:23-40)
            import warnings
            warnings.warn("'vertical_dim' is deprecated, use 'mask_dim'", DeprecationWarning)
            if mask_dim is None:
                mask_dim = vertical_dim

        self.loggy = _logger(loglevel)
        self.loglevel = loglevel
        self.transpose = transpose
        self.device = device
        self.lazy = bool(lazy)
        # opt-in: links of weight exactly 0 (3 of 4 bilinear links between aligned grids) are dropped when
        # the operators are built; results are bit-identical (SMM_CREATE_PRUNE_ZEROS)
        self.prune_zero_weights = bool(prune_zero_weights)
        # Device-resident fields kept batch-fastest (`DeviceArray(..., layout="sb")`: horizontal
        # dimensions first, e.g. (lat, lon, time)) run through the batch-fastest kernel; with
        # keep_batch_fastest the result stays in that layout too -- (lat, lon, time) on the target grid,
        # HBM-resident -- so a second Regridder consumes it without a transpose.
        self.keep_batch_fastest = bool(keep_batch_fastest)
        # skipna: each time step's non-finite source values drop out of every sum they touch and the rest is
        # renormalised -- the weights regenerated with that step's validity as source mask (SMM_APPLY_SKIPNA);
        # remap_area_min then thresholds the valid fraction of each target cell
        self.skipna = bool(skipna)
        # packed: an int16 / uint16 variable that carries scale_factor / add_offset / _FillValue / missing_value (a
        # file opened undecoded: io.open_dataset(path, decode=False)) is regridded raw -- shipped and gathered as
        # 2-byte elements, decoded inside the kernels (CFDecode) -- with the bits of a host decode
        self.packed = bool(packed)
        # packed_levels (with packed=True): packed variables on masked-level (3-D) weights are regridded raw too,
        # through the level-group entries (smm_group_apply*_cf; a raw GRIB variable: smm_group_apply_host_grib).  Off by
        # default: such a variable is decoded on the host first, as before
        self.packed_levels = bool(packed_levels)
        if self.packed_levels and not self.packed:
            raise ValueError('packed_levels=True needs packed=True')
        # packed_skipna (with packed=True and skipna=True): a raw GRIB variable stays raw under skipna too -- the gather
        # renormalises over the cells its bitmap leaves and the values its rule keeps finite (smm_apply_host_grib_na;
        # with packed_levels=True on masked-level weights smm_group_apply_host_grib_na).  Off by default: such a variable
        # is decoded on the host first, as before
        self.packed_skipna = bool(packed_skipna)
        if self.packed_skipna and not (self.packed and self.skipna):
            raise ValueError('packed_skipna=True needs packed=True and skipna=True')
        # grib_out (with packed=True): a raw GRIB variable on 2-D weights comes back GRIB simple-packed -- a `GribField`
        # encoded on the device with each source field's own width and decimal scale (GribEncode.from_field;
        # smm_apply_host_grib_pk), 2 B per cell at 16 bits over PCIe -- which a second Regridder(packed=True) ships raw
        # again and np.asarray decodes to float32.  Every other variable comes back as without it, with one INFO line
        # (one on masked-level weights too, unless grib_out_levels=True)
        self.grib_out = bool(grib_out)
        if self.grib_out and not self.packed:
            raise ValueError('grib_out=True needs packed=True')
        if self.grib_out and self.lazy:
            raise ValueError('grib_out=True packs an eager result: it does not go with lazy=True')
        # grib_out_levels (with grib_out=True and packed_levels=True): a raw GRIB variable on masked-level (3-D) weights
        # comes back GRIB simple-packed too (smm_group_apply_host_grib_pk) -- a `GribField` with one packed field per
        # source field, in the source's own order: its dims are the variable's (outer..., level, inner...) followed by
        # the target's horizontal ones, whatever `transpose` says of a float result.  Off by default: such a variable
        # comes back float64 with the INFO line, as before
        self.grib_out_levels = bool(grib_out_levels)
        if self.grib_out_levels and not (self.grib_out and self.packed_levels):
            raise ValueError('grib_out_levels=True needs grib_out=True and packed_levels=True')
        # grib_out_ccsds (with grib_out=True): on 2-D weights the packed result is CCSDS-coded on the device behind the
        # pack (smm_grib_aec_pack; GribEncode.from_field(src, ccsds=True)): a simple-packed source gets block size 32, an
        # interval of 128 blocks and the preprocessor, a CCSDS-packed source keeps its own parameters and stays raw end
        # to end -- no host decode, no INFO line.  Masked-level weights keep the simple-packed result of grib_out_levels
        self.grib_out_ccsds = bool(grib_out_ccsds)
        if self.grib_out_ccsds and not self.grib_out:
            raise ValueError('grib_out_ccsds=True needs grib_out=True')
        # grib_out_cpx (with grib_out=True): on 2-D weights the packed result is complex-packed on the device behind the
        # pack (templates 5.2 / 5.3; smm_grib_cpx_pack; GribEncode.from_field(src, cpx=True)): a simple-packed source gets
        # second-order differencing in groups of 32, a complex-packed source keeps its own order, is packed at the width
        # its integers decode to and stays raw end to end -- no host decode, no INFO line.  Masked-level weights keep the
        # simple-packed result of grib_out_levels
        self.grib_out_cpx = bool(grib_out_cpx)
        if self.grib_out_cpx and not self.grib_out:
            raise ValueError('grib_out_cpx=True needs grib_out=True')
        if self.grib_out_cpx and self.grib_out_ccsds:
            raise ValueError('grib_out_cpx=True does not go with grib_out_ccsds=True: a result is coded one way')
        # packed_out (with packed=True): a variable regridded raw comes back in its own raw dtype, encoded by the rule
        # of its own attributes (CFEncode) inside the kernels' stores, and keeps its packing attributes: it can be
        # written straight to a file.  Values that round outside the raw range become the fill value (no wrap-around)
        self.packed_out = bool(packed_out)
        if self.packed_out and not self.packed:
            raise ValueError('packed_out=True needs packed=True')
        # packed_out_levels (with packed_out=True): on masked-level (3-D) weights the result is encoded inside the
        # level-group kernels too (smm_group_apply*_pk) -- a host result comes back over PCIe as 2-byte cells, a
        # device-resident one stays raw in HBM.  Off by default: a host result is then encoded on the host and a
        # device-resident one stays float64, as before
        self.packed_out_levels = bool(packed_out_levels)
        if self.packed_out_levels and not self.packed_out:
            raise ValueError('packed_out_levels=True needs packed_out=True')
        # half: host float16 / bfloat16 fields are shipped as their 2-byte cells and widened to float32 inside the
        # kernels (the bits of regridding field.astype(float32)), and without an explicit out_dtype the result has the
        # field's own half type.  Off by default: a host float16 field is promoted to float64 first, as before.
        # Device-resident half fields take the half path either way (they were an error before)
        self.half = bool(half)
        # the reference always yields float64 (result_type(x, f64)); float32 is an opt-in narrowing store, float16 /
        # bfloat16 a correctly rounded one (no float32 in between)
        self.out_dtype_given = out_dtype is not None
        self.out_dtype = np.dtype(np.float64 if out_dtype is None else out_dtype)
        if self.out_dtype not in (np.dtype(np.float32), np.dtype(np.float64)) and not is_half_dtype(self.out_dtype):
            raise ValueError('out_dtype must be float32 or float64')
        if self.packed_out and self.out_dtype != np.dtype(np.float64):
            raise ValueError('packed_out=True encodes the float64 result: out_dtype must stay float64')
        if self.grib_out and self.out_dtype != np.dtype(np.float64):
            raise ValueError('grib_out=True packs the float64 result: out_dtype must stay float64')
        # gradients: every weight column of bicubic (`bic`, num_wgts = 4) and second-order conservative (`con2`,
        # num_wgts = 3) weights is applied, not column 0 alone as the reference does: the gradients of each field are
        # computed on the device by the rule of `gradients.GradientRule` and gathered beside the field
        # (smm_apply_cols).  Beyond the reference, off by default; 2-D weights on a regular lon/lat source only
        self.gradients = bool(gradients)
        if self.gradients:
            clash = [name for name, on in (("skipna", self.skipna), ("packed", self.packed), ("half", self.half),
                                           ("keep_batch_fastest", self.keep_batch_fastest),
                                           (f"out_dtype={self.out_dtype}", self.out_dtype != np.dtype(np.float64))) if on]
            if clash:
                raise ValueError(f"gradients=True does not go with {', '.join(clash)}: it goes with float32 / float64 "
                                 "fields in the native layout (host, device-resident or lazy), float64 results, 2-D "
                                 "weights, remap_area_min, the destination mask, lazy and prune_zero_weights")
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
        was_grib = isinstance(source_data.data, GribField)
        if was_grib:
            source_data = self._grib_or_decoded(source_data, datagridtype)
        grib_out = self.grib_out and isinstance(source_data.data, GribField) and (not datagridtype.mask_dim
                                                                                 or self.grib_out_levels)
        if self.grib_out and not grib_out:
            why = ("masked levels" if isinstance(source_data.data, GribField)
                   else "decoded on the host" if was_grib else "not a raw GRIB variable")
            self.loggy.info("grib_out: %s comes back as without it (%s)", source_data.name, why)
        cf = self._packed_rule(source_data) if self.packed else None
        enc = self._packed_out_rule(source_data) if (self.packed_out and cf is not None) else None
        packing = {k: source_data.attrs[k] for k in _CF_PACKING_ATTRS if k in source_data.attrs}
        out_dtype = self._result_dtype(source_data)
        if cf is not None and is_half_dtype(out_dtype):
            raise ValueError(f"packed=True regrids {source_data.name} raw: its result is float64 or packed, "
                             "a half-precision out_dtype does not go with it")
        if cf is not None and ((datagridtype.mask_dim and not self.packed_levels)
                               or self.out_dtype != np.dtype(np.float64)):
            # float32 results take no packed input, level groups only with packed_levels=True: decoded on the host,
            # regridded as before
            self.loggy.info("packed variable %s is decoded on the host (%s)", source_data.name,
                            "masked levels" if datagridtype.mask_dim else "out_dtype float32")
            source_data = self._decode_on_host(source_data, cf)
            cf = None
        if datagridtype.mask_dim and self.packed_out_levels:
            out = self.regrid3d(source_data, datagridtype, cf=cf, cf_out=enc, out_dtype=out_dtype,   # encoded inside the
                                grib_out=grib_out)                                                   # group kernels
            if out.data is None:
                enc = None
        elif datagridtype.mask_dim:
            out = self.regrid3d(source_data, datagridtype, cf=cf, out_dtype=out_dtype, grib_out=grib_out)
            if enc is not None and out.data is not None:
                enc = self._encode_on_host(out, enc)      # None when the result stays float64 (device-resident)
        else:
            out = self.regrid2d(source_data, datagridtype, cf=cf, cf_out=enc, out_dtype=out_dtype)
        if enc is not None:
            out.attrs.update(packing)      # the result is raw again: it keeps the rule it was encoded with
        elif cf is not None:
            for k in _CF_PACKING_ATTRS:
                out.attrs.pop(k, None)
        return out

    def _result_dtype(self, source_data):
        """out_dtype of one variable: the Regridder's, or with half=True and no explicit out_dtype the own type of a
        float16 / bfloat16 field."""
        dtype = getattr(source_data.data, "dtype", None)
        if self.half and not self.out_dtype_given and is_half_dtype(dtype):
            return np.dtype(dtype)
        return self.out_dtype

    def _ships_half(self, dtype):
        """Whether a host field of `dtype` is handed to the host entries as it is (half=True; bfloat16 has no other way)."""
        return is_half_dtype(dtype) and (self.half or np.dtype(dtype) == bfloat16)

    def _grib_or_decoded(self, source_data, datagridtype):
        """A GRIB variable kept raw (`GribField`): with packed=True on 2-D weights and a float64 result it stays as it
        is and apply_weights ships its bit streams (smm_apply_host_grib, with bitmaps smm_apply_host_grib_bm); so it
        does on masked-level weights with packed_levels=True (regrid3d: smm_group_apply_host_grib) when its dims are
        (outer..., level, inner..., horizontal...).  Everything else decodes it on the host -- what np.asarray would do
        anyway -- and goes on as before.  Under skipna it stays raw with packed_skipna=True (the _na entries)."""
        why = self._grib_decode_reason(source_data.dims, datagridtype, self._result_dtype(source_data),
                                       bool(datagridtype.mask_dim), ccsds=source_data.data.ccsds is not None,
                                       cpx=source_data.data.cpx is not None)
        if why is None:
            return source_data
        if self.packed:
            self.loggy.info("packed variable %s is decoded on the host (%s)", source_data.name, why)
        return DataArray(source_data.data.decode(), dims=source_data.dims, coords=source_data.coords,
                         attrs=source_data.attrs, name=source_data.name)

    def _grib_decode_reason(self, dims, gridtype, out_dtype, levels, ccsds=False, cpx=False):
        """Why a `GribField` with these dims is decoded on the host, or None: it takes the raw road.  levels: it meets
        masked-level (3-D) weights.  ccsds, cpx: some of its fields are CCSDS-packed or complex-packed (`GribField.coded`)
        -- their road is the one of 2-D weights (the codec's unpack step ahead of the gather), and a packed result only
        coded the same way again (grib_out_ccsds, grib_out_cpx): the row record of a complex-packed field does not hold
        the width of its integers, which the device decode reports chunk by chunk.  The one
        condition behind `_grib_or_decoded` and the guards of `apply_weights` and `regrid3d`, which direct calls reach
        without it."""
        codec, coded_out = (CPX, getattr(self, "grib_out_cpx", False)) if cpx else \
            (CCSDS, getattr(self, "grib_out_ccsds", False)) if ccsds else (None, False)
        if not self.packed:
            return "packed=False"
        if codec is not None and levels:
            return f"{codec.packing} on masked levels"
        if codec is not None and self.grib_out and not coded_out:
            return f"{codec.packing} with grib_out"
        if levels and not self.packed_levels:
            return "masked levels"
        if self.skipna and not self.packed_skipna:
            return "skipna"
        if np.dtype(out_dtype) != np.dtype(np.float64):
            return f"out_dtype {np.dtype(out_dtype)}"
        if levels and not self._grib_rows_by_level(dims, gridtype):
            return "masked levels: its fields are not ordered (outer..., level, inner...)"
        return None

    @staticmethod
    def _grib_rows_by_level(dims, datagridtype):
        """Whether the fields of a GribField with these dims -- one per index of its leading dims, in C order -- are the
        (outer..., level, inner...) batch rows of the group entry: the mask dimension among the leading dims, the
        horizontal ones trailing."""
        horizontal = [d for d in dims if d in (datagridtype.horizontal_dims or [])]
        lead = list(dims[:len(dims) - len(horizontal)])
        return bool(horizontal) and datagridtype.mask_dim in lead and not any(d in horizontal for d in lead)

    def _packed_out_rule(self, source_data):
        """The CFEncode of a packed variable's own attributes, or None (one WARNING) when they name no fill value."""
        try:
            return CFEncode.from_attrs(source_data.attrs, source_data.data.dtype)
        except ValueError as err:
            self.loggy.warning("packed variable %s comes back as float64, not packed: %s", source_data.name, err)
            return None

    def _encode_on_host(self, out, enc):
        """packed_out on masked-level (3-D) weights without packed_out_levels: a host result is encoded here with the
        same rule (the same bits as the level-group _pk entries give); a device-resident one stays float64."""
        data = out.data
        if isinstance(data, DeviceArray):
            self.loggy.warning("packed_out: the device-resident result of %s on masked-level weights stays float64",
                               out.name)
            return None
        self.loggy.info("packed_out: %s on masked-level weights is encoded on the host", out.name)
        if isinstance(data, LazyArray):
            out.data = LazyArray(data.shape, enc.raw_dtype, lambda: enc.encode(data.compute()))
        else:
            out.data = enc.encode(np.asarray(data))
        return enc

    def _packed_rule(self, source_data):
        """The CFDecode of a 2-byte integer variable that carries CF packing attributes, else None."""
        dtype = getattr(source_data.data, "dtype", None)
        if dtype is None or not is_packed_dtype(dtype) or not any(k in source_data.attrs for k in _CF_PACKING_ATTRS):
            return None
        try:
            return CFDecode.from_attrs(source_data.attrs, raw_dtype=dtype)
        except ValueError as err:      # more than two distinct fill values: the field is regridded as it was before
            self.loggy.warning("packed variable %s is not regridded raw: %s", source_data.name, err)
            return None

    @staticmethod
    def _decode_on_host(source_data, cf):
        src = source_data.data
        if isinstance(src, DeviceArray):
            data = to_device(cf.decode(src.to_host()), layout=src.layout)
        else:
            data = cf.decode(src.compute() if hasattr(src, "compute") else np.asarray(src))
        attrs = {k: v for k, v in source_data.attrs.items() if k not in _CF_PACKING_ATTRS}
        return DataArray(data, dims=source_data.dims, coords=source_data.coords, attrs=attrs, name=source_data.name)

    def _get_gridtype(self, datagridtype):
        """regrid.py:324-337."""
        if self.init_mode == 'weights':
            self.grids[0].dims = datagridtype.dims
            self.grids[0].horizontal_dims = datagridtype.horizontal_dims
            self.grids[0].other_dims = datagridtype.other_dims
        return next((grid for grid in self.grids if grid == datagridtype), None)

    def regrid2d(self, source_data, datagridtype, cf=None, cf_out=None, out_dtype=None):
        """regrid.py:429-456."""
        gridtype = self._get_gridtype(datagridtype)
        if gridtype is None:
            return DataArray(data=None)
        return self.apply_weights(source_data, gridtype.weights,
                                  weights_matrix=gridtype.weights_matrix,
                                  masked=gridtype.masked,
                                  horizontal_dims=gridtype.horizontal_dims, cf=cf, cf_out=cf_out, out_dtype=out_dtype,
                                  gradients=getattr(gridtype, "grad_rule", None))

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

    def apply_weights(self, source_data, weights, weights_matrix=None, masked=True,
                      horizontal_dims=None, cf=None, cf_out=None, out_dtype=None, gradients=None):
        """regrid.py:458-628 for one 2-D operator.  cf: the CFDecode of a raw int16 / uint16 field (packed=True);
        cf_out: the CFEncode its result is stored with (packed_out=True); out_dtype: this variable's result dtype
        (None: the Regridder's, or the field's own half type under half=True); gradients: the `GradientRule` of these
        weights (Regridder(gradients=True); None there: made from `weights`)."""
        source_data = from_xarray(source_data)
        if out_dtype is None:
            out_dtype = self._result_dtype(source_data)
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
        if rule is None and getattr(self, "gradients", False):
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

        src = source_data.data
        area_min, skipna = self.remap_area_min, self.skipna
        if isinstance(src, GribField) and self._grib_decode_reason(source_data.dims, None, out_dtype, False,
                                                                   ccsds=src.ccsds is not None, cpx=src.cpx is not None):
            src = src.decode()      # a direct call: only the raw road of _grib_or_decoded ships the bit streams
        res_dtype = out_dtype if cf_out is None else cf_out.raw_dtype
        src_dtype = getattr(src, "dtype", None)
        ship_half = self._ships_half(src_dtype)
        sb_in = isinstance(src, DeviceArray) and src.layout == "sb"
        if sb_in:
            n_h = len(source_data.dims) - len(kept_dims)
            if any(d not in horizontal_dims for d in source_data.dims[:n_h]):
                raise ValueError("a batch-fastest field (layout='sb') carries its horizontal dimensions first, "
                                 f"got dims {tuple(source_data.dims)}")
        elif self.keep_batch_fastest:
            raise ValueError("keep_batch_fastest needs a device-resident batch-fastest field "
                             "(source_data.data = DeviceArray(..., layout='sb'))")
        if rule is not None and sb_in:
            raise ValueError("gradients=True does not go with a batch-fastest field (layout='sb'): it goes with float32 / "
                             "float64 fields in the native layout (host, device-resident or lazy)")
        grad_kw = {} if rule is None else {"gradients": rule}
        sb_out = sb_in and self.keep_batch_fastest
        out_shape = (tgt_shape + kept_shape) if sb_out else (kept_shape + tgt_shape)
        out_dims = (tgt_dims + kept_dims) if sb_out else (kept_dims + tgt_dims)

        def apply_rows(host):
            """(rows, S) host block -> (rows, D): chunks stream through the library's H2D / kernel /
            D2H pipeline."""
            host = np.asarray(host)
            if ship_half and host.dtype != src_dtype:
                # a lazy field promised half-precision chunks (the result dtype was fixed from that): no silent promotion
                raise ValueError(f"half=True: a chunk of dtype {host.dtype} in a field of dtype {src_dtype}")
            if cf is None and host.dtype not in (np.float32, np.float64) and not ship_half:
                host = host.astype(np.float64)  # result_type(x, f64), regrid.py:550
            host = np.ascontiguousarray(host)
            if host.shape[1] != op.n_src:
                raise ValueError(f"source grid has {host.shape[1]} cells, weights expect {op.n_src}")
            return op.apply_host(host, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=skipna,
                                 cf=cf, cf_out=cf_out, half=ship_half, **grad_kw)

        def compute():
            if isinstance(src, GribField):
                # GRIB simple packing regridded raw (packed=True): the file's bytes and one rule per field go to the GPU
                if src.n_points != op.n_src:
                    raise ValueError(f"source grid has {src.n_points} cells, weights expect {op.n_src}")
                if src.rows.size != n_batch:
                    raise ValueError(f"{src.rows.size} GRIB fields for {n_batch} batch rows of shape {tuple(kept_shape)}")
                # (with their bitmaps, if any: smm_apply_host_grib_bm ranks them on the device)
                if self.grib_out:     # the result packed on the device, each field by its source's width and D
                    # (grib_out_ccsds: and its integers coded as CCSDS streams behind the pack; a CCSDS source goes in raw.
                    # grib_out_cpx: the same with complex packing)
                    enc = GribEncode.from_field(src, ccsds=True if self.grib_out_ccsds else None,
                                                cpx=True if self.grib_out_cpx else None)
                    y = op.apply_host_grib(src.buf, src.rows, masked=masked, remap_area_min=area_min, bitmaps=src.bitmaps,
                                           skipna=skipna, grib_out=enc, coded=src.coded)
                    return GribField(y.buf, y.rows, kept_shape + tgt_shape, op.n_dst, bitmaps=y.bitmaps, ccsds=y.ccsds,
                                     cpx=y.cpx)
                # (CCSDS-packed fields: their streams are decoded on the device ahead of the gather, smm_grib_aec_unpack)
                # (complex-packed fields likewise: smm_grib_cpx_unpack; those with missing values inside their groups --
                # open_dataset(..., cpx_missing=True) -- through smm_grib_cpx_unpack_mv, which hands the gather a bitmap)
                y = op.apply_host_grib(src.buf, src.rows, masked=masked, remap_area_min=area_min, bitmaps=src.bitmaps,
                                       skipna=skipna, coded=src.coded)
                return y.reshape(kept_shape + tgt_shape)
            if sb_in:
                x = src.reshape(-1, n_batch)                  # (S, B): the batch values of a cell contiguous
                if x.shape[0] != op.n_src:
                    raise ValueError(f"source grid has {x.shape[0]} cells, weights expect {op.n_src}")
                y = op.apply(x, masked=masked, remap_area_min=area_min, out_dtype=out_dtype,
                             keep_batch_fastest=sb_out, skipna=skipna, cf=cf, cf_out=cf_out)
                return y.reshape(*out_shape)
            if isinstance(src, DeviceArray):
                x = src.reshape(n_batch, -1)
                if x.shape[1] != op.n_src:
                    raise ValueError(f"source grid has {x.shape[1]} cells, weights expect {op.n_src}")
                y = op.apply(x, masked=masked, remap_area_min=area_min, out_dtype=out_dtype, skipna=skipna, cf=cf,
                             cf_out=cf_out, **grad_kw)
                return y.reshape(*(kept_shape + tgt_shape))
            host = src.compute() if isinstance(src, LazyArray) else np.asarray(src)
            return apply_rows(host.reshape(n_batch, -1)).reshape(kept_shape + tgt_shape)

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
    def regrid3d(self, source_data, datagridtype, cf=None, cf_out=None, out_dtype=None, grib_out=False):
        """regrid.py:339-427 as one grouped launch: per data level the nearest
        weights level (tolerance 1e-3) selects operator, mask and frac.  cf: the CFDecode of a raw int16 / uint16
        field (packed=True, packed_levels=True); cf_out: the CFEncode its result is stored with (packed_out=True,
        packed_out_levels=True); grib_out: a raw GRIB variable comes back as a `GribField` in its own field order
        (grib_out_levels=True)."""
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

        if self.transpose:
            out_dims = rest_dims + [mask_dim] + tgt_dims
            out_shape = rest_shape + [n_lev] + tgt_shape
        else:
            out_dims = [mask_dim] + rest_dims + tgt_dims
            out_shape = [n_lev] + rest_shape + tgt_shape

        src = source_data.data
        S, D = group.n_src, group.n_dst
        area_min, transpose = self.remap_area_min, self.transpose
        if out_dtype is None:
            out_dtype = self._result_dtype(source_data)
        skipna = self.skipna
        if isinstance(src, GribField) and self._grib_decode_reason(source_data.dims, gridtype, out_dtype, True,
                                                                   ccsds=src.ccsds is not None, cpx=src.cpx is not None):
            src = src.decode()      # a direct call: only the raw road of _grib_or_decoded ships the bit streams
        grib_out = bool(grib_out) and isinstance(src, GribField) and not self.lazy
        if grib_out:      # one packed field per source field, in the source's order: no transpose
            out_dims = kept_dims + tgt_dims
            out_shape = [source_data.sizes[d] for d in kept_dims] + tgt_shape
        ship_half = self._ships_half(getattr(src, "dtype", None))
        sb_in = isinstance(src, DeviceArray) and src.layout == "sb"
        if sb_in:
            # batch-fastest per level: (mask_dim, horizontal..., everything else...)
            n_h = len(source_data.dims) - len(kept_dims)
            if source_data.dims[0] != mask_dim or any(d not in horizontal_dims for d in source_data.dims[1:1 + n_h]):
                raise ValueError("a batch-fastest masked field (layout='sb') is laid out (mask_dim, horizontal "
                                 f"dims..., other dims...), got dims {tuple(source_data.dims)}")
        elif self.keep_batch_fastest:
            raise ValueError("keep_batch_fastest needs a device-resident batch-fastest field "
                             "(source_data.data = DeviceArray(..., layout='sb'))")
        sb_out = sb_in and self.keep_batch_fastest
        if sb_out:
            out_dims = [mask_dim] + tgt_dims + rest_dims
            out_shape = [n_lev] + tgt_shape + rest_shape

        def compute():
            if isinstance(src, GribField):
                # GRIB simple packing regridded raw (packed=True, packed_levels=True): the file's bytes, one rule per
                # field and the fields' bitmaps go to the GPU, all levels of a block of the outer axis in one launch
                if src.n_points != S:
                    raise ValueError(f"source grid has {src.n_points} cells, weights expect {S}")
                if src.rows.size != n_outer * n_lev * n_inner:
                    raise ValueError(f"{src.rows.size} GRIB fields for batch rows of shape {(n_outer, n_lev, n_inner)}")
                dims3 = (n_outer, n_lev, n_inner)
                if grib_out:     # the result packed on the device, each field by its source's width and D
                    y = group.apply_host_grib(src.buf, src.rows.reshape(dims3), level_index, masked_levels,
                                              bitmaps=None if src.bitmaps is None else src.bitmaps.reshape(dims3),
                                              masked=any_masked, remap_area_min=area_min, skipna=skipna,
                                              grib_out=GribEncode.from_field(src))
                    return GribField(y.buf, y.rows, out_shape, D, bitmaps=y.bitmaps)
                out = group.apply_host_grib(src.buf, src.rows.reshape(dims3), level_index, masked_levels,
                                            bitmaps=None if src.bitmaps is None else src.bitmaps.reshape(dims3),
                                            masked=any_masked, remap_area_min=area_min, transpose=transpose, skipna=skipna)
                return out.reshape(out_shape)
            if sb_in:
                x = src.reshape(n_lev, -1, n_outer * n_inner)
                if x.shape[1] != S:
                    raise ValueError(f"source grid has {x.shape[1]} cells, weights expect {S}")
                y = group.apply_sb(x, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                   transpose=transpose, out_dtype=out_dtype, keep_batch_fastest=sb_out, skipna=skipna,
                                   cf=cf, cf_out=cf_out)
                return y.reshape(*out_shape)
            if isinstance(src, DeviceArray):
                x = src.reshape(n_outer, n_lev, n_inner, -1)
                y = group.apply(x, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                transpose=transpose, out_dtype=out_dtype, skipna=skipna, cf=cf, cf_out=cf_out)
                return y.reshape(*out_shape)
            host = src.compute() if isinstance(src, LazyArray) else np.asarray(src)   # a dask field is computed here
            if ship_half and host.dtype != src.dtype:
                raise ValueError(f"half=True: a chunk of dtype {host.dtype} in a field of dtype {src.dtype}")
            if cf is None and host.dtype not in (np.float32, np.float64) and not ship_half:
                host = host.astype(np.float64)
            host = np.ascontiguousarray(host).reshape(n_outer, n_lev, n_inner, -1)
            if host.shape[3] != S:
                raise ValueError(f"source grid has {host.shape[3]} cells, weights expect {S}")
            # host field: chunks of the outer axis stream through the group's pipeline
            out = group.apply_host(host, level_index, masked_levels, masked=any_masked, remap_area_min=area_min,
                                   transpose=transpose, out_dtype=out_dtype, skipna=skipna, cf=cf, cf_out=cf_out,
                                   half=ship_half)
            return out.reshape(out_shape)

        res_dtype = out_dtype if cf_out is None else cf_out.raw_dtype
        out_data = LazyArray(out_shape, res_dtype, compute) if self.lazy else compute()

        kept_for_coords = kept_dims
        w2d = weights
        return self._finish(out_data, out_dims, source_data, kept_for_coords, w2d, tgt_shape, tgt_dims)


def regrid(source_data, target_grid=None, weights=None, transpose=True, cdo='cdo'):
    """One-shot helper (regrid.py:656-677)."""
    regridder = Regridder(source_data, target_grid=target_grid, weights=weights, cdo=cdo,
                          transpose=transpose)
    return regridder.regrid(source_data)
