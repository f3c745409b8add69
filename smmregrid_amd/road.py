"""Which road a variable takes through the Regridder, decided once: `decide(switches, facts)` is a pure function over
plain values -- the Regridder's switches, what is known of a variable without touching its values -- and returns a
`Road` that `regrid.py` carries out: the log lines to emit, the host decode to perform, the operator entry to call.
Nothing here touches a device, a file or a field's values.
"""
from collections import namedtuple

import numpy as np

F64 = np.dtype(np.float64)
BFLOAT16 = np.dtype([("bfloat16", "<u2")])      # `device.bfloat16`: the project's 2-byte dtype, equal by structure
_HALF = (np.dtype(np.float16), BFLOAT16)
CF_PACKING_ATTRS = ("scale_factor", "add_offset", "_FillValue", "missing_value")


def is_half(dtype):
    return dtype is not None and np.dtype(dtype) in _HALF


# ------------------------------------------------------------------------------------------------ the switches
class Switches(namedtuple("Switches", "lazy skipna keep_batch_fastest transpose out_dtype out_dtype_given packed "
                                      "packed_levels packed_skipna packed_out packed_out_levels half grib_out "
                                      "grib_out_levels grib_out_ccsds grib_out_cpx gradients categorical")):
    """The Regridder's switches as one immutable value.

    lazy: nothing is launched before ``.values`` / ``.compute()`` (see `lazy`).
    keep_batch_fastest: device-resident fields kept batch-fastest (`DeviceArray(..., layout="sb")`: horizontal
      dimensions first, e.g. (lat, lon, time)) run through the batch-fastest kernel; with keep_batch_fastest the result
      stays in that layout too -- (lat, lon, time) on the target grid, HBM-resident -- so a second Regridder consumes it
      without a transpose.
    skipna: each time step's non-finite source values drop out of every sum they touch and the rest is renormalised --
      the weights regenerated with that step's validity as source mask (SMM_APPLY_SKIPNA); remap_area_min then
      thresholds the valid fraction of each target cell.
    transpose: on masked-level weights the level axis of the result follows the other kept dims (regrid.py:420-427 of
      the reference); off, it leads (the concat order, regrid.py:410).
    out_dtype: the reference always yields float64 (result_type(x, f64)); float32 is an opt-in narrowing store,
      float16 / bfloat16 a correctly rounded one (no float32 in between).  out_dtype_given: it was named by the caller.
    packed: an int16 / uint16 variable that carries scale_factor / add_offset / _FillValue / missing_value (a file
      opened undecoded: io.open_dataset(path, decode=False)) is regridded raw -- shipped and gathered as 2-byte
      elements, decoded inside the kernels (CFDecode) -- with the bits of a host decode.
    packed_levels (with packed=True): packed variables on masked-level (3-D) weights are regridded raw too, through the
      level-group entries (smm_group_apply*_cf; a raw GRIB variable: smm_group_apply_host_grib).  Off by default: such
      a variable is decoded on the host first, as before.
    packed_skipna (with packed=True and skipna=True): a raw GRIB variable stays raw under skipna too -- the gather
      renormalises over the cells its bitmap leaves and the values its rule keeps finite (smm_apply_host_grib_na; with
      packed_levels=True on masked-level weights smm_group_apply_host_grib_na).  Off by default: such a variable is
      decoded on the host first, as before.
    grib_out (with packed=True): a raw GRIB variable on 2-D weights comes back GRIB simple-packed -- a `GribField`
      encoded on the device with each source field's own width and decimal scale (GribEncode.from_field;
      smm_apply_host_grib_pk), 2 B per cell at 16 bits over PCIe -- which a second Regridder(packed=True) ships raw
      again and np.asarray decodes to float32.  Every other variable comes back as without it, with one INFO line (one
      on masked-level weights too, unless grib_out_levels=True).
    grib_out_levels (with grib_out=True and packed_levels=True): a raw GRIB variable on masked-level (3-D) weights
      comes back GRIB simple-packed too (smm_group_apply_host_grib_pk) -- a `GribField` with one packed field per
      source field, in the source's own order: its dims are the variable's (outer..., level, inner...) followed by the
      target's horizontal ones, whatever `transpose` says of a float result.  Off by default: such a variable comes
      back float64 with the INFO line, as before.
    grib_out_ccsds (with grib_out=True): on 2-D weights the packed result is CCSDS-coded on the device behind the pack
      (smm_grib_aec_pack; GribEncode.from_field(src, ccsds=True)): a simple-packed source gets block size 32, an
      interval of 128 blocks and the preprocessor, a CCSDS-packed source keeps its own parameters and stays raw end to
      end -- no host decode, no INFO line.  Masked-level weights keep the simple-packed result of grib_out_levels.
    grib_out_cpx (with grib_out=True): on 2-D weights the packed result is complex-packed on the device behind the
      pack (templates 5.2 / 5.3; smm_grib_cpx_pack; GribEncode.from_field(src, cpx=True)): a simple-packed source gets
      second-order differencing in groups of 32, a complex-packed source keeps its own order, is packed at the width
      its integers decode to and stays raw end to end -- no host decode, no INFO line.  Masked-level weights keep the
      simple-packed result of grib_out_levels.
    packed_out (with packed=True): a variable regridded raw comes back in its own raw dtype, encoded by the rule of its
      own attributes (CFEncode) inside the kernels' stores, and keeps its packing attributes: it can be written
      straight to a file.  Values that round outside the raw range become the fill value (no wrap-around).
    packed_out_levels (with packed_out=True): on masked-level (3-D) weights the result is encoded inside the
      level-group kernels too (smm_group_apply*_pk) -- a host result comes back over PCIe as 2-byte cells, a
      device-resident one stays raw in HBM.  Off by default: a host result is then encoded on the host and a
      device-resident one stays float64, as before.
    half: host float16 / bfloat16 fields are shipped as their 2-byte cells and widened to float32 inside the kernels
      (the bits of regridding field.astype(float32)), and without an explicit out_dtype the result has the field's own
      half type.  Off by default: a host float16 field is promoted to float64 first, as before.  Device-resident half
      fields take the half path either way (they were an error before).
    gradients: every weight column of bicubic (`bic`, num_wgts = 4) and second-order conservative (`con2`,
      num_wgts = 3) weights is applied, not column 0 alone as the reference does: the gradients of each field are
      computed on the device by the rule of `gradients.GradientRule` and gathered beside the field (smm_apply_cols).
      Beyond the reference, off by default; 2-D weights on a regular lon/lat source only.
    categorical: variables of class codes (every variable, or those the Regridder was given by name) are regridded by
      largest area fraction -- per target cell the class whose source cells cover the largest summed share of it
      (`categorical.ModeRule`; smm_apply_mode) -- and come back in their own dtype with their attributes.  Meant for
      conservative weights (`method="laf"` weights are the one-cell approximation of it).  Beyond the reference, off by
      default; host fields and native-layout DeviceArrays on 2-D weights."""
    __slots__ = ()

    @classmethod
    def of(cls, out_dtype=None, transpose=True, **on):
        """From the constructor's keywords: every switch as a bool, out_dtype as a numpy dtype (None: float64)."""
        return cls(out_dtype=np.dtype(np.float64 if out_dtype is None else out_dtype), out_dtype_given=out_dtype is not None,
                   transpose=transpose, **{name: bool(on.get(name, False)) for name in cls._fields
                                           if name not in ("out_dtype", "out_dtype_given", "transpose")})

    # the conditions beside the switches that the table below speaks of
    always = True
    out_dtype_built = property(lambda self: self.out_dtype in (np.dtype(np.float32), F64) or is_half(self.out_dtype))
    out_dtype_narrow = property(lambda self: self.out_dtype != F64)


NEEDS, EXCLUDES = "needs", "excludes"
# (switch, needs all of / excludes each of, the others, the refusal), walked in order: the first that applies wins
PREREQUISITES = (
    ("packed_levels", NEEDS, ("packed",), "packed_levels=True needs packed=True"),
    ("packed_skipna", NEEDS, ("packed", "skipna"), "packed_skipna=True needs packed=True and skipna=True"),
    ("grib_out", NEEDS, ("packed",), "grib_out=True needs packed=True"),
    ("grib_out", EXCLUDES, ("lazy",), "grib_out=True packs an eager result: it does not go with lazy=True"),
    ("grib_out_levels", NEEDS, ("grib_out", "packed_levels"), "grib_out_levels=True needs grib_out=True and packed_levels=True"),
    ("grib_out_ccsds", NEEDS, ("grib_out",), "grib_out_ccsds=True needs grib_out=True"),
    ("grib_out_cpx", NEEDS, ("grib_out",), "grib_out_cpx=True needs grib_out=True"),
    ("grib_out_cpx", EXCLUDES, ("grib_out_ccsds",), "grib_out_cpx=True does not go with grib_out_ccsds=True: a result is coded one way"),
    ("packed_out", NEEDS, ("packed",), "packed_out=True needs packed=True"),
    ("packed_out_levels", NEEDS, ("packed_out",), "packed_out_levels=True needs packed_out=True"),
    ("always", NEEDS, ("out_dtype_built",), "out_dtype must be float32 or float64"),
    ("packed_out", EXCLUDES, ("out_dtype_narrow",), "packed_out=True encodes the float64 result: out_dtype must stay float64"),
    ("grib_out", EXCLUDES, ("out_dtype_narrow",), "grib_out=True packs the float64 result: out_dtype must stay float64"),
    ("gradients", EXCLUDES, ("skipna", "packed", "half", "keep_batch_fastest", "out_dtype_narrow"),
     "gradients=True does not go with {clash}: it goes with float32 / float64 fields in the native layout (host, "
     "device-resident or lazy), float64 results, 2-D weights, remap_area_min, the destination mask, lazy and "
     "prune_zero_weights"),
    ("categorical", EXCLUDES, ("skipna", "packed", "packed_levels", "packed_skipna", "packed_out", "packed_out_levels", "half",
                               "keep_batch_fastest", "gradients", "grib_out", "grib_out_levels", "grib_out_ccsds",
                               "grib_out_cpx", "lazy", "out_dtype_given"),
     "categorical does not go with {clash}: a class variable comes back in its own dtype, eagerly, by largest area "
     "fraction; it goes with host arrays and native-layout DeviceArrays, 2-D weights, remap_area_min, the destination "
     "mask and prune_zero_weights"),
)


def refusal(switches):
    """The message of the first prerequisite or clash of `PREREQUISITES` the switches break, or None."""
    for switch, kind, others, message in PREREQUISITES:
        if not getattr(switches, switch):
            continue
        clash = [f"out_dtype={switches.out_dtype}" if o in ("out_dtype_narrow", "out_dtype_given") else o
                 for o in others if getattr(switches, o)]
        if (kind == NEEDS and len(clash) < len(others)) or (kind == EXCLUDES and clash):
            return message.format(clash=", ".join(clash))
    return None


# ------------------------------------------------------------------------------------------------ the facts of a variable
HOST, LAZY, DASK, BS, SB, GRIB = "host", "lazy", "dask", "bs", "sb", "grib"


class Facts(namedtuple("Facts", "name held dtype dims horizontal_dims mask_dim cf cf_out codec grad_rule direct out_dtype "
                                "grib_out categorical", defaults=(False, False, None, False, False, None, False, False))):
    """What is known of a variable without touching its values.
    held: HOST (a numpy array), LAZY (a `LazyArray`), DASK, BS / SB (a `DeviceArray` of that layout) or GRIB (a
    `GribField`); dtype, dims: the variable's; horizontal_dims: those of its dims the weights regrid; mask_dim: the
    level dimension when it meets masked-level (3-D) weights, else None.
    cf / cf_out: a `CFDecode` / `CFEncode` of its attributes stands ready (packed / packed_out were on and the rule could
    be built); codec: of a `GribField`, None (simple packing only), "ccsds" or "cpx"; grad_rule: its grid has a
    `GradientRule`.
    direct: `apply_weights` / `regrid3d` were called directly -- the caller chose cf, cf_out, out_dtype (None: by the
    switches) and, on masked-level weights, grib_out itself; nothing is logged and no packed field is decoded.
    categorical: the variable is one of those `Regridder(categorical=...)` regrids by largest area fraction."""
    __slots__ = ()

    @property
    def levels(self):
        return self.mask_dim is not None

    @property
    def rows_by_level(self):
        """Whether the fields of a GribField with these dims -- one per index of its leading dims, in C order -- are the
        (outer..., level, inner...) batch rows of the group entry: the mask dimension among the leading dims, the
        horizontal ones trailing."""
        horizontal = [d for d in self.dims if d in self.horizontal_dims]
        lead = list(self.dims[:len(self.dims) - len(horizontal)])
        return bool(horizontal) and self.mask_dim in lead and not any(d in horizontal for d in lead)


# ------------------------------------------------------------------------------------------------ the road
# source roads: the field as it is (PLAIN: float32 / float64), its raw GRIB bit streams, its raw CF-packed integers, its
# 2-byte half cells; DECODED on the host first (`why` says why), PROMOTED to float64 on the host (result_type(x, f64))
PLAIN, RAW_GRIB, RAW_CF, HALF, DECODED, PROMOTED = "plain", "raw GRIB", "raw CF", "half", "decoded", "promoted"
# result roads: float cells of `out_dtype`; CF-encoded in the kernels' stores or on the host, or left float64 on the device
# (packed_out on masked-level weights without packed_out_levels); a `GribField` packed on the device
FLOAT, CF_KERNEL, CF_HOST, FLOAT64_DEVICE = "float", "CF in the kernel", "CF on the host", "float64 on the device"
GRIB_SIMPLE, GRIB_CCSDS, GRIB_CPX = "GRIB simple", "GRIB CCSDS", "GRIB complex"
GRIB_RESULTS = (GRIB_SIMPLE, GRIB_CCSDS, GRIB_CPX)
# a class variable (categorical): its codes as they are, and the class of largest area fraction in the field's own dtype
CLASS_CODES, MODE = "class codes", "mode"
# a refusal is (stage, message), a ValueError: of the VARIABLE, raised before anything is done with it, or of its LAYOUT,
# raised where the apply has found its dims and operator
VARIABLE, LAYOUT = "variable", "layout"
INFO, WARNING = "info", "warning"


class Road(namedtuple("Road", "source why result out_dtype ship_half sb_in sb_out gradients refusal lines after")):
    """source, why, result: see above; out_dtype: the variable's result dtype (of the float64 result a CF or GRIB result
    road encodes); ship_half: a host field's 2-byte half cells are handed over as they are; sb_in / sb_out: the field /
    the result is batch-fastest; gradients: every weight column is applied; refusal: None or (stage, message); lines:
    (level, text) pairs to log before the apply, after: those to log once it has given a result."""
    __slots__ = ()


_CODEC_WORDS = {"ccsds": ("CCSDS packing", "grib_out_ccsds"), "cpx": ("complex packing", "grib_out_cpx")}


def _why_grib_decodes(s, f, out_dtype):
    """Why a `GribField` is decoded on the host, or None: it takes the raw road.  CCSDS-packed or complex-packed fields
    (f.codec) take the road of 2-D weights only (the codec's unpack step ahead of the gather), and a packed result only
    coded the same way again (grib_out_ccsds, grib_out_cpx): the row record of a complex-packed field does not hold the
    width of its integers, which the device decode reports chunk by chunk."""
    packing, coded_out = _CODEC_WORDS.get(f.codec, (None, None))
    if not s.packed:
        return "packed=False"
    if packing is not None and f.levels:
        return f"{packing} on masked levels"
    if packing is not None and s.grib_out and not getattr(s, coded_out):
        return f"{packing} with grib_out"
    if f.levels and not s.packed_levels:
        return "masked levels"
    if s.skipna and not s.packed_skipna:
        return "skipna"
    if out_dtype != F64:
        return f"out_dtype {out_dtype}"
    if f.levels and not f.rows_by_level:
        return "masked levels: its fields are not ordered (outer..., level, inner...)"
    return None


def _layout_refusal(s, f, sb_in):
    n_h = sum(d in f.horizontal_dims for d in f.dims)
    if sb_in and f.levels:      # batch-fastest per level: (mask_dim, horizontal..., everything else...)
        if f.dims[0] != f.mask_dim or any(d not in f.horizontal_dims for d in f.dims[1:1 + n_h]):
            return ("a batch-fastest masked field (layout='sb') is laid out (mask_dim, horizontal dims..., other dims...), "
                    f"got dims {tuple(f.dims)}")
    elif sb_in:
        if any(d not in f.horizontal_dims for d in f.dims[:n_h]):
            return f"a batch-fastest field (layout='sb') carries its horizontal dimensions first, got dims {tuple(f.dims)}"
    elif s.keep_batch_fastest:
        return ("keep_batch_fastest needs a device-resident batch-fastest field "
                "(source_data.data = DeviceArray(..., layout='sb'))")
    if f.grad_rule and sb_in and not f.levels:
        return ("gradients=True does not go with a batch-fastest field (layout='sb'): it goes with float32 / float64 "
                "fields in the native layout (host, device-resident or lazy)")
    return None


def _decide_categorical(f):
    """The road of a class variable: its codes as they are through the mode entries, or the refusal of what they are not
    built for -- raw GRIB fields, batch-fastest fields, masked-level (3-D) weights."""
    clash = "a GribField (raw GRIB input)" if f.held == GRIB else "a batch-fastest field (layout='sb')" if f.held == SB else \
        "masked-level (3-D) weights" if f.levels else None
    refused = None if clash is None else (VARIABLE, f"categorical does not go with {clash}: {f.name} is regridded by largest "
                                                    "area fraction as a host array or a native-layout DeviceArray on 2-D weights")
    return Road(CLASS_CODES, None, MODE, None if f.dtype is None else np.dtype(f.dtype), False, False, False, False, refused,
                (), ())


def decide(s, f):
    """The `Road` of a variable with the facts `f` under the switches `s`."""
    if f.categorical:
        return _decide_categorical(f)
    if f.out_dtype is not None:
        out_dtype = np.dtype(f.out_dtype)
    else:      # the Regridder's, or with half=True and no explicit out_dtype a half field's own type
        out_dtype = np.dtype(f.dtype) if s.half and not s.out_dtype_given and is_half(f.dtype) else s.out_dtype
    lines, after, refused = [], [], None
    source, why, dtype = PLAIN, None, f.dtype
    if f.held == GRIB:
        why = _why_grib_decodes(s, f, out_dtype)
        source = RAW_GRIB if why is None else DECODED
    cf, enc = f.cf, f.cf_out
    if f.direct:
        grib_out = source == RAW_GRIB and ((f.grib_out and not s.lazy) if f.levels else s.grib_out)
    else:
        if source == DECODED and s.packed:
            lines.append((INFO, f"packed variable {f.name} is decoded on the host ({why})"))
        grib_out = s.grib_out and source == RAW_GRIB and (not f.levels or s.grib_out_levels)
        if s.grib_out and not grib_out:
            lines.append((INFO, f"grib_out: {f.name} comes back as without it (%s)" % (
                "masked levels" if source == RAW_GRIB else "decoded on the host" if f.held == GRIB else "not a raw GRIB variable")))
        if cf and is_half(out_dtype):
            refused = (VARIABLE, f"packed=True regrids {f.name} raw: its result is float64 or packed, "
                                 "a half-precision out_dtype does not go with it")
        elif cf and ((f.levels and not s.packed_levels) or s.out_dtype != F64):
            # float32 results take no packed input, level groups only with packed_levels=True
            source, why, cf = DECODED, "masked levels" if f.levels else "out_dtype float32", False
            lines.append((INFO, f"packed variable {f.name} is decoded on the host ({why})"))
    if source == DECODED:
        dtype = np.dtype(np.float32)      # what a GribField decodes to; a CFDecode gives float32 or float64: no half either
    ship_half = is_half(dtype) and (s.half or dtype == BFLOAT16)
    if cf:
        source = RAW_CF
    elif source == PLAIN and ship_half and f.held not in (BS, SB):
        source = HALF
    elif source == PLAIN and f.held == HOST and dtype not in (np.dtype(np.float32), F64):
        source = PROMOTED

    device_result = f.held in (BS, SB) and not s.lazy
    if grib_out:
        result = GRIB_SIMPLE if f.levels else GRIB_CCSDS if s.grib_out_ccsds else GRIB_CPX if s.grib_out_cpx else GRIB_SIMPLE
    elif enc and (f.direct or not f.levels or s.packed_out_levels):
        result = CF_KERNEL
    elif enc and device_result:
        result = FLOAT64_DEVICE
        after.append((WARNING, f"packed_out: the device-resident result of {f.name} on masked-level weights stays float64"))
    elif enc:
        result = CF_HOST
        after.append((INFO, f"packed_out: {f.name} on masked-level weights is encoded on the host"))
    else:
        result = FLOAT

    sb_in = f.held == SB
    if refused is None:
        message = _layout_refusal(s, f, sb_in)
        refused = None if message is None else (LAYOUT, message)
    return Road(source, why, result, out_dtype, ship_half, sb_in, sb_in and s.keep_batch_fastest,
                f.grad_rule and not f.levels, refused, tuple(lines), tuple(after))
