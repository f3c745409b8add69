"""smmregrid_amd -- MI355X-native sparse regrid engine (drop-in for the
apply path of jhardenberg/smmregrid: Regridder(...).regrid(), CdoGenerate)."""
from .regrid import Regridder, regrid
from .cdogenerate import CdoGenerate, cdo_generate_weights
from .gridtype import GridType
from .gridmeta import CdoGrid, GridDetector, GridInspector
from .operator import SparseOperator, OperatorGroup
from .device import (CFDecode, CFEncode, DeviceArray, bfloat16, from_bfloat16, grib_aec_pack, grib_cpx_pack, grib_pack, grib_unpack,
                     grib_unpack_cpx, grib_unpack_cpx_mv, pinned_empty,
                     to_bfloat16, to_device)
from .xrlite import DataArray, Dataset
from .gradients import GradientRule
from .categorical import ModeRule
from .griblite import GRIB_AEC_DTYPE, GRIB_BITMAP_DTYPE, GRIB_CPX_DTYPE, GRIB_ENCODE_DTYPE, GRIB_NO_BITMAP, GRIB_ROW_DTYPE, GribEncode, GribField, aec_encode, cpx_encode

__version__ = '0.1.0'

__all__ = ["Regridder", "regrid", "CdoGenerate", "cdo_generate_weights", "GridType", "GridInspector", "GridDetector", "CdoGrid",
           "SparseOperator", "OperatorGroup", "CFDecode", "CFEncode", "DeviceArray", "to_device", "pinned_empty", "DataArray", "Dataset",
           "bfloat16", "to_bfloat16", "from_bfloat16", "GRIB_ROW_DTYPE", "GribField",
           "GRIB_BITMAP_DTYPE", "GRIB_NO_BITMAP", "GRIB_ENCODE_DTYPE", "GribEncode", "grib_pack",
           "GRIB_AEC_DTYPE", "grib_unpack", "grib_aec_pack", "aec_encode",
           "GRIB_CPX_DTYPE", "grib_unpack_cpx", "grib_unpack_cpx_mv", "grib_cpx_pack", "cpx_encode",
           "GradientRule", "ModeRule"]
