// GRIB simple-packed fields regridded raw (smm_apply_grib): the kernel's arguments and its launcher, which is compiled
// in an object of its own (smm_grib.hip).  The kernel is kernel A (smm_kernels.hpp: SELL-64, one destination row per
// lane, BT batch rows register-blocked) with the X access replaced by the bit extraction and decode of smm_grib_codec.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/smmregrid_amd.h"
#include "smm_kernels.hpp"

struct GribArgs {
  const LevelDesc* descs;        // device, one element: the operator's SELL layout and epilogue vectors
  const uint32_t* x;             // device: the packed bytes as 32-bit words (4-byte aligned)
  const smm_grib_row_t* rows;    // device [n_j]: where batch row j starts in x and how it decodes
  double* y;                     // device: row j at y + j * ldy
  int64_t ldy, n_j, n_dblocks, n_jtiles, n_dst;
  uint64_t last_word;            // index of the last word of x: no load goes past it
  double area_min;
  int masked;
};

namespace smm_launch {
// div: some row of the call has ddiv != 1.0 (the instantiation with the f64 division); fill: the 1e20 fill is on
int launch_grib(const GribArgs& a, bool div, bool fill, hipStream_t s);
}
