// Source gradients and the K-column apply (smm_grad_plan_*, smm_gradients, smm_apply_cols; smm_grad.hip): the handle of
// a source grid's gradient tables and the argument structs of the two kernels.  Not part of the ABI.  The rule itself is
// the text of include/smmregrid_amd.h; smmregrid_amd.gradients.GradientRule states it in numpy and makes the tables.
#pragma once

#include <cstdint>

#include "smm_devmem.hpp"

constexpr int kGradMaxPlanes = 3;

struct smm_grad_plan {
  int device = -1;
  int64_t nx = 0, ny = 0;
  int periodic = 0;
  int n_planes = 0;
  int kind[kGradMaxPlanes] = {0, 0, 0};   // SMM_GRAD_I / _J / _IJ, in the order of the weight columns 1..
  smm::DeviceBuf<double> d_si, d_sj, d_ci;   // [3 * nx], [3 * ny], [ny]
};

// Arguments of the stencil kernel.  A workgroup owns kGradTileX consecutive columns of kGradBandRows consecutive rows of
// one batch row: block id = (batch row * n_bands + band) * n_xtiles + x tile.
struct GradArgs {
  const void* x;   // row b at x + b * ldx elements
  double* g;       // plane p of row b at g + b * ld_row + p * ld_plane
  const double* si;
  const double* sj;
  const double* ci;
  int64_t ldx, ld_plane, ld_row;
  int nx, ny, periodic, n_planes;
  int kind[kGradMaxPlanes];
  int n_xtiles, n_bands;
};

// Arguments of the K-column gather: smm_apply_sell_kernel's walk over one operator, with the K - 1 weight planes beside
// val and the K - 1 gradient planes beside x.
struct ColsArgs {
  const int64_t* slice_off;
  const int32_t* col;
  const double* val;      // column 0, SELL slots
  const double* xval;     // columns 1.., plane k - 1 at xval + (k - 1) * n_slots
  const int32_t* rowlen;
  const uint8_t* imask;   // [n_dst] or null
  const double* frac;     // [n_dst] or null
  const void* x;          // row b at x + b * ldx elements
  const double* g;        // plane k - 1 of row b at g + b * g_ld_row + (k - 1) * g_ld_plane
  double* y;              // row b at y + b * ldy
  int64_t n_slots, ldx, g_ld_row, g_ld_plane, ldy;
  int64_t n_j, n_dst, n_dblocks, n_jtiles;
  double area_min;
  int masked;
};
