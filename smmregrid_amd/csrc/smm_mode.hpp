// The categorical apply (smm_apply_mode; smm_mode.hip): the row rule of "largest area fraction" regridding, written once
// for both forms of the kernel and for the CPU harness (tests/cpp/mode_harness.cpp), and the kernel's argument struct.
// Not part of the ABI.  The rule is the text of include/smmregrid_amd.h ("categorical fields"); smmregrid_amd.categorical.
// ModeRule states it in numpy.  Plain C++: nothing here needs the HIP headers.
#pragma once

#include <cstdint>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define SMM_MODE_HD __host__ __device__ inline __attribute__((always_inline))
#else
#define SMM_MODE_HD inline
#endif

// Which values are missing: a float that is not finite; an integer equal to one of the first n_fill fills.
struct ModeMissing {
  int32_t n_fill = 0;
  int32_t fill[2] = {0, 0};
};

SMM_MODE_HD bool mode_missing(float v, const ModeMissing&) { return !(__builtin_fabsf(v) < __builtin_inff()); }
SMM_MODE_HD bool mode_missing(double v, const ModeMissing&) { return !(__builtin_fabs(v) < __builtin_inf()); }
SMM_MODE_HD bool mode_missing(int32_t v, const ModeMissing& m) {
  return (m.n_fill > 0 && v == m.fill[0]) || (m.n_fill > 1 && v == m.fill[1]);
}

// What a row gives: the slot of the winner's first link (-1: the row is dead) and the winner's share (+0.0 when dead).
struct ModeResult {
  int k;
  double share;
};

// One destination row of one batch row.  `links` gives the row's `len` links in ascending source order:
//   links.value(k)   the gathered x[b, col_k] -- float, double, or an int16 / uint16 widened to int32
//   links.weight(k)  w_k, column 0
// masked: the row is masked out (SMM_APPLY_MASKED and dst_imask[d] == 0); frac: dst_frac[d], 1.0 without one.
//
// tot and val first, in link order from +0.0.  Then every link that is not missing and whose value did not occur at an
// earlier link is a candidate: its class's share is summed from +0.0 over the links from there on that compare equal,
// one add per link -- the bits of the plain apply on the indicator field x == c, whose other products are +-0.0 and
// leave a sum that starts at +0.0 alone.  The best is replaced on a strictly greater share only, so bit-equal shares go
// to the class whose first link comes first, and a share that is not > 0.0 never wins.  The work is O(len * classes).
template <typename Links>
SMM_MODE_HD ModeResult mode_row(int len, const Links& links, const ModeMissing& miss, bool masked, double frac,
                                double area_min) {
  double tot = 0.0, val = 0.0;
  for (int k = 0; k < len; ++k) {
    const double w = links.weight(k);
    tot = tot + w;
    if (!mode_missing(links.value(k), miss)) val = val + w;
  }
  ModeResult best{-1, 0.0};
  for (int k = 0; k < len; ++k) {
    const auto v = links.value(k);
    if (mode_missing(v, miss)) continue;
    bool seen = false;
    for (int j = 0; j < k && !seen; ++j) seen = links.value(j) == v;
    if (seen) continue;
    double share = links.weight(k);   // +0.0 + w_k
    share = 0.0 + share;
    for (int j = k + 1; j < len; ++j)
      if (links.value(j) == v) share = share + links.weight(j);
    if (share > best.share) {
      best.k = k;
      best.share = share;
    }
  }
  bool dead = masked || best.k < 0;
  if (area_min > 0.0) dead = dead || (frac * (val / tot) < area_min);
  if (dead) {
    best.k = -1;
    best.share = 0.0;
  }
  return best;
}

// Arguments of smm_mode_kernel.  A workgroup owns kWavesPerBlock slices of one batch row: block id = batch row (of this
// launch) * n_dblocks + destination block (of this launch); db0 is the first destination block of the launch.
struct ModeArgs {
  const int64_t* slice_off;
  const int32_t* col;
  const double* val;      // column 0, SELL slots
  const int32_t* rowlen;
  const uint8_t* imask;   // [n_dst] or null
  const double* frac;     // [n_dst] or null
  const void* x;          // row b at x + b * ldx elements
  void* y;                // row b at y + b * ldy elements, the field's own type
  double* share;          // row b at share + b * ld_share, or null
  int64_t ldx, ldy, ld_share;
  int64_t n_dst, n_dblocks, db0;
  double area_min;
  ModeMissing miss;
  int32_t fill_out;
  int masked;
  int lds_slots;          // slots of a slice the workgroup's LDS holds per wave: slices up to that long take the LDS form
};
