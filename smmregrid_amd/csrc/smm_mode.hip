// Categorical fields regridded by largest area fraction (gfx950): smm_apply_mode and smm_mode_launch_info.  One kernel
// in two forms over the operator's SELL-64 tables, one destination row per lane, a slice per wave:
//   LDS form     the wave gathers its slice's values once into LDS as [slot][lane] -- a lane reads back only what it
//                wrote itself, 4-byte cells lane-contiguous, so there is no bank conflict and no barrier -- and the class
//                scan of mode_row (smm_mode.hpp) runs from there; the weights are read again from the val stream
//   global form  a slice with more slots than the LDS holds gathers from X again inside the scan: right for any row
//                length, slow, and rare (the longest rows of a HEALPix target's polar caps)
// The form is chosen per slice, so one launch runs both.  The rule is the text of include/smmregrid_amd.h ("categorical
// fields"); nothing is multiplied, the shares are plain float64 adds in link order.
#include "smm_mode.hpp"

#include <algorithm>
#include <limits>
#include <string>
#include <type_traits>

#include "smm_device.hpp"

#pragma clang fp contract(off)

namespace {

// LDS of one wave: 16 KiB, 64 slots of 4-byte cells (float; int16 / uint16 widened) or 32 of double.  A workgroup of four
// waves takes at most 64 KiB: two workgroups per CU.  The launch asks for min(capacity, the operator's longest row), so
// operators of short rows run at the occupancy the registers allow.
constexpr int kModeLdsBytesPerWave = 16 << 10;

template <typename XT>
struct ModeCell {
  using type = std::conditional_t<std::is_floating_point<XT>::value, XT, int32_t>;
};
template <typename XT>
constexpr int mode_capacity() {
  return kModeLdsBytesPerWave / (64 * (int)sizeof(typename ModeCell<XT>::type));
}

template <typename CT>
struct LdsLinks {
  const CT* cell;                        // this lane's column of the wave's LDS: slot k at cell[k * 64]
  const double* __restrict__ w;          // this lane's weights: slot k at w[k * 64]
  __device__ __forceinline__ CT value(int k) const { return cell[k * 64]; }
  __device__ __forceinline__ double weight(int k) const { return w[(int64_t)k * 64]; }
};
template <typename XT, typename CT>
struct GlobalLinks {
  const XT* __restrict__ row;            // the batch row of X
  const int32_t* __restrict__ c;         // this lane's columns: slot k at c[k * 64]
  const double* __restrict__ w;
  __device__ __forceinline__ CT value(int k) const { return (CT)row[c[(int64_t)k * 64]]; }
  __device__ __forceinline__ double weight(int k) const { return w[(int64_t)k * 64]; }
};

template <typename XT>
__global__ __launch_bounds__(kThreads) void smm_mode_kernel(ModeArgs a) {
  using CT = typename ModeCell<XT>::type;
  extern __shared__ __attribute__((aligned(16))) char mode_lds[];
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bid = blockIdx.x;
  const int64_t db = a.db0 + bid % a.n_dblocks;
  const int64_t b = bid / a.n_dblocks;
  const int64_t slice = db * kWavesPerBlock + wave;
  if (slice * 64 >= a.n_dst) return;     // no barrier below: a wave is on its own
  const int64_t d = slice * 64 + lane;   // rowlen covers whole slices: rows past n_dst have length 0

  const XT* __restrict__ xrow = (const XT*)a.x + b * a.ldx;
  const int64_t off = a.slice_off[slice];
  const int nslots = (int)((a.slice_off[slice + 1] - off) >> 6);
  const int len = a.rowlen[d];           // padded slots are never looked at: every walk stops at len
  const int32_t* __restrict__ cp = a.col + off + lane;
  const double* __restrict__ wp = a.val + off + lane;

  bool masked = false;
  double frac = 1.0;
  if (d < a.n_dst) {
    if (a.masked && a.imask) masked = a.imask[d] == 0;
    if (a.frac) frac = a.frac[d];
  }

  ModeResult r;
  CT winner = CT(0);
  if (nslots <= a.lds_slots) {           // wave-uniform
    CT* cell = (CT*)mode_lds + (size_t)wave * a.lds_slots * 64 + lane;
    for (int k = 0; k < nslots; ++k)
      if (k < len) cell[k * 64] = (CT)xrow[cp[(int64_t)k * 64]];
    const LdsLinks<CT> links{cell, wp};
    r = mode_row(len, links, a.miss, masked, frac, a.area_min);
    if (r.k >= 0) winner = links.value(r.k);
  } else {
    const GlobalLinks<XT, CT> links{xrow, cp, wp};
    r = mode_row(len, links, a.miss, masked, frac, a.area_min);
    if (r.k >= 0) winner = links.value(r.k);
  }
  if (d < a.n_dst) {
    XT out;
    if (r.k >= 0) {
      out = (XT)winner;
    } else {
      if constexpr (std::is_floating_point<XT>::value) out = (XT)__builtin_nan("");
      else out = (XT)a.fill_out;
    }
    ((XT*)a.y)[b * a.ldy + d] = out;
    if (a.share) a.share[b * a.ld_share + d] = r.share;
  }
}

int64_t mode_grid_limit() { return std::min<int64_t>(grid_limit(), 0x7fffffffLL); }

int mode_capacity_of(int x_dtype) {
  return x_dtype == SMM_F64 ? mode_capacity<double>() : mode_capacity<float>();
}
// slots per wave the launch asks LDS for
int mode_lds_slots(const smm_operator* op, int x_dtype) {
  return (int)std::min<int64_t>(mode_capacity_of(x_dtype), op->csr.max_row_nnz);
}
size_t mode_cell_bytes(int x_dtype) { return x_dtype == SMM_F64 ? 8 : 4; }
size_t mode_elem_bytes(int x_dtype) { return x_dtype == SMM_F64 ? 8 : (x_dtype == SMM_F32 ? 4 : 2); }

template <typename XT>
int launch_mode(ModeArgs a, int64_t n_batch, size_t lds_bytes, hipStream_t s) {
  // the grid is cut along the batch, and where one batch row alone exceeds the limit along the destination blocks too
  const int64_t limit = mode_grid_limit();
  const int64_t all_db = a.n_dblocks;
  const int64_t db_step = std::min(all_db, limit);
  const int64_t rows_max = std::max<int64_t>(1, limit / db_step);
  const char* x = (const char*)a.x;
  char* y = (char*)a.y;
  double* share = a.share;
  for (int64_t r0 = 0; r0 < n_batch; r0 += rows_max) {
    const int64_t nr = std::min(rows_max, n_batch - r0);
    a.x = x + (size_t)(r0 * a.ldx) * sizeof(XT);
    a.y = y + (size_t)(r0 * a.ldy) * sizeof(XT);
    a.share = share ? share + r0 * a.ld_share : nullptr;
    for (int64_t db0 = 0; db0 < all_db; db0 += db_step) {
      a.db0 = db0;
      a.n_dblocks = std::min(db_step, all_db - db0);
      hipLaunchKernelGGL(smm_mode_kernel<XT>, dim3((unsigned)(nr * a.n_dblocks)), dim3(kThreads), lds_bytes, s, a);
      SMM_HIP(hipGetLastError());
    }
  }
  return SMM_OK;
}

// what the raw type of an integer field can hold
bool mode_fits(int x_dtype, int32_t v) {
  return x_dtype == SMM_I16 ? (v >= -32768 && v <= 32767) : (v >= 0 && v <= 65535);
}

}  // namespace

extern "C" {

int smm_mode_launch_info(smm_operator_t op, int x_dtype, int* capacity, int* lds_slots, int64_t* lds_bytes,
                         int64_t* n_lds_slices, int64_t* n_global_slices) {
  return guarded([&]() -> int {
    if (x_dtype != SMM_F32 && x_dtype != SMM_F64 && x_dtype != SMM_I16 && x_dtype != SMM_U16)
      return fail(SMM_ERR_UNSUPPORTED, "the categorical apply is built for SMM_F32, SMM_F64, SMM_I16 and SMM_U16 fields");
    if (capacity) *capacity = mode_capacity_of(x_dtype);
    if (!op) {                           // the capacity depends on the type alone
      if (lds_slots || lds_bytes || n_lds_slices || n_global_slices) return fail(SMM_ERR_INVALID, "null operator");
      return SMM_OK;
    }
    const int slots = mode_lds_slots(op, x_dtype);
    int64_t n_lds = 0, n_glob = 0;
    const auto& so = op->sell_shape.slice_off;
    for (size_t i = 0; i + 1 < so.size(); ++i) ((so[i + 1] - so[i]) >> 6) <= slots ? ++n_lds : ++n_glob;
    if (lds_slots) *lds_slots = slots;
    if (lds_bytes) *lds_bytes = (int64_t)kWavesPerBlock * slots * 64 * (int64_t)mode_cell_bytes(x_dtype);
    if (n_lds_slices) *n_lds_slices = n_lds;
    if (n_global_slices) *n_global_slices = n_glob;
    return SMM_OK;
  });
}

int smm_apply_mode(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int64_t ldy, double* share,
                   int64_t ld_share, int64_t n_batch, double remap_area_min, unsigned flags, const smm_mode_rule_t* rule,
                   void* stream) {
  return guarded([&]() -> int {
    // what is not built, before the handles are looked at
    if (int rc = check_flags(flags)) return rc;
    if (flags & SMM_APPLY_SKIPNA)
      return fail(SMM_ERR_UNSUPPORTED, "SMM_APPLY_SKIPNA is not built for the categorical apply: a missing value takes part in no class as it is");
    if (flags & SMM_APPLY_NO_FILL)
      return fail(SMM_ERR_UNSUPPORTED, "SMM_APPLY_NO_FILL does not go with the categorical apply: it has no 1e20 fill to leave out");
    if (flags & SMM_APPLY_KERNEL_TILE)
      return fail(SMM_ERR_UNSUPPORTED, "the LDS tile kernel is not built for the categorical apply: it runs on the SELL tables");
    if (flags & (SMM_APPLY_SB_PACKED | SMM_APPLY_SB_Y_SB | SMM_APPLY_HOST_NO_PACK))
      return fail(SMM_ERR_UNSUPPORTED, "the batch-fastest and host-pack flags do not go with the categorical apply: it takes the native (B, S) layout on the device");
    if (x_dtype == SMM_F16 || x_dtype == SMM_BF16)
      return fail(SMM_ERR_UNSUPPORTED, "the categorical apply is not built for half-precision fields (SMM_F16 / SMM_BF16)");
    const bool is_float = x_dtype == SMM_F32 || x_dtype == SMM_F64;
    const bool is_int = x_dtype == SMM_I16 || x_dtype == SMM_U16;
    if (!is_float && !is_int)
      return fail(SMM_ERR_UNSUPPORTED, "field dtype must be SMM_F32, SMM_F64, SMM_I16 or SMM_U16");
    // the rule
    if (is_float && rule) return fail(SMM_ERR_INVALID, "a float field takes no smm_mode_rule_t: its missing value is whatever is not finite");
    if (is_int && !rule) return fail(SMM_ERR_INVALID, "an integer field needs a smm_mode_rule_t (its fill values and fill_out)");
    if (rule) {
      if (rule->n_fill < 0 || rule->n_fill > 2)
        return fail(SMM_ERR_INVALID, "smm_mode_rule_t.n_fill=" + std::to_string(rule->n_fill) + " outside 0..2");
      for (int i = 0; i < rule->n_fill; ++i)
        if (!mode_fits(x_dtype, rule->fill[i]))
          return fail(SMM_ERR_INVALID, "smm_mode_rule_t.fill[" + std::to_string(i) + "]=" + std::to_string(rule->fill[i]) +
                                           " is no value of the field's raw type");
      if (!mode_fits(x_dtype, rule->fill_out))
        return fail(SMM_ERR_INVALID, "smm_mode_rule_t.fill_out=" + std::to_string(rule->fill_out) + " is no value of the field's raw type");
      if (rule->reserved != 0) return fail(SMM_ERR_INVALID, "smm_mode_rule_t.reserved must be 0");
    }
    if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
    const size_t esz = mode_elem_bytes(x_dtype);
    if ((uintptr_t)x % esz || (uintptr_t)y % esz || (uintptr_t)share % 8)
      return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    if (!op) return fail(SMM_ERR_INVALID, "null operator");
    const int64_t S = op->csr.n_src, D = op->csr.n_dst;
    if (n_batch > 0 && (ldx < S || ldy < D)) return fail(SMM_ERR_INVALID, "ldx/ldy smaller than the grid size");
    if (n_batch > 0 && share && ld_share < D) return fail(SMM_ERR_INVALID, "ld_share smaller than the target grid");
    if (int rc = check_area_min(remap_area_min)) return rc;
    if (int rc = check_epilogue(op, flags & SMM_APPLY_MASKED, remap_area_min, "the operator")) return rc;
    if (n_batch == 0 || D == 0) return SMM_OK;
    if (!x || !y) return fail(SMM_ERR_INVALID, "null field pointer");
    DeviceGuard guard(op->device);
    if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");

    ModeArgs a{};
    a.slice_off = op->d_slice_off.get();
    a.col = op->d_col.get();
    a.val = op->d_val.get();
    a.rowlen = op->d_rowlen.get();
    a.imask = op->d_imask.get();
    a.frac = op->d_frac.get();
    a.x = x;
    a.y = y;
    a.share = share;
    a.ldx = ldx;
    a.ldy = ldy;
    a.ld_share = ld_share;
    a.n_dst = D;
    a.n_dblocks = ((D + 63) / 64 + kWavesPerBlock - 1) / kWavesPerBlock;
    a.area_min = remap_area_min;
    a.masked = (flags & SMM_APPLY_MASKED) ? 1 : 0;
    if (rule) {
      a.miss.n_fill = rule->n_fill;
      a.miss.fill[0] = rule->fill[0];
      a.miss.fill[1] = rule->fill[1];
      a.fill_out = rule->fill_out;
    }
    a.lds_slots = mode_lds_slots(op, x_dtype);
    const size_t lds_bytes = (size_t)kWavesPerBlock * (size_t)a.lds_slots * 64 * mode_cell_bytes(x_dtype);
    hipStream_t s = (hipStream_t)stream;
    switch (x_dtype) {
      case SMM_F64: return launch_mode<double>(a, n_batch, lds_bytes, s);
      case SMM_F32: return launch_mode<float>(a, n_batch, lds_bytes, s);
      case SMM_I16: return launch_mode<int16_t>(a, n_batch, lds_bytes, s);
      default: return launch_mode<uint16_t>(a, n_batch, lds_bytes, s);
    }
  });
}

}  // extern "C"
