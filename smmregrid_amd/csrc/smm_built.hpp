// The built (X type, Y type) combinations of the launch templates, written down once: the extern template
// declarations, the run-time dispatch (visit_built) and the dtype check of the apply paths (is_built) all come
// from SMM_BUILT below.  Every row is built plain and with SMM_APPLY_SKIPNA; smm_launch_inst.hip instantiates them.
#pragma once

#include "smm_launch.hpp"

namespace smm_launch {

using XI16F = PackedX<int16_t, float>;
using XI16D = PackedX<int16_t, double>;
using XU16F = PackedX<uint16_t, float>;
using XU16D = PackedX<uint16_t, double>;
using YI16 = PackedY<int16_t>;
using YU16 = PackedY<uint16_t>;
using XF16 = HalfX<HalfKind::f16>;
using XBF16 = HalfX<HalfKind::bf16>;
using YF16 = HalfY<HalfKind::f16>;
using YBF16 = HalfY<HalfKind::bf16>;
constexpr int kAnyDecode = -1;   // float X: the decode dtype plays no part

// M(x_dtype, decode_dtype, XT, y_dtype, YT, TILE): TILE = 1 where launch_tile is built too (float pairs only)
#define SMM_BUILT(M)                              \
  M(SMM_F64, kAnyDecode, double, SMM_F64, double, 1) \
  M(SMM_F64, kAnyDecode, double, SMM_F32, float, 1)  \
  M(SMM_F32, kAnyDecode, float, SMM_F64, double, 1)  \
  M(SMM_F32, kAnyDecode, float, SMM_F32, float, 1)   \
  M(SMM_I16, SMM_F32, XI16F, SMM_F64, double, 0)     \
  M(SMM_I16, SMM_F64, XI16D, SMM_F64, double, 0)     \
  M(SMM_U16, SMM_F32, XU16F, SMM_F64, double, 0)     \
  M(SMM_U16, SMM_F64, XU16D, SMM_F64, double, 0)     \
  M(SMM_F32, kAnyDecode, float, SMM_I16, YI16, 0)    \
  M(SMM_F64, kAnyDecode, double, SMM_I16, YI16, 0)   \
  M(SMM_I16, SMM_F32, XI16F, SMM_I16, YI16, 0)       \
  M(SMM_I16, SMM_F64, XI16D, SMM_I16, YI16, 0)       \
  M(SMM_F32, kAnyDecode, float, SMM_U16, YU16, 0)    \
  M(SMM_F64, kAnyDecode, double, SMM_U16, YU16, 0)   \
  M(SMM_U16, SMM_F32, XU16F, SMM_U16, YU16, 0)       \
  M(SMM_U16, SMM_F64, XU16D, SMM_U16, YU16, 0)       \
  M(SMM_F16, kAnyDecode, XF16, SMM_F64, double, 0)   \
  M(SMM_F16, kAnyDecode, XF16, SMM_F16, YF16, 0)     \
  M(SMM_BF16, kAnyDecode, XBF16, SMM_F64, double, 0) \
  M(SMM_BF16, kAnyDecode, XBF16, SMM_BF16, YBF16, 0) \
  M(SMM_F32, kAnyDecode, float, SMM_F16, YF16, 0)    \
  M(SMM_F64, kAnyDecode, double, SMM_F16, YF16, 0)   \
  M(SMM_F32, kAnyDecode, float, SMM_BF16, YBF16, 0)  \
  M(SMM_F64, kAnyDecode, double, SMM_BF16, YBF16, 0)

#define SMM_EXTERN_TILE_0(XT, YT, NA)
#define SMM_EXTERN_TILE_1(XT, YT, NA)                                                                       \
  extern template int launch_tile<XT, YT, NA>(const ApplyArgs&, int64_t, int, int64_t, int64_t, int, bool, \
                                              unsigned, hipStream_t);
#define SMM_EXTERN_NA(XT, YT, TILE, NA)                                                                \
  extern template int launch_sell<XT, YT, NA>(const ApplyArgs&, int64_t, bool, unsigned, hipStream_t); \
  extern template int launch_sb<XT, YT, NA>(const SbArgs&, bool, unsigned, hipStream_t);              \
  extern template int launch_sb_group<XT, YT, NA>(const SbGroupArgs&, bool, unsigned, hipStream_t);   \
  SMM_EXTERN_TILE_##TILE(XT, YT, NA)
#define SMM_EXTERN(XD, DD, XT, YD, YT, TILE) SMM_EXTERN_NA(XT, YT, TILE, false) SMM_EXTERN_NA(XT, YT, TILE, true)
SMM_BUILT(SMM_EXTERN)
#undef SMM_EXTERN
#undef SMM_EXTERN_NA
#undef SMM_EXTERN_TILE_1
#undef SMM_EXTERN_TILE_0

// One built combination as a type tag: what visit_built hands to its callable
template <typename X, typename Y, bool NA, bool TILE>
struct Built {
  using XT = X;
  using YT = Y;
  static constexpr bool skipna = NA, tile = TILE;   // tile: launch_tile exists for <XT, YT, skipna>
};

constexpr bool built_row(int x_dtype, int y_dtype, int decode_dtype, int xd, int dd, int yd) {
  return x_dtype == xd && y_dtype == yd && (dd == kAnyDecode || decode_dtype == dd);
}

// Whether the run-time dtypes name a row of SMM_BUILT (decode_dtype counts for packed X only)
constexpr bool is_built(int x_dtype, int y_dtype, int decode_dtype) {
#define SMM_ROW(XD, DD, XT, YD, YT, TILE) \
  if (built_row(x_dtype, y_dtype, decode_dtype, XD, DD, YD)) return true;
  SMM_BUILT(SMM_ROW)
#undef SMM_ROW
  return false;
}

// fn(Built<XT, YT, SKIPNA, TILE>()) for the row of SMM_BUILT the run-time dtypes name; SMM_ERR_UNSUPPORTED for any other
template <typename F>
int visit_built(int x_dtype, int y_dtype, int decode_dtype, bool skipna, F&& fn) {
#define SMM_ROW(XD, DD, XT, YD, YT, TILE)                      \
  if (built_row(x_dtype, y_dtype, decode_dtype, XD, DD, YD))   \
    return skipna ? fn(Built<XT, YT, true, TILE != 0>()) : fn(Built<XT, YT, false, TILE != 0>());
  SMM_BUILT(SMM_ROW)
#undef SMM_ROW
  return smm::fail_msg(SMM_ERR_UNSUPPORTED, "this field / result / decode type combination is not built");
}

}  // namespace smm_launch
