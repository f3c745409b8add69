// One variant of the kernel launch templates (the Makefile's INST list; all of them together: SMM_BUILT, smm_built.hpp).
// -DSMM_XT=... -DSMM_YT=...: one float (X, Y) pair, all four launchers.  With -DSMM_PACKED=1: the int16 / uint16 packed-X
// launchers that decode to SMM_XT instead.  With -DSMM_PACKED_Y=1: the launchers that store CF-packed int16 / uint16
// results (PackedY), for float X of type SMM_XT or, with -DSMM_PACKED=1 too, packed X of the same raw type decoded to
// SMM_XT.  With -DSMM_HALF=f16 / bf16: the half-precision rows of that kind (HalfX / HalfY) -- -DSMM_HALF_X=1: a half field
// to f64 and to its own type; else: f32 and f64 fields to a half result.  -DSMM_SKIPNA=1: the SMM_APPLY_SKIPNA variants of
// the same.
#include "smm_launch.hpp"

#ifndef SMM_SKIPNA
#define SMM_SKIPNA 0
#endif

namespace smm_launch {
#ifdef SMM_HALF
// Half-precision fields and results (smm_kernels.hpp): kernel A, kernel C and the grouped kernel C.  No tile kernel.
#define SMM_INST_HALF(XT, YT)                                                                            \
  template int launch_sell<XT, YT, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, bool, unsigned, hipStream_t); \
  template int launch_sb<XT, YT, SMM_SKIPNA != 0>(const SbArgs&, bool, unsigned, hipStream_t);           \
  template int launch_sb_group<XT, YT, SMM_SKIPNA != 0>(const SbGroupArgs&, bool, unsigned, hipStream_t);
#ifdef SMM_HALF_X
SMM_INST_HALF(HalfX<HalfKind::SMM_HALF>, double)
SMM_INST_HALF(HalfX<HalfKind::SMM_HALF>, HalfY<HalfKind::SMM_HALF>)
#else
SMM_INST_HALF(float, HalfY<HalfKind::SMM_HALF>)
SMM_INST_HALF(double, HalfY<HalfKind::SMM_HALF>)
#endif
#undef SMM_INST_HALF
#elif defined(SMM_PACKED_Y)
// CF-packed 16-bit results encoded in the stores (PackedY, smm_kernels.hpp): kernel A, kernel C of single operators
// and the grouped kernel C of level groups.  No tile kernel; packed X only with Y's own raw type.
#ifdef SMM_PACKED
#define SMM_PKY_X(Q) PackedX<Q, SMM_XT>
#else
#define SMM_PKY_X(Q) SMM_XT
#endif
#define SMM_INST_PACKED_Y(Q)                                                                                        \
  template int launch_sell<SMM_PKY_X(Q), PackedY<Q>, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, bool, unsigned,    \
                                                                      hipStream_t);                                 \
  template int launch_sb<SMM_PKY_X(Q), PackedY<Q>, SMM_SKIPNA != 0>(const SbArgs&, bool, unsigned, hipStream_t);    \
  template int launch_sb_group<SMM_PKY_X(Q), PackedY<Q>, SMM_SKIPNA != 0>(const SbGroupArgs&, bool, unsigned,       \
                                                                          hipStream_t);
SMM_INST_PACKED_Y(int16_t)
SMM_INST_PACKED_Y(uint16_t)
#undef SMM_INST_PACKED_Y
#undef SMM_PKY_X
#elif defined(SMM_PACKED)
// CF-packed 16-bit X decoded to SMM_XT in registers (PackedX, smm_kernels.hpp): kernel A, kernel C and the grouped
// kernel C of level groups, f64 results
#define SMM_INST_PACKED(Q)                                                                                          \
  template int launch_sell<PackedX<Q, SMM_XT>, double, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, bool, unsigned,  \
                                                                        hipStream_t);                               \
  template int launch_sb<PackedX<Q, SMM_XT>, double, SMM_SKIPNA != 0>(const SbArgs&, bool, unsigned, hipStream_t); \
  template int launch_sb_group<PackedX<Q, SMM_XT>, double, SMM_SKIPNA != 0>(const SbGroupArgs&, bool, unsigned,     \
                                                                            hipStream_t);
SMM_INST_PACKED(int16_t)
SMM_INST_PACKED(uint16_t)
#undef SMM_INST_PACKED
#else
template int launch_sell<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, bool, unsigned, hipStream_t);
template int launch_tile<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, int, int64_t, int64_t, int, bool,
                                                          unsigned, hipStream_t);
template int launch_sb<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const SbArgs&, bool, unsigned, hipStream_t);
template int launch_sb_group<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const SbGroupArgs&, bool, unsigned, hipStream_t);
#endif
}  // namespace smm_launch
