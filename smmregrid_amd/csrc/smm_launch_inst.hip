// One (X dtype, Y dtype, SKIPNA) triple of the kernel launch templates; built with -DSMM_XT=... -DSMM_YT=...
// and -DSMM_SKIPNA=1 for the SMM_APPLY_SKIPNA variants.  With -DSMM_PACKED=1: the int16 / uint16 packed-X launchers
// that decode to SMM_XT instead
#include "smm_launch.hpp"

#ifndef SMM_SKIPNA
#define SMM_SKIPNA 0
#endif

namespace smm_launch {
#ifdef SMM_PACKED
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
