// One (X dtype, Y dtype, SKIPNA) triple of the kernel launch templates; built with -DSMM_XT=... -DSMM_YT=...
// and -DSMM_SKIPNA=1 for the SMM_APPLY_SKIPNA variants
#include "smm_launch.hpp"

#ifndef SMM_SKIPNA
#define SMM_SKIPNA 0
#endif

namespace smm_launch {
template int launch_sell<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, bool, unsigned, hipStream_t);
template int launch_tile<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const ApplyArgs&, int64_t, int, int64_t, int64_t, int, bool,
                                                          unsigned, hipStream_t);
template int launch_sb<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const SbArgs&, bool, unsigned, hipStream_t);
template int launch_sb_group<SMM_XT, SMM_YT, SMM_SKIPNA != 0>(const SbGroupArgs&, bool, unsigned, hipStream_t);
}  // namespace smm_launch
