// smm_grib_pack's kernels and launcher (gfx950): float64 results into GRIB simple packing before they leave the device.
// A field's reference value and binary scale follow from its own minimum and maximum, so nothing of this can sit in the
// stores of the apply kernels: a range pass that also writes the bitmap, a rule pass, the rank tables of the bitmaps
// (smm_grib.hip's build, on the bytes just written), and a pack pass -- one thread per 32-bit word of a row's stream.
// The rule is the text in smm_grib_codec.hpp; plain vector stores, no atomics, 256 threads everywhere but the rule pass.
#include "smm_grib.hpp"

#include <algorithm>
#include <string>

#include "smm_grib_codec.hpp"
#include "smm_launch.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int kPackThreads = 256, kPackWaves = kPackThreads / 64;
constexpr uint32_t kSegCells = 32u * (uint32_t)smm_grib::kGribSegBlocks;

// a launch covers rows [j0, j0 + grid rows): the args carry the whole call, the kernels add j0
struct PackPart {
  int64_t j0;
};

// ---- 1: range + bitmap.  One workgroup per (row, segment); a wave takes 64 consecutive cells per step, its ballot is
// two bitmap words (cell 32k is the top bit of word k, the word big-endian in memory), lane 0 stores them.  Cells at or
// beyond n_dst are not present: the pad bits are zero.  Every word k < n_blocks of the row's bitmap part is written.
__global__ __launch_bounds__(kPackThreads) void smm_grib_range_kernel(GribPackArgs a, PackPart part) {
  __shared__ double smin[kPackWaves], smax[kPackWaves];
  __shared__ uint32_t scnt[kPackWaves];
  const int64_t j = part.j0 + blockIdx.x / a.n_segs;
  const uint32_t seg = blockIdx.x % a.n_segs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const GribPackRow* __restrict__ rows = a.rows;
  const GribPackRow r = rows[j];
  const double* __restrict__ y = a.y + j * a.ldy;
  uint32_t* __restrict__ words = a.out + (r.slot_off >> 2);

  double mn = __builtin_inf(), mx = -__builtin_inf();
  uint32_t cnt = 0;
  const uint32_t c0 = seg * kSegCells;   // < n_dst < 2^31
  for (uint32_t it = 0; it < kSegCells / kPackThreads; ++it) {
    const uint32_t base = c0 + it * kPackThreads;   // <= 2^31 + 32768: 32 bits hold it
    if (base >= a.n_dst) break;                     // block-uniform
    const uint32_t c = base + threadIdx.x;
    bool p = false;
    double t = 0.0;
    if (c < a.n_dst) p = smm_grib::grib_encode_t(y[c], r.ddiv, &t);
    if (p) {
      mn = t < mn ? t : mn;
      mx = t > mx ? t : mx;
      ++cnt;
    }
    const uint64_t bal = __ballot(p);
    if (lane == 0) {
      const uint32_t k = (base + (uint32_t)wave * 64u) >> 5;
      if (k < a.n_blocks) words[k] = __builtin_bswap32(__builtin_bitreverse32((uint32_t)bal));
      if (k + 1 < a.n_blocks) words[k + 1] = __builtin_bswap32(__builtin_bitreverse32((uint32_t)(bal >> 32)));
    }
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane == 0) smin[wave] = mn, smax[wave] = mx, scnt[wave] = cnt;
  __syncthreads();
  if (threadIdx.x == 0) {
#pragma unroll
    for (int w = 1; w < kPackWaves; ++w) {
      mn = smin[w] < mn ? smin[w] : mn;
      mx = smax[w] > mx ? smax[w] : mx;
      cnt += scnt[w];
    }
    const int64_t at = j * a.n_segs + seg;
    a.part_min[at] = mn;
    a.part_max[at] = mx;
    a.part_cnt[at] = cnt;
  }
}

// ---- 2: the rule.  One wave per row: the lanes stride over the row's segments, a shuffle reduction, lane 0 applies
// grib_encode_rule and writes the rule for the pack and the records the caller gets.  min, max and an integer sum: the
// result does not depend on the order.
__global__ __launch_bounds__(64) void smm_grib_rule_kernel(GribPackArgs a, PackPart part) {
  const int64_t j = part.j0 + blockIdx.x;
  const int lane = threadIdx.x;
  double mn = __builtin_inf(), mx = -__builtin_inf();
  uint32_t cnt = 0;
  for (uint32_t s = lane; s < a.n_segs; s += 64) {
    const int64_t at = j * a.n_segs + s;
    const double smn = a.part_min[at], smx = a.part_max[at];
    mn = smn < mn ? smn : mn;
    mx = smx > mx ? smx : mx;
    cnt += a.part_cnt[at];
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const double omn = __shfl_xor(mn, o, 64), omx = __shfl_xor(mx, o, 64);
    mn = omn < mn ? omn : mn;
    mx = omx > mx ? omx : mx;
    cnt += __shfl_xor(cnt, o, 64);
  }
  if (lane != 0) return;
  const GribPackRow r = a.rows[j];
  const smm_grib::GribPackRule rule = smm_grib::grib_encode_rule(mn, mx, cnt, r.nbits);
  a.rules[j] = rule;
  smm_grib_row_t rec;
  rec.byte_off = r.pub_off + smm_grib::pack_bitmap_bytes(a.n_dst);
  rec.ref = rule.ref;
  rec.bscale = __builtin_ldexp(1.0, rule.E);
  rec.ddiv = r.ddiv;
  rec.nbits = rule.width;
  rec.reserved = 0;
  a.rec_rows[j] = rec;
  smm_grib_bitmap_t bm;
  bm.bitmap_off = cnt == a.n_dst ? SMM_GRIB_NO_BITMAP : r.pub_off;
  bm.n_values = cnt;
  a.rec_bm[j] = bm;
}

// ---- 3: pack.  One thread per 32-bit word of a row's stream part (the grid covers max_words per row; a narrower row's
// surplus threads leave).  The word is smm_grib_codec.hpp's grib_pack_word -- the values that overlap it, their q
// recomputed from Y and the row's rule; a row with missing cells finds the cell of its first value by binary search over
// the rank table and walks the set bits from there, a row with every cell present takes cell = value on a block-uniform
// branch -- stored big-endian; words the stream does not reach are stored as zero.
__global__ __launch_bounds__(kPackThreads) void smm_grib_pack_kernel(GribPackArgs a, PackPart part, uint32_t blocks_per_row) {
  const int64_t j = part.j0 + blockIdx.x / blocks_per_row;
  const uint32_t w = (blockIdx.x % blocks_per_row) * kPackThreads + threadIdx.x;
  const GribPackRow* __restrict__ rows = a.rows;
  const GribPackRow r = rows[j];
  const uint32_t n_words = (uint32_t)(smm_grib::align4(smm_grib::row_bytes(a.n_dst, r.nbits)) >> 2);
  if (w >= n_words) return;
  const smm_grib::GribPackRule* __restrict__ rules = a.rules;
  const smm_grib::GribPackRule rule = rules[j];
  const double* __restrict__ y = a.y + j * a.ldy;
  uint32_t* __restrict__ out = a.out + ((r.slot_off + smm_grib::pack_bitmap_bytes(a.n_dst)) >> 2);

  const uint32_t word = smm_grib::grib_pack_word(y, r.ddiv, rule, a.n_dst, a.table + j * a.n_blocks, a.n_blocks, w);
  out[w] = __builtin_bswap32(word);
}

}  // namespace

namespace smm_launch {

int launch_grib_pack(const GribPackArgs& a, const GribBuildArgs& build, int64_t limit, hipStream_t s) {
  if (a.n_j <= 0 || a.n_dst == 0) return SMM_OK;
  limit = std::min<int64_t>(std::max<int64_t>(limit, 1), 0x7fffffffLL);
  const uint32_t blocks_per_row = (a.max_words + kPackThreads - 1) / kPackThreads;
  // rows per launch so that no grid passes the limit: the pack has the most workgroups per row, or the range pass
  const int64_t per_row = std::max<int64_t>(std::max<int64_t>(blocks_per_row, a.n_segs), 1);
  if (per_row > limit)
    return smm::fail_msg(SMM_ERR_INVALID, "one row alone needs a launch grid beyond " + std::to_string(limit) + " workgroups");
  const int64_t rows_per = limit / per_row;
  for (int64_t j0 = 0; j0 < a.n_j; j0 += rows_per) {
    const int64_t nr = std::min(rows_per, a.n_j - j0);
    hipLaunchKernelGGL(smm_grib_range_kernel, dim3((unsigned)(nr * a.n_segs)), dim3(kPackThreads), 0, s, a, PackPart{j0});
    SMM_LAUNCH_HIP(hipGetLastError());
  }
  for (int64_t j0 = 0; j0 < a.n_j; j0 += limit) {
    const int64_t nr = std::min(limit, a.n_j - j0);
    hipLaunchKernelGGL(smm_grib_rule_kernel, dim3((unsigned)nr), dim3(64), 0, s, a, PackPart{j0});
    SMM_LAUNCH_HIP(hipGetLastError());
  }
  for (int64_t j0 = 0; j0 < a.n_j; j0 += rows_per) {
    GribBuildArgs b = build;
    b.bm = build.bm + j0;
    b.n_j = std::min(rows_per, a.n_j - j0);
    if (int rc = launch_grib_build(b, s)) return rc;
  }
  for (int64_t j0 = 0; j0 < a.n_j; j0 += rows_per) {
    const int64_t nr = std::min(rows_per, a.n_j - j0);
    hipLaunchKernelGGL(smm_grib_pack_kernel, dim3((unsigned)(nr * blocks_per_row)), dim3(kPackThreads), 0, s, a, PackPart{j0},
                       blocks_per_row);
    SMM_LAUNCH_HIP(hipGetLastError());
  }
  return SMM_OK;
}

}  // namespace smm_launch
