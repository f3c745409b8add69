// smm_apply_grib's kernel and launcher (gfx950): kernel A with the gather replaced -- per link two unconditional
// 32-bit loads from the packed bit stream, a byte swap, a 64-bit shift and the row's decode rule.
#include "smm_grib.hpp"

#include <algorithm>
#include <string>
#include <type_traits>

#include "smm_grib_codec.hpp"
#include "smm_launch.hpp"

#pragma clang fp contract(off)

namespace {

// BT batch rows per thread as in smm_apply_sell_kernel.  What a batch row needs -- its first word, the bit offset of
// its first value inside it, its width and rule -- is read once per block through a block-uniform index of the
// const __restrict__ row table: scalar loads, scalar registers.  DIV: grib_decode.
template <int BT, bool DIV>
__global__ __launch_bounds__(kThreads) void smm_apply_grib_kernel(GribArgs a, bool fill) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bid = blockIdx.x;
  const int64_t db = bid % a.n_dblocks;
  const int64_t jt = bid / a.n_dblocks;
  const LevelDesc L = a.descs[0];

  const int64_t slice = db * kWavesPerBlock + wave;
  const int64_t d = slice * 64 + lane;
  if (slice * 64 >= a.n_dst) return;

  const int64_t j0 = jt * BT;
  const smm_grib_row_t* __restrict__ rows = a.rows;
  const uint32_t* __restrict__ xw[BT];
  double* __restrict__ yr[BT];
  uint32_t bit0[BT], lastw[BT];
  int nbits[BT];
  double ref[BT], bscale[BT], ddiv[BT];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    int64_t j = j0 + t;
    if (j > a.n_j - 1) j = a.n_j - 1;
    const smm_grib_row_t r = rows[j];
    // a 0-bit row may start at the very end of the buffer: its words are clamped like every other load
    const uint64_t w = std::min<uint64_t>(r.byte_off >> 2, a.last_word);
    xw[t] = a.x + w;
    lastw[t] = (uint32_t)std::min<uint64_t>(a.last_word - w, 0xfffffffeull);
    bit0[t] = 8u * (uint32_t)(r.byte_off & 3);
    nbits[t] = r.nbits;
    ref[t] = r.ref;
    bscale[t] = r.bscale;
    ddiv[t] = r.ddiv;
    yr[t] = a.y + j * a.ldy;
  }

  const int64_t off = L.slice_off[slice];
  const int nslots = (int)((L.slice_off[slice + 1] - off) >> 6);
  const int len = L.rowlen[d];
  const int32_t* __restrict__ cp = L.col + off + lane;
  const double* __restrict__ vp = L.val + off + lane;

  RowSum<float, false> acc[BT];
  // padded slots: a valid column and weight +0.0, bitwise no-ops on a finite value (smm_apply_sell_kernel)
#pragma unroll 2
  for (int k = 0; k < nslots; ++k) {
    const uint32_t c = (uint32_t)cp[(int64_t)k * 64];
    const double w = vp[(int64_t)k * 64];
    double xv[BT];
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      const uint64_t p = (uint64_t)bit0[t] + (uint64_t)c * (uint32_t)nbits[t];
      const uint32_t q = smm_grib::grib_extract(xw[t], p, nbits[t], lastw[t]);
      const float v = smm_grib::grib_decode<DIV>(q, ref[t], bscale[t], ddiv[t]);
      xv[t] = (double)((fill && !__builtin_isfinite(v)) ? (float)1e20 : v);
    }
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[t].add(w, xv[t]);
  }
  if (len == 0) {
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[t].clear();
  }

  if (d < a.n_dst) {
    bool dead = false;
    if (a.masked && L.imask) dead = (L.imask[d] == 0);
    if (a.area_min > 0.0 && L.frac) dead = dead || (L.frac[d] < a.area_min);
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      if (j0 + t < a.n_j) yr[t][d] = epilogue(acc[t].num, dead);
    }
  }
}

}  // namespace

namespace smm_launch {

int launch_grib(const GribArgs& a, bool div, bool fill, hipStream_t s) {
  GribArgs args = a;
  auto go = [&](auto bt_tag, auto div_tag) -> int {
    constexpr int BT = decltype(bt_tag)::value;
    args.n_jtiles = (a.n_j + BT - 1) / BT;
    const int64_t total = args.n_dblocks * args.n_jtiles;
    if (total <= 0) return SMM_OK;
    if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "launch grid exceeds 2^31-1 blocks");
    hipLaunchKernelGGL((smm_apply_grib_kernel<BT, decltype(div_tag)::value>), dim3((unsigned)total), dim3(kThreads), 0, s,
                       args, fill);
    SMM_LAUNCH_HIP(hipGetLastError());
    return SMM_OK;
  };
  auto with_bt = [&](auto div_tag) -> int {
    switch (sell_batch_rows(a.n_j)) {   // as launch_sell: 4 rows per thread, SMM_TUNE_SELL_BATCH_ROWS asks for 8 or 2
      case 8: return go(std::integral_constant<int, 8>(), div_tag);
      case 4: return go(std::integral_constant<int, 4>(), div_tag);
      case 2: return go(std::integral_constant<int, 2>(), div_tag);
      default: return go(std::integral_constant<int, 1>(), div_tag);
    }
  };
  return div ? with_bt(std::true_type()) : with_bt(std::false_type());
}

}  // namespace smm_launch
