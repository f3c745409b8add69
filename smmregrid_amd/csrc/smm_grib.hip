// smm_apply_grib's kernel and launcher (gfx950): kernel A with the gather replaced -- per link two unconditional
// 32-bit loads from the packed bit stream, a byte swap, a 64-bit shift and the row's decode rule.  For
// smm_apply_grib_bm: the two kernels that build the rank tables of bitmapped rows, and the gather that reads them.
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
// BM (smm_apply_grib_bm): a row with a bitmap loads, per link, the 8-byte rank-table entry of the cell's 32-cell block
// and reads the stream at the cell's rank; its table pointer -- null for a row without a bitmap, which takes
// rank = c, present = true -- is scalar like the rest of the rule, so the branch on it is block-uniform.
// GRP (smm_group_apply_grib): the block id splits into (destination block, batch tile, level) as in
// smm_apply_sell_kernel; the level's descriptor comes from descs[lev_map[l]], its mask switch from lev_masked, and the
// BT batch rows are rows (o, i) of that one level: row j of the level is record o * rec_o + l * rec_l + i of the row
// table and the bitmap records -- a block-uniform index like j itself, so the rule stays in scalar registers -- and its
// results go to y + o * ys_o + l * ys_l + i * ys_i.
// NA (the _na entries): the SMM_APPLY_SKIPNA rule of include/smmregrid_amd.h as smm_apply_sell_kernel<float, double, BT,
// true> applies it to the decoded field -- the value goes to a RowSum<float, true> raw (no 1e20 fill; a missing cell is
// the NaN of the select), tot takes every slot's weight in slot order, and the store is skipna_epilogue with the static
// mask alone.
template <bool GRP, bool BM>
using GribKernelArgs = std::conditional_t<GRP, GribGroupArgs, std::conditional_t<BM, GribBitmapArgs, GribArgs>>;

template <int BT, bool DIV, bool BM, bool GRP = false, bool NA = false>
__global__ __launch_bounds__(kThreads) void smm_apply_grib_kernel(GribKernelArgs<GRP, BM> a, bool fill) {
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int64_t bid = blockIdx.x;
  int64_t db = bid % a.n_dblocks;
  int64_t jt = bid / a.n_dblocks;
  int64_t l = 0;
  int di = 0;
  if constexpr (GRP) {
    // the grid has fewer than 2^31 blocks, so its three factors fit 32 bits: plain 32-bit scalar divisions
    const uint32_t nd = (uint32_t)a.n_dblocks, nt = (uint32_t)a.n_jtiles;
    const uint32_t q = blockIdx.x / nd, lev = q / nt;
    db = blockIdx.x - q * nd;
    jt = q - lev * nt;
    l = lev;
    di = a.lev_map[l];
  }
  const LevelDesc L = a.descs[di];

  const int64_t slice = db * kWavesPerBlock + wave;
  const int64_t d = slice * 64 + lane;
  if (slice * 64 >= a.n_dst) return;

  const int64_t j0 = jt * BT;
  // GRP: (o, i) of the block's first batch row -- one division per block; a launch holds fewer than 2^31 rows per
  // level (launch_grib_group), so 32 bits do.  The rows are walked from it twice, for the rules here and for the Y
  // rows in the epilogue: BT result pointers would sit in scalar registers through the whole link loop.
  uint32_t go0 = 0, gi0 = 0;
  bool use_mask = a.masked != 0;
  if constexpr (GRP) {
    go0 = (uint32_t)j0 / (uint32_t)a.n_inner;
    gi0 = (uint32_t)j0 - go0 * (uint32_t)a.n_inner;
    use_mask = use_mask && (a.lev_masked ? a.lev_masked[di] != 0 : true);
  }
  uint32_t go = go0, gi = gi0;
  const smm_grib_row_t* __restrict__ rows = a.rows;
  const uint32_t* __restrict__ xw[BT];
  double* __restrict__ yr[GRP ? 1 : BT];
  uint32_t bit0[BT], lastw[BT];
  int nbits[BT];
  double ref[BT], bscale[BT], ddiv[BT];
  const smm_grib::GribRankEntry* __restrict__ tab[BM ? BT : 1];
#pragma unroll
  for (int t = 0; t < BT; ++t) {
    int64_t j = j0 + t;
    if (j > a.n_j - 1) j = a.n_j - 1;
    int64_t rec = j;
    if constexpr (GRP) {
      rec = (int64_t)go * a.rec_o + l * a.rec_l + gi;
      if (j0 + t < a.n_j - 1 && ++gi == (uint32_t)a.n_inner) gi = 0, ++go;   // the next row; past the last: repeated
    }
    const smm_grib_row_t r = rows[rec];
    if constexpr (BM) {
      const GribRowBitmap* __restrict__ bm = a.bm;
      const GribRowBitmap m = bm[rec];
      tab[t] = m.bitmap_off == SMM_GRIB_NO_BITMAP ? nullptr : a.table + m.table_off;
    }
    // a 0-bit row may start at the very end of the buffer: its words are clamped like every other load
    const uint64_t w = std::min<uint64_t>(r.byte_off >> 2, a.last_word);
    xw[t] = a.x + w;
    lastw[t] = (uint32_t)std::min<uint64_t>(a.last_word - w, 0xfffffffeull);
    bit0[t] = 8u * (uint32_t)(r.byte_off & 3);
    nbits[t] = r.nbits;
    ref[t] = r.ref;
    bscale[t] = r.bscale;
    ddiv[t] = r.ddiv;
    if constexpr (!GRP) yr[t] = a.y + j * a.ldy;
  }

  const int64_t off = L.slice_off[slice];
  const int nslots = (int)((L.slice_off[slice + 1] - off) >> 6);
  const int len = L.rowlen[d];
  const int32_t* __restrict__ cp = L.col + off + lane;
  const double* __restrict__ vp = L.val + off + lane;

  RowSum<float, NA> acc[BT];
  [[maybe_unused]] double tot = 0.0;   // NA: the row's weight sum, shared by the BT batch rows
  // padded slots: a valid column and weight +0.0, bitwise no-ops on a finite value (smm_apply_sell_kernel)
#pragma unroll 2
  for (int k = 0; k < nslots; ++k) {
    const uint32_t c = (uint32_t)cp[(int64_t)k * 64];
    const double w = vp[(int64_t)k * 64];
    double xv[BT];
#pragma unroll
    for (int t = 0; t < BT; ++t) {
      uint32_t i = c;   // the value's index in the row's stream
      bool present = true;
      if constexpr (BM) {
        if (tab[t]) {
          const smm_grib::GribRankEntry e = tab[t][c >> 5];
          i = smm_grib::bitmap_index(e, c);
          present = smm_grib::bitmap_present(e, c);
        }
      }
      const uint64_t p = (uint64_t)bit0[t] + (uint64_t)i * (uint32_t)nbits[t];
      const uint32_t q = smm_grib::grib_extract(xw[t], p, nbits[t], lastw[t]);
      float v = smm_grib::grib_decode<DIV>(q, ref[t], bscale[t], ddiv[t]);
      if constexpr (BM) v = present ? v : __builtin_nanf("");   // a missing cell: its loads went out, a select drops them
      if constexpr (NA)
        xv[t] = (double)v;
      else
        xv[t] = (double)((fill && !__builtin_isfinite(v)) ? (float)1e20 : v);
    }
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[t].add(w, xv[t]);
    if constexpr (NA) tot = tot + w;
  }
  if (len == 0) {
#pragma unroll
    for (int t = 0; t < BT; ++t) acc[t].clear();
  }

  if (d < a.n_dst) {
    bool dead = false;
    if (use_mask && L.imask) dead = (L.imask[d] == 0);
    [[maybe_unused]] double frac_d = 1.0;
    if constexpr (NA) {
      if (L.frac) frac_d = L.frac[d];   // the area test is skipna_epilogue's
    } else {
      if (a.area_min > 0.0 && L.frac) dead = dead || (L.frac[d] < a.area_min);
    }
    auto finish = [&](const RowSum<float, NA>& s) -> double {
      if constexpr (NA)
        return skipna_epilogue(s.num, s.den, s.inv, tot, dead, L.frac != nullptr, frac_d, a.area_min);
      else
        return epilogue(s.num, dead);
    };
    if constexpr (GRP) {
      go = go0, gi = gi0;
#pragma unroll
      for (int t = 0; t < BT; ++t) {
        if (j0 + t < a.n_j) {
          double* __restrict__ yrow = a.y + ((int64_t)go * a.ys_o + l * a.ys_l + (int64_t)gi * a.ys_i);
          yrow[d] = finish(acc[t]);
          if (++gi == (uint32_t)a.n_inner) gi = 0, ++go;
        }
      }
    } else {
#pragma unroll
      for (int t = 0; t < BT; ++t) {
        if (j0 + t < a.n_j) yr[t][d] = finish(acc[t]);
      }
    }
  }
}

// ---- the rank tables of smm_apply_grib_bm.  One workgroup per (row, segment of kGribSegBlocks 32-cell blocks); a
// thread holds kBuildPerThread consecutive blocks.  Rows without a bitmap leave at once (block-uniform).
constexpr int kBuildThreads = 256, kBuildWaves = kBuildThreads / 64;
constexpr int kBuildPerThread = smm_grib::kGribSegBlocks / kBuildThreads;
static_assert(kBuildPerThread * kBuildThreads == smm_grib::kGribSegBlocks, "a segment is whole blocks per thread");

struct BuildRow {
  const uint32_t* __restrict__ words;
  uint32_t bit0, lastw;
};
__device__ __forceinline__ BuildRow build_row(const GribBuildArgs& a, uint64_t bitmap_off) {
  const uint64_t w = std::min<uint64_t>(bitmap_off >> 2, a.last_word);   // as the gather clamps a row's first word
  return BuildRow{a.x + w, 8u * (uint32_t)(bitmap_off & 3), (uint32_t)std::min<uint64_t>(a.last_word - w, 0xfffffffeull)};
}
// sum over the wave, in every lane
__device__ __forceinline__ uint32_t wave_sum(uint32_t v) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o, 64);
  return v;
}

// 1: totals[table number * n_segs + seg] = set bits of the segment
__global__ __launch_bounds__(kBuildThreads) void smm_grib_bitmap_totals_kernel(GribBuildArgs a) {
  __shared__ uint32_t wsum[kBuildWaves];
  const int64_t j = blockIdx.x / a.n_segs;
  const uint32_t seg = blockIdx.x % a.n_segs;
  const GribRowBitmap* __restrict__ bm = a.bm;
  const uint64_t off = bm[j].bitmap_off;
  if (off == SMM_GRIB_NO_BITMAP) return;
  const BuildRow r = build_row(a, off);
  const uint32_t k0 = seg * (uint32_t)smm_grib::kGribSegBlocks + threadIdx.x * kBuildPerThread;
  uint32_t n = 0;
#pragma unroll
  for (int i = 0; i < kBuildPerThread; ++i)
    if (k0 + i < a.n_blocks) n += smm_grib::popcount32(smm_grib::bitmap_block(r.words, r.bit0, k0 + i, a.n_src, r.lastw));
  n = wave_sum(n);
  if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = n;
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t t = 0;
#pragma unroll
    for (int w = 0; w < kBuildWaves; ++w) t += wsum[w];
    a.totals[bm[j].table_off / a.n_blocks * a.n_segs + seg] = t;   // every table has n_blocks entries: its number
  }
}

// 2: the entries of one segment.  The totals of the segments before it are summed by the whole workgroup; inside the
// segment a thread's blocks are scanned in registers, the threads of a wave by an inclusive shuffle scan, the waves
// through LDS.
__global__ __launch_bounds__(kBuildThreads) void smm_grib_bitmap_scan_kernel(GribBuildArgs a) {
  __shared__ uint32_t wsum[kBuildWaves], wbefore[kBuildWaves];
  const int64_t j = blockIdx.x / a.n_segs;
  const uint32_t seg = blockIdx.x % a.n_segs;
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const GribRowBitmap* __restrict__ bm = a.bm;
  const GribRowBitmap m = bm[j];
  if (m.bitmap_off == SMM_GRIB_NO_BITMAP) return;
  const BuildRow r = build_row(a, m.bitmap_off);

  uint32_t before = 0;
  const uint32_t* __restrict__ tot = a.totals + m.table_off / a.n_blocks * a.n_segs;
  for (uint32_t s = threadIdx.x; s < seg; s += kBuildThreads) before += tot[s];
  before = wave_sum(before);
  if (lane == 0) wbefore[wave] = before;

  const uint32_t k0 = seg * (uint32_t)smm_grib::kGribSegBlocks + threadIdx.x * kBuildPerThread;
  uint32_t bits[kBuildPerThread], mine = 0;
#pragma unroll
  for (int i = 0; i < kBuildPerThread; ++i) {
    bits[i] = k0 + i < a.n_blocks ? smm_grib::bitmap_block(r.words, r.bit0, k0 + i, a.n_src, r.lastw) : 0u;
    mine += smm_grib::popcount32(bits[i]);
  }
  uint32_t incl = mine;   // inclusive scan over the lanes of the wave
#pragma unroll
  for (int o = 1; o < 64; o <<= 1) {
    const uint32_t up = __shfl_up(incl, o, 64);
    if (lane >= o) incl += up;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  uint32_t rank = incl - mine;
#pragma unroll
  for (int w = 0; w < kBuildWaves; ++w) {
    rank += wbefore[w];
    if (w < wave) rank += wsum[w];
  }
  smm_grib::GribRankEntry* __restrict__ out = a.table + m.table_off;
#pragma unroll
  for (int i = 0; i < kBuildPerThread; ++i) {
    if (k0 + i < a.n_blocks) out[k0 + i] = smm_grib::GribRankEntry{bits[i], rank};
    rank += smm_grib::popcount32(bits[i]);
  }
}

}  // namespace

namespace smm_launch {

namespace {
// n_lev: the levels of a grouped launch (GribGroupArgs), 1 for the operator entries
template <bool BM, bool GRP, class Args>
int launch_grib_any(const Args& a, int64_t n_lev, bool div, bool na, bool fill, hipStream_t s) {
  Args args = a;
  auto go = [&](auto bt_tag, auto div_tag, auto na_tag) -> int {
    constexpr int BT = decltype(bt_tag)::value;
    args.n_jtiles = (a.n_j + BT - 1) / BT;
    const int64_t total = args.n_dblocks * args.n_jtiles * n_lev;
    if (total <= 0) return SMM_OK;
    if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "launch grid exceeds 2^31-1 blocks");
    hipLaunchKernelGGL((smm_apply_grib_kernel<BT, decltype(div_tag)::value, BM, GRP, decltype(na_tag)::value>),
                       dim3((unsigned)total), dim3(kThreads), 0, s, args, fill);
    SMM_LAUNCH_HIP(hipGetLastError());
    return SMM_OK;
  };
  auto with_bt = [&](auto div_tag, auto na_tag) -> int {
    switch (sell_batch_rows(a.n_j)) {   // as launch_sell: 4 rows per thread, SMM_TUNE_SELL_BATCH_ROWS asks for 8 or 2
      case 8: return go(std::integral_constant<int, 8>(), div_tag, na_tag);
      case 4: return go(std::integral_constant<int, 4>(), div_tag, na_tag);
      case 2: return go(std::integral_constant<int, 2>(), div_tag, na_tag);
      default: return go(std::integral_constant<int, 1>(), div_tag, na_tag);
    }
  };
  auto with_div = [&](auto na_tag) -> int {
    return div ? with_bt(std::true_type(), na_tag) : with_bt(std::false_type(), na_tag);
  };
  return na ? with_div(std::true_type()) : with_div(std::false_type());
}
}  // namespace

int launch_grib(const GribArgs& a, bool div, bool na, bool fill, hipStream_t s) {
  return launch_grib_any<false, false>(a, 1, div, na, fill, s);
}
int launch_grib_bitmap(const GribBitmapArgs& a, bool div, bool na, bool fill, hipStream_t s) {
  return launch_grib_any<true, false>(a, 1, div, na, fill, s);
}
int launch_grib_group(const GribGroupArgs& a, int64_t n_lev, bool bitmaps, bool div, bool na, bool fill, hipStream_t s) {
  return bitmaps ? launch_grib_any<true, true>(a, n_lev, div, na, fill, s)
                 : launch_grib_any<false, true>(a, n_lev, div, na, fill, s);
}

int launch_grib_build(const GribBuildArgs& a, hipStream_t s) {
  const int64_t total = a.n_j * (int64_t)a.n_segs;
  if (total <= 0) return SMM_OK;
  if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "bitmap table build exceeds 2^31-1 blocks");
  hipLaunchKernelGGL(smm_grib_bitmap_totals_kernel, dim3((unsigned)total), dim3(kBuildThreads), 0, s, a);
  SMM_LAUNCH_HIP(hipGetLastError());
  hipLaunchKernelGGL(smm_grib_bitmap_scan_kernel, dim3((unsigned)total), dim3(kBuildThreads), 0, s, a);
  SMM_LAUNCH_HIP(hipGetLastError());
  return SMM_OK;
}

}  // namespace smm_launch
