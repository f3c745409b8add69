// Kernel launch templates, one explicit instantiation per built (X type, Y type, SKIPNA) triple -- the list is SMM_BUILT
// in smm_built.hpp.  smm_launch_inst.hip is compiled once per variant of the Makefile's INST list, twenty-eight objects side by
// side: the tile kernel alone has several hundred instantiations, which one translation unit would compile for minutes.
// SKIPNA = true builds the SMM_APPLY_SKIPNA variants (smm_kernels.hpp, RowSum) in objects of their own.
#pragma once

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstdint>
#include <string>
#include <type_traits>

#include "../../include/smmregrid_amd.h"
#include "smm_kernels.hpp"

#pragma clang fp contract(off)

namespace smm {
int fail_msg(int code, const std::string& msg);   // sets the thread-local error text (smm_device.hip)
int tuning(int knob);                             // smm_debug_set_tuning's current value (0 = library default)
}

namespace smm_launch {

#define SMM_LAUNCH_HIP(call)                                                              \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess) {                                                               \
      (void)hipGetLastError();                                                            \
      return smm::fail_msg(SMM_ERR_HIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
    }                                                                                     \
  } while (0)

// batch rows per thread of the SELL kernel for a batch of n_j rows
inline int sell_batch_rows(int64_t n_j) {
  const int want = smm::tuning(SMM_TUNE_SELL_BATCH_ROWS);
  if (n_j >= 8 && want == 8) return 8;
  if (n_j >= 4 && want != 2) return 4;
  return n_j >= 2 ? 2 : 1;
}

// Extra dynamic LDS requested for every wave of the batch-fastest kernels (tuning knob SMM_TUNE_SB_LDS_PAD, bytes): it
// caps the waves per CU -- the 16.6-KB tile alone allows 9.  Measured (profiles/r05_sb_experiments.txt): config 3 is level
// down to 7 waves per CU and loses below; config 2 gains 0 - 5 % at 6 - 8.  No pad by default.
inline size_t sb_lds_pad() { return (size_t)std::max(smm::tuning(SMM_TUNE_SB_LDS_PAD), 0); }

// consecutive logical blocks given to one XCD (tile and batch-fastest kernels); 0 = dispatcher order
inline int xcd_run_length() {
  const int want = smm::tuning(SMM_TUNE_XCD_RUN);
  return want < 0 ? 0 : (want > 0 ? want : 32);
}

// Destination rows per tile (TD) of the batch-fastest kernel for a Y element of ysz bytes: one 128-B line of Y per
// batch row for f64 (16 rows) and f32 (32).  A 2-byte Y (packed or half precision) takes 64 rows -- the same 128-B runs, a 17-KB LDS tile
// like f64's -- or 16 (32-B runs, a 4-KB tile) under SMM_TUNE_SB_PACKED_Y_ROWS = 16: both are built, DESIGN.md section 4
// has the measurement.
inline int sb_tile_rows(size_t ysz) {
  if (ysz == 8) return 16;
  if (ysz == 4) return 32;
  return smm::tuning(SMM_TUNE_SB_PACKED_Y_ROWS) == 16 ? 16 : 64;
}

template <typename XT, typename YT, bool SKIPNA>
int launch_sell(const ApplyArgs& a, int64_t n_lev, bool fill, unsigned flags, hipStream_t s) {
  ApplyArgs args = a;
  auto go = [&](auto bt_tag) -> int {
    constexpr int BT = decltype(bt_tag)::value;
    args.n_jtiles = (a.n_j + BT - 1) / BT;
    const int64_t total = args.n_dblocks * args.n_jtiles * n_lev;
    if (total <= 0) return SMM_OK;
    if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "launch grid exceeds 2^31-1 blocks");
    hipLaunchKernelGGL((smm_apply_sell_kernel<XT, YT, BT, SKIPNA>), dim3((unsigned)total), dim3(kThreads), 0,
                       s, args, fill);
    SMM_LAUNCH_HIP(hipGetLastError());
    return SMM_OK;
  };
  // batch rows per thread: 4 (gather-bound operators want many waves in flight: scatter -3 %,
  // config 2 -1 % against 8); SMM_TUNE_SELL_BATCH_ROWS asks for 8 or 2
  switch (sell_batch_rows(a.n_j)) {
    case 8: return go(std::integral_constant<int, 8>());
    case 4: return go(std::integral_constant<int, 4>());
    case 2: return go(std::integral_constant<int, 2>());
    default: return go(std::integral_constant<int, 1>());
  }
}

// Launch geometry of the tile kernel, shared by the launcher and smm_operator_launch_info.
struct TileLaunchCfg {
  int j_per_block = 0;     // batch rows walked by one workgroup
  int64_t n_jtiles = 0;
  int64_t total = 0;       // workgroups
  int xcd_remap = 0;
  int threads = 0;
  int np_needed = 0;       // 16-B staging pieces per thread of the widest block
  int rows = 1;            // batch rows staged per barrier pair (R)
  bool dma = false;        // staging by LDS-DMA into a ring of two tile slots (single-row steps)
  size_t tile = 0, lds = 0;
  bool big_operator = false;
};

inline TileLaunchCfg tile_launch_cfg(const ApplyArgs& a, int64_t n_lev, int tile_which, int64_t max_chunks,
                                     int64_t max_row_nnz, unsigned flags, size_t xsz) {
  TileLaunchCfg c;
  (void)flags;
  const int jpb = std::max(smm::tuning(SMM_TUNE_TILE_WALK), 0);
  const int staging = smm::tuning(SMM_TUNE_TILE_STAGING);          // 1 = registers, 2 = LDS-DMA forced
  const int rows_knob = smm::tuning(SMM_TUNE_TILE_ROWS_PER_STEP);  // 1 / 2 / 4
  // Batch rows walked per workgroup: the prologue (links -> registers) is amortised over
  // them, so heavier rows want longer walks; keep >= ~4096 workgroups to fill 256 CUs.
  // An operator that does not stay in L2 (links x 12 B beyond ~32 MB) is re-read from HBM by every
  // walk: amortise it over long walks whatever the row length.
  c.big_operator = a.n_dst * std::max<int64_t>(max_row_nnz, 1) * 12 > (32ll << 20);
  int64_t walk = jpb ? (int64_t)jpb : (c.big_operator ? 128 : (max_row_nnz <= 4 ? 4 : 64));
  if (!jpb)
    while (walk > 1 && a.n_dblocks * ((a.n_j + walk - 1) / walk) * n_lev < 4096) walk /= 2;
  c.j_per_block = (int)std::min<int64_t>(a.n_j, walk);
  c.n_jtiles = c.j_per_block > 0 ? (a.n_j + c.j_per_block - 1) / c.j_per_block : 0;
  c.total = a.n_dblocks * c.n_jtiles * n_lev;
  // runs of 32 consecutive blocks per XCD (SMM_TUNE_XCD_RUN: another run length, -1 = dispatcher order)
  c.xcd_remap = xcd_run_length();
  const int64_t max_pieces = max_chunks * (int64_t)(kChunkElems * xsz / 16);
  c.threads = (tile_which ? 1 : kWavesPerBlock) * 64;  // == tile_waves(MAXK) * 64
  c.np_needed = (int)((max_pieces + c.threads - 1) / c.threads);
  // whole rounds of one 16-B piece per thread: every lane stores its pieces unpredicated, the
  // last round's surplus lands in padding
  c.tile = (size_t)std::max(c.np_needed, 1) * c.threads * 16;
  // Small tiles (one or two 16-B pieces per thread, 4-wave shape): a step of 4 / 2 batch rows per
  // barrier pair keeps as many bytes in flight as a full tile would (SMM_TUNE_TILE_ROWS_PER_STEP lowers it).
  c.rows = 1;
  if (!tile_which) c.rows = c.np_needed <= 1 ? 4 : (c.np_needed <= 2 ? 2 : 1);
  while (c.rows > 1 && (c.rows > c.j_per_block || (rows_knob > 0 && c.rows > rows_knob))) c.rows /= 2;
  // LDS-DMA staging instead (smm_kernels.hpp, DMA): on by default for the small tiles the multi-row
  // steps serve (two slots of <= 8 KB keep every workgroup slot of the CU), SMM_TUNE_TILE_STAGING = 2 forces it
  // for any tile of either block shape that keeps its links in registers, 1 switches it off.
  // The DMA moves aligned 16-B pieces: base, strides and row length must be multiples of 16 B.
  const bool aligned = ((uintptr_t)a.x % 16 == 0) && (a.xs_o * (int64_t)xsz % 16 == 0) &&
                       (a.xs_l * (int64_t)xsz % 16 == 0) && (a.xs_i * (int64_t)xsz % 16 == 0) &&
                       (a.n_src * (int64_t)xsz % 16 == 0);
  const bool wanted = staging == 2 || (staging == 0 && !tile_which && c.np_needed <= 2);
  c.dma = wanted && aligned && a.sub_shift == 0 && max_row_nnz > 0 && max_row_nnz <= 48 && 2 * c.tile <= 65536;
  if (c.dma) {
    // Rows per step of the DMA ring (two groups of `rows` slots).  Tiles of one piece per thread (4 KB:
    // coarse -> fine regrids, whose steps are pure round trips) take two rows per step -- 16 KB per
    // workgroup still keeps every workgroup slot of the CU (upsampling r360x180 -> r1440x721 2.71 -> 2.39 ms);
    // with 8-KB tiles two rows cost workgroups (config-4 geometry 4.71 -> 5.05 ms, four rows 5.92).
    // SMM_TUNE_TILE_ROWS_PER_STEP picks one, two or four.
    c.rows = 1;
    if (!tile_which && c.np_needed <= 4)
      c.rows = (rows_knob == 1 || rows_knob == 2 || rows_knob == 4) ? rows_knob : (c.np_needed <= 1 ? 2 : 1);
    while (c.rows > 1 && (c.rows > c.j_per_block || 2 * c.rows * c.tile > 65536)) c.rows /= 2;
  }
  c.lds = c.dma ? 2 * (size_t)c.rows * c.tile : c.tile * (size_t)c.rows;
  return c;
}

// Part-of-a-slice blocks (sub_shift > 0) let the idle lanes take over parts of the rows (SPLIT kernels) when a
// lane group's share fits the link registers (SMM_TUNE_TILE_SPLIT_ROWS = 1: off, for A/B runs).
inline bool tile_split(int sub_shift, int64_t max_row_nnz) {
  return sub_shift > 0 && smm::tuning(SMM_TUNE_TILE_SPLIT_ROWS) != 1 && max_row_nnz <= ((int64_t)48 << sub_shift);
}

// Whether the tile form launch_tile would pick has an SMM_APPLY_SKIPNA variant: the forms that keep the links in
// registers, one lane per row (4-wave blocks, single-wave blocks of 17 - 48 links, register or LDS-DMA staging).
// SPLIT rows and rows streamed from L2 (more than 48 links) have none: SKIPNA runs kernel A for them.
inline bool tile_has_skipna(int tile_which, int sub_shift, int64_t max_row_nnz) {
  if (!tile_which) return max_row_nnz <= 16;
  if (tile_split(sub_shift, max_row_nnz)) return false;
  return smm::tuning(SMM_TUNE_TILE_LINKS) != 1 && max_row_nnz <= 48;
}

template <typename XT, typename YT, bool SKIPNA>
int launch_tile(const ApplyArgs& a, int64_t n_lev, int tile_which, int64_t max_chunks,
                int64_t max_row_nnz, int tile_flags, bool fill, unsigned flags, hipStream_t s) {
  ApplyArgs args = a;
  const TileLaunchCfg cfg = tile_launch_cfg(a, n_lev, tile_which, max_chunks, max_row_nnz, flags, sizeof(XT));
  args.j_per_block = cfg.j_per_block;
  args.n_jtiles = cfg.n_jtiles;
  const int64_t total = cfg.total;
  if (total <= 0) return SMM_OK;
  if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "launch grid exceeds 2^31-1 blocks");
  args.n_blocks = total;
  args.xcd_remap = cfg.xcd_remap;
  const int np_needed = cfg.np_needed;
  const int rows = cfg.rows;
  args.tile_bytes = (int)cfg.tile;
  const size_t lds = cfg.lds;

  const bool dma = cfg.dma;   // LDS-DMA staging into a ring of two tile slots (tile_launch_cfg)
  // one tile form: links in registers (MAXK, 0 = streamed), pieces per thread, NT bits, rows per step, SPLIT, DMA
  auto go3 = [&](auto k_tag, auto np_tag, auto nt_tag, auto r_tag, auto split_tag, auto dma_tag) -> int {
    constexpr int MAXK = decltype(k_tag)::value;
    constexpr int NP = decltype(np_tag)::value;
    constexpr int NT = decltype(nt_tag)::value;
    constexpr int R = decltype(r_tag)::value;
    hipLaunchKernelGGL((smm_apply_tile2_kernel<XT, YT, MAXK, NP, NT, R, decltype(split_tag)::value, decltype(dma_tag)::value, SKIPNA>),
                       dim3((unsigned)total), dim3(tile_waves(MAXK) * 64), lds, s, args, fill);
    SMM_LAUNCH_HIP(hipGetLastError());
    return SMM_OK;
  };
  auto go_dma = [&](auto k_tag, auto np_tag, auto nt_tag) -> int {
    constexpr int MAXK = decltype(k_tag)::value;
    if constexpr (MAXK > 0) {
      auto go_r = [&](auto r_tag) -> int { return go3(k_tag, np_tag, nt_tag, r_tag, std::false_type(), std::true_type()); };
      if constexpr (MAXK <= 16 && decltype(np_tag)::value <= 4) {
        if (rows == 4) return go_r(std::integral_constant<int, 4>());
        if (rows == 2) return go_r(std::integral_constant<int, 2>());
      }
      return go_r(std::integral_constant<int, 1>());
    } else {
      return smm::fail_msg(SMM_ERR_UNSUPPORTED, "LDS-DMA staging needs the links in registers");
    }
  };
  // Part-of-a-slice blocks: the idle lanes take over parts of the rows (SPLIT kernels, tile_split).
  const int n_grp = 1 << args.sub_shift;
  const bool split = tile_split(args.sub_shift, max_row_nnz);
  const int64_t per_grp = (max_row_nnz + n_grp - 1) / n_grp;
  if (SKIPNA && !tile_has_skipna(tile_which, args.sub_shift, max_row_nnz))
    return smm::fail_msg(SMM_ERR_UNSUPPORTED, "SMM_APPLY_SKIPNA: the planned tile form (split or streamed rows) has no skipna variant");
  auto go2 = [&](auto k_tag, auto np_tag, auto nt_tag) -> int {
    constexpr int MAXK = decltype(k_tag)::value;
    if (dma) return go_dma(k_tag, np_tag, nt_tag);
    if constexpr (!SKIPNA && (MAXK == 32 || MAXK == 48)) {
      if (split) return go3(k_tag, np_tag, nt_tag, std::integral_constant<int, 1>(), std::true_type(), std::false_type());
    }
    auto go_r = [&](auto np, auto r_tag) -> int { return go3(k_tag, np, nt_tag, r_tag, std::false_type(), std::false_type()); };
    if constexpr (MAXK > 0 && MAXK <= 16) {
      if (rows == 4) return go_r(std::integral_constant<int, 1>(), std::integral_constant<int, 4>());
      if (rows == 2) return go_r(std::integral_constant<int, 2>(), std::integral_constant<int, 2>());
    }
    if constexpr (SKIPNA && MAXK == 0)
      return smm::fail_msg(SMM_ERR_INTERNAL, "SMM_APPLY_SKIPNA reached the streamed-link tile form");   // refused above
    else
      return go_r(np_tag, std::integral_constant<int, 1>());
  };
  auto with_k = [&](auto fn) -> int {  // plan shape 0 <-> 4 waves (rows of <= 16 links), shape 1.. <-> 1 wave
    if (!tile_which) {
      if (max_row_nnz > 16)
        return smm::fail_msg(SMM_ERR_UNSUPPORTED, "4-wave tile blocks serve rows of at most 16 links");
      if (max_row_nnz <= 4) return fn(std::integral_constant<int, 4>());
      if (max_row_nnz <= 8) return fn(std::integral_constant<int, 8>());
      return fn(std::integral_constant<int, 16>());
    }
    if (smm::tuning(SMM_TUNE_TILE_LINKS) == 1) return fn(std::integral_constant<int, 0>());  // tuning: stream the links
    if (split) return per_grp <= 32 ? fn(std::integral_constant<int, 32>()) : fn(std::integral_constant<int, 48>());
    if (max_row_nnz <= 32) return fn(std::integral_constant<int, 32>());
    if (max_row_nnz <= 48) return fn(std::integral_constant<int, 48>());
    return fn(std::integral_constant<int, 0>());  // longer rows: links streamed from L2
  };
  if (np_needed > 16)
    return smm::fail_msg(SMM_ERR_UNSUPPORTED, "tile plan exceeds the staging register budget");
  // Y stores are always non-temporal; X loads are non-temporal only if no staged line is shared between
  // blocks (tile_reuse false).  SMM_TUNE_TILE_X_LOADS = 1 / 2 forces non-temporal / cached X loads.  (Cached Y
  // stores measured flat or worse everywhere and are no longer built.)
  const bool tile_reuse = tile_flags & 1;
  int nt = tile_reuse ? 2 : 3;
  if (smm::tuning(SMM_TUNE_TILE_X_LOADS) == 1) nt = 3;
  if (smm::tuning(SMM_TUNE_TILE_X_LOADS) == 2) nt = 2;
  return with_k([&](auto k_tag) -> int {
    auto with_nt = [&](auto np_tag) -> int {
      if (nt == 2) return go2(k_tag, np_tag, std::integral_constant<int, 2>());
      return go2(k_tag, np_tag, std::integral_constant<int, 3>());
    };
    if (np_needed <= 4) return with_nt(std::integral_constant<int, 4>());
    if (np_needed <= 8) return with_nt(std::integral_constant<int, 8>());
    return with_nt(std::integral_constant<int, 16>());
  });
}

// Batch-fastest layout (kernel C).  TD destination rows per tile: 16 doubles = one 128-B line of Y
// per batch row; f32 output takes 32 rows for the same line; a packed 2-byte Y: sb_tile_rows.
template <typename YT, typename F>
int with_sb_tile_rows(F fn) {
  constexpr size_t YSZ = sizeof(typename YTraits<YT>::raw);
  if constexpr (YSZ == 8) return fn(std::integral_constant<int, 16>());
  else if constexpr (YSZ == 4) return fn(std::integral_constant<int, 32>());
  else
    return sb_tile_rows(YSZ) == 16 ? fn(std::integral_constant<int, 16>()) : fn(std::integral_constant<int, 64>());
}

// The two kernels behind launch_sb_any: the kernel template, and where its argument struct keeps the grid size.
struct SbSingle {
  template <typename XT, typename YT, int TD, int U, bool FILL, bool YSB, bool SKIPNA>
  static constexpr auto kernel() { return &smm_apply_sb_kernel<XT, YT, TD, U, FILL, YSB, SKIPNA>; }
  static int64_t set_grid(SbArgs& a, int64_t tiles) { return a.n_blocks = tiles; }
};
// grid = levels x (destination tiles x batch tiles); the caller has filled a.lev[0 .. n_lev) and the per-level strides
struct SbGroup {
  template <typename XT, typename YT, int TD, int U, bool FILL, bool YSB, bool SKIPNA>
  static constexpr auto kernel() { return &smm_group_apply_sb_kernel<XT, YT, TD, U, FILL, YSB, SKIPNA>; }
  static int64_t set_grid(SbGroupArgs& a, int64_t tiles) { return (a.blocks_per_level = tiles) * a.n_lev; }
};

template <typename K, typename XT, typename YT, bool SKIPNA, int TD, typename Args>
int launch_sb_any(const Args& a, bool fill, unsigned flags, hipStream_t s) {
  Args args = a;
  constexpr int BT = 128;
  args.n_dtiles = (a.n_dst + TD - 1) / TD;
  args.n_btiles = (a.n_batch + BT - 1) / BT;
  const int64_t total = K::set_grid(args, args.n_dtiles * args.n_btiles);
  if (total <= 0) return SMM_OK;
  if (total > 0x7fffffffLL) return smm::fail_msg(SMM_ERR_INVALID, "launch grid exceeds 2^31-1 blocks");
  args.xcd_remap = xcd_run_length();
  // Tile order: strips of 2 destination tiles, inside a strip destination tile fastest, then batch tile
  // (config 2: 1.76 -> 1.65 ms against destination-tile-fastest order over the whole grid; strips of 1, 4,
  // 8, 16 tiles within 3 % of it).  SMM_TUNE_SB_STRIP: -1 = whole-grid order, n = strips of n tiles.
  const int strip = smm::tuning(SMM_TUNE_SB_STRIP);
  args.b_fastest = strip < 0 ? 0 : (strip > 0 ? strip : 2);
  const bool ysb = (flags & SMM_APPLY_SB_Y_SB) != 0;   // result kept batch-fastest: Y (D, ldy >= B)
  auto go = [&](auto u_tag, auto fill_tag) {
    constexpr int UU = decltype(u_tag)::value;
    constexpr bool FF = decltype(fill_tag)::value;
    if (ysb)
      hipLaunchKernelGGL((K::template kernel<XT, YT, TD, UU, FF, true, SKIPNA>()), dim3((unsigned)total), dim3(64), sb_lds_pad(), s, args);
    else
      hipLaunchKernelGGL((K::template kernel<XT, YT, TD, UU, FF, false, SKIPNA>()), dim3((unsigned)total), dim3(64), sb_lds_pad(), s, args);
  };
  auto with_fill = [&](auto u_tag) {   // SKIPNA tests the raw values itself (SMM_APPLY_NO_FILL is refused with it)
    if (fill || SKIPNA) go(u_tag, std::true_type());
    else if constexpr (!SKIPNA) go(u_tag, std::false_type());
  };
  if (smm::tuning(SMM_TUNE_SB_LOADS) == 4) with_fill(std::integral_constant<int, 4>());   // tuning: 4 loads per batch instead of 8
  else with_fill(std::integral_constant<int, 8>());
  SMM_LAUNCH_HIP(hipGetLastError());
  return SMM_OK;
}

template <typename XT, typename YT, bool SKIPNA>
int launch_sb(const SbArgs& a, bool fill, unsigned flags, hipStream_t s) {
  return with_sb_tile_rows<YT>([&](auto td) { return launch_sb_any<SbSingle, XT, YT, SKIPNA, decltype(td)::value>(a, fill, flags, s); });
}

// The batch-fastest kernel over the data levels of a group in ONE launch (smm_group_apply_sb).
template <typename XT, typename YT, bool SKIPNA>
int launch_sb_group(const SbGroupArgs& a, bool fill, unsigned flags, hipStream_t s) {
  return with_sb_tile_rows<YT>([&](auto td) { return launch_sb_any<SbGroup, XT, YT, SKIPNA, decltype(td)::value>(a, fill, flags, s); });
}

}  // namespace smm_launch
