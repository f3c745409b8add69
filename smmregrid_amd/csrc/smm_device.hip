// libsmmregrid_hip: HIP kernels (gfx950) and the C ABI declared in
// include/smmregrid_amd.h.
//
// Hot path of jhardenberg/smmregrid rebuilt for MI355X:
//   regrid.py:545-547  fill of non-finite source values with 1e20     (fused, on load)
//   regrid.py:550      tensordot(X(B,S), W(S,D))                      (CSR SpMM, HBM-bound)
//   regrid.py:553-570  dst_imask / dst_frac / >1e19 -> NaN            (fused, on store)
//   regrid.py:387-418  per-level loop, concat, transpose              (one grouped launch)
//   weights.py:47-52   mask pre-compute                               (same kernel, B = 1)
//
// X keeps the reference's native layout: batch rows of S contiguous source
// cells (regrid.py:539-541), so no transpose pass is ever made.  The product
// is memory bound (2 flop per gathered 8-B element): the kernels are built
// around HBM traffic, not MFMA.
//
// Summation order: links of a destination row are accumulated sequentially in
// ascending source index with separate multiply and add (no FMA contraction),
// exactly the order of the CPU oracle (oracle/), so f64 results are bit
// identical to it.
#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <string>
#include <thread>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "smm_internal.h"
#include "smm_built.hpp"
#include "smm_device.hpp"

#pragma clang fp contract(off)

namespace {

thread_local std::string g_last_error;

constexpr bool is_float_dtype(int d) { return d == SMM_F32 || d == SMM_F64; }
constexpr bool is_packed_dtype(int d) { return d == SMM_I16 || d == SMM_U16; }
constexpr bool is_half_dtype(int d) { return d == SMM_F16 || d == SMM_BF16; }
inline size_t dtype_size(int d) { return d == SMM_F64 ? 8 : (d == SMM_F32 ? 4 : 2); }

// The field types and rules of one apply call: filled once at the ABI boundary (apply_entry), then passed down by
// const reference.  has_cf / has_enc: a validated smm_cf_decode_t (make_cf) / smm_cf_encode_t (make_enc) is in cf / enc.
struct CallDesc {
  int x_dtype, y_dtype;
  unsigned flags;
  double area_min;               // remap_area_min
  bool has_cf = false, has_enc = false;
  CfParams cf{};
  int decode_dtype = SMM_F64;    // of a packed X
  CfOutParams enc{};
  bool packed_x() const { return is_packed_dtype(x_dtype); }
  bool half() const { return is_half_dtype(x_dtype) || is_half_dtype(y_dtype); }   // SMM_F16 / SMM_BF16 X or Y
  bool skipna() const { return (flags & SMM_APPLY_SKIPNA) != 0; }
  CallDesc with_flags(unsigned f) const {
    CallDesc c = *this;
    c.flags = f;
    return c;
  }
  // fn(smm_launch::Built<XT, YT, SKIPNA, TILE>()) for the call's types
  template <typename F>
  int dispatch(F&& fn) const {
    return smm_launch::visit_built(x_dtype, y_dtype, decode_dtype, skipna(), fn);
  }
};

// X dtype check shared by the apply paths: float always, packed only with a decode rule (the _cf / _pk entries); with an
// encode rule (the _pk entries) y_dtype is SMM_I16 / SMM_U16, checked by make_enc.  This is the place that words the
// refusals; what it lets through is exactly the built list of smm_built.hpp (static_assert below).
struct Refusal {
  int code;
  const char* msg;
};
constexpr Refusal x_dtype_refusal(int x_dtype, int y_dtype, bool cf, bool enc) {
  if (is_half_dtype(x_dtype) || is_half_dtype(y_dtype)) {
    if (cf || enc) return {SMM_ERR_INVALID, "SMM_F16 / SMM_BF16 take no decode or encode rule: use the plain entries"};
    if (is_half_dtype(x_dtype) ? (y_dtype == SMM_F64 || y_dtype == x_dtype) : is_float_dtype(x_dtype)) return {SMM_OK, nullptr};
    return {SMM_ERR_UNSUPPORTED, "this SMM_F16 / SMM_BF16 pairing is not built: a half field gives SMM_F64 or its own type, "
                                 "a half result takes an SMM_F32 / SMM_F64 field or a field of its own type"};
  }
  if (enc) {
    if (!is_packed_dtype(y_dtype)) return {SMM_ERR_INVALID, "an encode rule needs y_dtype SMM_I16 or SMM_U16"};
    if (is_float_dtype(x_dtype)) return {SMM_OK, nullptr};
    if (!(cf && is_packed_dtype(x_dtype)))
      return {SMM_ERR_UNSUPPORTED, "field dtype must be SMM_F32, SMM_F64 or, with a decode rule, SMM_I16 / SMM_U16"};
    if (x_dtype != y_dtype)
      return {SMM_ERR_UNSUPPORTED, "a packed field produces packed results of its own raw type only"};
    return {SMM_OK, nullptr};
  }
  if (!(is_float_dtype(x_dtype) || (cf && is_packed_dtype(x_dtype))) || !is_float_dtype(y_dtype))
    return {SMM_ERR_UNSUPPORTED, is_packed_dtype(x_dtype)
                                     ? "SMM_I16 / SMM_U16 fields go through the _cf entries (smm_apply_cf, ...)"
                                     : "field dtype must be SMM_F32 or SMM_F64"};
  if (cf && is_packed_dtype(x_dtype) && y_dtype != SMM_F64)
    return {SMM_ERR_UNSUPPORTED, "packed fields produce SMM_F64 results (y_dtype SMM_F32 is not built)"};
  return {SMM_OK, nullptr};
}
inline int check_x_dtype(const CallDesc& c) {
  const Refusal r = x_dtype_refusal(c.x_dtype, c.y_dtype, c.has_cf, c.has_enc);
  return r.code ? fail(r.code, r.msg) : SMM_OK;
}
// A call that carries the rules its dtypes need (a packed X its decode rule, a packed Y its encode rule) is accepted
// exactly when its combination is built.
constexpr bool refusals_match_built() {
  for (int x = SMM_F32; x <= SMM_BF16; ++x)
    for (int y = SMM_F32; y <= SMM_BF16; ++y)
      for (int dd = SMM_F32; dd <= SMM_F64; ++dd)
        if ((x_dtype_refusal(x, y, is_packed_dtype(x), is_packed_dtype(y)).code == SMM_OK) != smm_launch::is_built(x, y, dd))
          return false;
  return true;
}
static_assert(refusals_match_built(), "check_x_dtype and SMM_BUILT (smm_built.hpp) disagree");

}  // namespace

namespace {
// smm_debug_set_tuning: process-wide knobs of tests / tools / benchmarks, 0 = the library's own choice
std::atomic<int> g_tuning[SMM_TUNE_COUNT];
// largest 1-D launch grid (workgroups); smm_debug_set_grid_limit lowers it so that tests reach the split path
std::atomic<int64_t> g_grid_limit{0x7fffffffLL};
// test hook for the pipelines' error path (smm_debug_fail_at_chunk): chunk c of the next host-pipeline
// calls fails; -1 (the default) = off.  Set explicitly by the tests, never read from the environment.
std::atomic<int64_t> g_fail_at_chunk{-1};
// What the host pipelines spent where, summed since the last reset (smm_debug_host_stats).
struct HostStats {
  std::mutex mu;
  double v[SMM_HOST_STAT_COUNT] = {};
} g_host_stats;
}  // namespace

namespace smm {   // declared in smm_launch.hpp (smm_comm.cpp declares fail_msg itself) and smm_device.hpp
int fail_msg(int code, const std::string& msg) {
  g_last_error = msg;
  return code;
}
int tuning(int knob) { return (knob >= 0 && knob < SMM_TUNE_COUNT) ? g_tuning[knob].load(std::memory_order_relaxed) : 0; }
int64_t grid_limit() { return g_grid_limit.load(); }
int64_t test_fail_chunk() { return g_fail_at_chunk.load(std::memory_order_relaxed); }
void add_host_stats(const double* v) {
  std::lock_guard<std::mutex> lock(g_host_stats.mu);
  for (int i = 0; i < SMM_HOST_STAT_COUNT; ++i) g_host_stats.v[i] += v[i];
  g_host_stats.v[SMM_HOST_STAT_THREADS] = (double)smm::staging_threads();
}
}  // namespace smm

namespace {

template <typename T>
int upload(DeviceBuf<T>& buf, const std::vector<T>& h) {   // buf is empty after a failure
  SMM_HIP(buf.upload(h));
  return SMM_OK;
}

int refresh_desc(smm_operator* op) {
  const LevelDesc L = op->desc(op->native_plan());
  if (!op->d_desc.get()) SMM_HIP(op->d_desc.alloc(1));
  SMM_HIP(hipMemcpy(op->d_desc.get(), &L, sizeof(LevelDesc), hipMemcpyHostToDevice));
  return SMM_OK;
}

// Build and upload tile plan `which` of the operator if it does not exist yet (a failed upload: built, not valid, empty).
int ensure_plan(smm_operator* op, int which) {
  std::lock_guard<std::mutex> lock(op->plan_mu);
  smm_operator::TilePlan& pl = op->plan[which];
  if (pl.built) return SMM_OK;
  smm::HostTilePlan hp;
  // LDS / staging-register budget: 64 KiB per 4-wave block, 16 KiB per single-wave block (whatever
  // part of the slice's rows it owns)
  const int64_t budget = which == 0 ? kTileMaxChunks : kTileMaxChunks / kWavesPerBlock;
  smm::build_tile_plan(op->csr, op->sell_shape, shape_rows(which), kChunkElems, budget, hp);
  smm::tighten_tile_plan(op->csr, hp, budget);
  pl.built = true;
  if (!hp.valid) return SMM_OK;
  smm_operator::TilePlan up;   // filled here, moved into the handle once every upload has succeeded
  int rc = SMM_OK;
  if ((rc = upload(up.d_blk_chunk_off, hp.blk_chunk_off)) || (rc = upload(up.d_chunk_src, hp.chunk_src)) ||
      (rc = upload(up.d_lcol, hp.lcol)) || (rc = upload(up.d_blk_direct, hp.blk_direct)))
    return rc;
  up.built = up.valid = true;
  up.max_chunks = hp.max_block_chunks;
  up.total_chunks = hp.total_chunks;
  up.total_lines = hp.total_lines;
  up.reuse = hp.total_chunks * 50 > hp.distinct_chunks * 51;  // > 2 % of lines staged twice
  // at least a tenth of every staged 128-B line is consumed: the lines are the ones a gather would
  // fetch anyway, and staging fetches them coalesced (r3600x1800 -> r360x180 bilinear uses 20 %:
  // tile 0.48 ms, SELL 0.64 ms; HEALPix-nested source, nearest neighbour, 14 %: 1.87 vs 2.10 ms;
  // r3600x1800 nearest neighbour, 10 %: equal)
  up.preferred = hp.total_distinct * 10 >= hp.total_lines * 16;
  pl = std::move(up);
  return SMM_OK;
}

// the launch templates live in smm_launch.hpp; their instantiations (SMM_BUILT, smm_built.hpp) are compiled in
// smm_launch_inst.hip and only declared here
using smm_launch::launch_sell;
using smm_launch::launch_tile;
using smm_launch::launch_sb;
using smm_launch::launch_sb_group;

// Device copy of the canonical CSR (+ packed column ranks) for the batch-fastest kernel.
int ensure_sb(smm_operator* op) {
  std::lock_guard<std::mutex> lock(op->plan_mu);
  if (op->sb_ready) return SMM_OK;
  const smm::HostCsr& c = op->csr;
  std::vector<int32_t> rank((size_t)std::max<int64_t>(c.n_src, 1), -1), colp((size_t)c.nnz);
  for (int32_t s : c.col) rank[(size_t)s] = 0;
  int32_t r = 0;
  for (int64_t s = 0; s < c.n_src; ++s)
    if (rank[(size_t)s] == 0) rank[(size_t)s] = r++;
  for (int64_t i = 0; i < c.nnz; ++i) colp[(size_t)i] = rank[(size_t)c.col[(size_t)i]];
  op->h_used.clear();
  op->h_used.reserve((size_t)c.n_used_src);
  for (int64_t s = 0; s < c.n_src; ++s)
    if (rank[(size_t)s] >= 0) op->h_used.push_back((int32_t)s);
  DeviceBuf<int64_t> rowptr;
  DeviceBuf<int32_t> col, colp_d;
  DeviceBuf<double> val;
  int rc = SMM_OK;
  if ((rc = upload(rowptr, c.rowptr)) || (rc = upload(col, c.col)) || (rc = upload(colp_d, colp)) ||
      (rc = upload(val, c.val)))
    return rc;   // the handle holds none of the four
  op->d_csr_rowptr = std::move(rowptr);
  op->d_csr_col = std::move(col);
  op->d_csr_colp = std::move(colp_d);
  op->d_csr_val = std::move(val);
  op->sb_ready = true;
  return SMM_OK;
}

struct LaunchInfo {
  bool tile = false, big_operator = false, dma = false;
  int j_per_block = 0, rows_per_step = 1, rows_per_block = 0;
  int64_t n_jtiles = 0, n_blocks = 0, lds_bytes = 0;
};

// What run_apply launches: the level descriptors and the tile plan of one operator or of a group
struct ApplyTarget {
  const LevelDesc* d_descs;
  int64_t n_src, n_dst;
  int tile_which;
  bool tile_ok, tile_preferred;
  int tile_flags;   // bit 0: some staged lines are shared by several blocks
  int64_t tile_max_chunks, max_row_nnz;
};
ApplyTarget target_of(const smm_operator* op) {
  const int pw = op->native_plan();
  const smm_operator::TilePlan& pl = op->plan[pw];
  return {op->d_desc.get(), op->csr.n_src, op->csr.n_dst, pw, pl.valid, pl.preferred, pl.reuse ? 1 : 0, pl.max_chunks,
          op->csr.max_row_nnz};
}
ApplyTarget target_of(const smm_group* g) {
  return {g->d_descs.get(), g->ops[0]->csr.n_src, g->ops[0]->csr.n_dst, g->tile_which, g->tile_valid, g->tile_preferred,
          g->tile_reuse ? 1 : 0, g->tile_max_chunks, g->max_row_nnz};
}

// Common launch path for a single operator or a group.  info_only: nothing is launched, *info_only gets the geometry.
int run_apply(const ApplyTarget& t, const int32_t* d_lev_map, const uint8_t* d_lev_masked, const void* x, int64_t xs_o,
              int64_t xs_l, int64_t xs_i, void* y, int64_t ys_o, int64_t ys_l, int64_t ys_i, int64_t n_outer,
              int64_t n_lev, int64_t n_inner, const CallDesc& call, hipStream_t s, LaunchInfo* info_only = nullptr) {
  const int64_t n_src = t.n_src, n_dst = t.n_dst, tile_max_chunks = t.tile_max_chunks, max_row_nnz = t.max_row_nnz;
  const int tile_which = t.tile_which;
  const unsigned flags = call.flags;
  const double area_min = call.area_min;
  if (n_outer < 0 || n_lev < 0 || n_inner < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (n_outer == 0 || n_lev == 0 || n_inner == 0 || n_dst == 0) return SMM_OK;
  if (!info_only && (!x || !y)) return fail(SMM_ERR_INVALID, "null field pointer");
  const bool packed = call.packed_x(), enc = call.has_enc, half = call.half();
  if (int drc = check_x_dtype(call)) return drc;
  if (int arc = check_area_min(area_min)) return arc;

  ApplyArgs a{};
  a.descs = t.d_descs;
  a.lev_map = d_lev_map;
  a.lev_masked = d_lev_masked;
  a.x = x;
  a.y = y;
  a.xs_o = xs_o;
  a.xs_l = xs_l;
  a.xs_i = xs_i;
  a.ys_o = ys_o;
  a.ys_l = ys_l;
  a.ys_i = ys_i;
  a.n_j = n_outer * n_inner;
  a.n_inner = n_inner;
  a.n_src = n_src;
  a.n_dst = n_dst;
  a.n_dblocks = ((n_dst + 63) / 64 + kWavesPerBlock - 1) / kWavesPerBlock;  // SELL: 4 slices per workgroup
  a.area_min = area_min;
  a.masked = (flags & SMM_APPLY_MASKED) ? 1 : 0;
  const bool fill = !(flags & SMM_APPLY_NO_FILL);
  if (packed) a.cf = call.cf;
  if (enc) a.cfo = call.enc;

  const size_t xsz = dtype_size(call.x_dtype);
  bool use_tile = false;
  // SMM_APPLY_SKIPNA: tile forms without a skipna variant (split rows, rows streamed from L2) run kernel A instead
  const bool tile_skipna_ok = !(flags & SMM_APPLY_SKIPNA) ||
                              smm_launch::tile_has_skipna(tile_which, tile_which >= 2 ? tile_which - 1 : 0, max_row_nnz);
  if (packed || enc || half) {
    // the LDS tile kernel stages 16-B pieces of 4- or 8-byte elements: packed X runs kernel A whatever the plan, and
    // so do packed results and half-precision fields and results (the tile kernel is not built for them either)
    if (flags & SMM_APPLY_KERNEL_TILE)
      return fail(SMM_ERR_UNSUPPORTED, half ? "the LDS tile kernel is not built for half-precision fields or results (SMM_F16 / SMM_BF16)"
                                            : "the LDS tile kernel is not built for packed fields or results (SMM_I16 / SMM_U16)");
    if (!info_only && ((uintptr_t)x % xsz) != 0) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    if (!info_only && (enc || is_half_dtype(call.y_dtype)) && ((uintptr_t)y % 2) != 0)
      return fail(SMM_ERR_INVALID, "result pointer is not element aligned");
  } else if (flags & SMM_APPLY_KERNEL_TILE) {
    if (!t.tile_ok) return fail(SMM_ERR_UNSUPPORTED, "operator has no LDS tile plan");
    if (!tile_skipna_ok)
      return fail(SMM_ERR_UNSUPPORTED, "SMM_APPLY_SKIPNA: the planned tile form (split or streamed rows) has no skipna variant");
    use_tile = true;
  } else if (!(flags & SMM_APPLY_KERNEL_SELL)) {
    use_tile = t.tile_ok && t.tile_preferred && tile_skipna_ok;
  }
  // The staging loads are 16 B wide but only need element alignment (unaligned 16-B global loads
  // are legal on gfx950; rows of odd length still run ~10 % faster than the SELL kernel).
  if (use_tile && ((uintptr_t)x % xsz) != 0) {
    if (flags & SMM_APPLY_KERNEL_TILE) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    use_tile = false;
  }

  if (use_tile) {
    const int64_t rows = shape_rows(tile_which);          // destination rows per block of the tile plan
    a.n_dblocks = (n_dst + rows - 1) / rows;
    a.sub_shift = tile_which >= 2 ? tile_which - 1 : 0;   // block = 1 / 2^sub_shift of a slice
  }
  if (info_only) {
    info_only->tile = use_tile;
    if (use_tile) {
      const smm_launch::TileLaunchCfg c =
          smm_launch::tile_launch_cfg(a, n_lev, tile_which, tile_max_chunks, max_row_nnz, flags, xsz);
      info_only->j_per_block = c.j_per_block;
      info_only->n_jtiles = c.n_jtiles;
      info_only->n_blocks = c.total;
      info_only->rows_per_step = c.rows;
      info_only->lds_bytes = (int64_t)c.lds;
      info_only->big_operator = c.big_operator;
      info_only->dma = c.dma;
      info_only->rows_per_block = (int)shape_rows(tile_which);
    } else {
      const int bt = smm_launch::sell_batch_rows(a.n_j);
      info_only->j_per_block = bt;
      info_only->n_jtiles = (a.n_j + bt - 1) / bt;
      info_only->n_blocks = a.n_dblocks * info_only->n_jtiles * n_lev;
      info_only->rows_per_step = bt;
      info_only->rows_per_block = 256;
    }
    return SMM_OK;
  }
  // One launch when the grid fits (always, short of ~2^31 workgroups); else the batch is cut into parts
  // (smm::split_batch) that are launched one after the other on the same stream.
  auto blocks_for = [&](int64_t n_o, int64_t n_i) -> int64_t {
    ApplyArgs t = a;
    t.n_j = n_o * n_i;
    t.n_inner = n_i;
    if (use_tile)
      return smm_launch::tile_launch_cfg(t, n_lev, tile_which, tile_max_chunks, max_row_nnz, flags, xsz).total;
    const int bt = smm_launch::sell_batch_rows(t.n_j);
    return t.n_dblocks * ((t.n_j + bt - 1) / bt) * n_lev;
  };
  const size_t ysz = dtype_size(call.y_dtype);
  auto launch_part = [&](int64_t o0, int64_t n_o, int64_t i0, int64_t n_i) -> int {
    ApplyArgs p = a;
    p.x = (const char*)x + (o0 * xs_o + i0 * xs_i) * (int64_t)xsz;
    p.y = (char*)y + (o0 * ys_o + i0 * ys_i) * (int64_t)ysz;
    p.n_j = n_o * n_i;
    p.n_inner = n_i;
    return call.dispatch([&](auto b) -> int {
      using B = decltype(b);
      if constexpr (B::tile)   // float pairs: the only ones use_tile can be set for
        if (use_tile)
          return launch_tile<typename B::XT, typename B::YT, B::skipna>(p, n_lev, tile_which, tile_max_chunks, max_row_nnz,
                                                                        t.tile_flags, fill, flags, s);
      return launch_sell<typename B::XT, typename B::YT, B::skipna>(p, n_lev, fill, flags, s);
    });
  };
  const int rc = smm::split_batch(0, n_outer, 0, n_inner, grid_limit(), blocks_for, launch_part);
  if (rc == -1)
    return fail(SMM_ERR_INVALID, "one batch row alone needs a launch grid beyond " + std::to_string(grid_limit()) +
                                     " workgroups (destination blocks x levels)");
  return rc;
}

}  // namespace

namespace {

int host_pack(void* out, const void* x, size_t xsz, int64_t n_inner, int64_t stride_o, int64_t stride_i,
              const std::vector<int32_t>& used, int64_t rows) {
  return stage_status(smm::host_pack(out, x, xsz, n_inner, stride_o, stride_i, used.data(), (int64_t)used.size(), rows,
                                     smm::tuning(SMM_TUNE_HOST_PACK_STORES) != 1),
                      "host pack");
}
int host_pack(void* out, const void* x, size_t xsz, int64_t ldx, const std::vector<int32_t>& used, int64_t rows) {
  return host_pack(out, x, xsz, std::max<int64_t>(rows, 1), 0, ldx, used, rows);
}

}  // namespace

// ------------------------------------------------------------------ C ABI

extern "C" {

int smm_abi_version(void) { return SMM_ABI_VERSION; }
const char* smm_last_error(void) { return g_last_error.c_str(); }

int smm_device_count(int* count) {
  if (!count) return fail(SMM_ERR_INVALID, "null count");
  *count = 0;
  int n = 0;
  hipError_t e = hipGetDeviceCount(&n);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return fail(SMM_ERR_NO_DEVICE, std::string("hipGetDeviceCount: ") + hipGetErrorString(e));
  }
  *count = n;
  return SMM_OK;
}
int smm_set_device(int device) {
  SMM_HIP(hipSetDevice(device));
  return SMM_OK;
}
int smm_get_device(int* device) {
  if (!device) return fail(SMM_ERR_INVALID, "null device");
  SMM_HIP(hipGetDevice(device));
  return SMM_OK;
}
int smm_device_name(int device, char* buf, size_t buflen) {
  if (!buf || buflen == 0) return fail(SMM_ERR_INVALID, "null buffer");
  hipDeviceProp_t p;
  SMM_HIP(hipGetDeviceProperties(&p, device));
  snprintf(buf, buflen, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
  return SMM_OK;
}
int smm_mem_info(size_t* free_bytes, size_t* total_bytes) {
  size_t f = 0, t = 0;
  SMM_HIP(hipMemGetInfo(&f, &t));
  if (free_bytes) *free_bytes = f;
  if (total_bytes) *total_bytes = t;
  return SMM_OK;
}
int smm_malloc(void** dptr, size_t bytes) {
  if (!dptr) return fail(SMM_ERR_INVALID, "null dptr");
  *dptr = nullptr;
  SMM_HIP(hipMalloc(dptr, bytes ? bytes : 1));
  return SMM_OK;
}
int smm_free(void* dptr) {
  if (dptr) SMM_HIP(hipFree(dptr));
  return SMM_OK;
}
int smm_host_alloc(void** hptr, size_t bytes) {
  if (!hptr) return fail(SMM_ERR_INVALID, "null hptr");
  *hptr = nullptr;
  SMM_HIP(hipHostMalloc(hptr, bytes ? bytes : 1, hipHostMallocDefault));
  return SMM_OK;
}
int smm_host_free(void* hptr) {
  if (hptr) SMM_HIP(hipHostFree(hptr));
  return SMM_OK;
}
int smm_host_memcpy(void* dst_host, const void* src_host, size_t bytes) {
  if (bytes == 0) return SMM_OK;
  if (!dst_host || !src_host) return fail(SMM_ERR_INVALID, "null host pointer");
  return host_copy(dst_host, src_host, bytes);
}
int smm_memcpy_h2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return SMM_OK;
  if (stream)
    SMM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, (hipStream_t)stream));
  else
    SMM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyHostToDevice));
  return SMM_OK;
}
int smm_memcpy_d2h(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return SMM_OK;
  if (stream)
    SMM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToHost, (hipStream_t)stream));
  else
    SMM_HIP(hipMemcpy(dst, src, bytes, hipMemcpyDeviceToHost));
  return SMM_OK;
}
int smm_memcpy_d2d(void* dst, const void* src, size_t bytes, void* stream) {
  if (bytes == 0) return SMM_OK;
  SMM_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
  return SMM_OK;
}
int smm_memcpy2d_h2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                     void* stream) {
  if (width == 0 || height == 0) return SMM_OK;
  if (dpitch < width || spitch < width) return fail(SMM_ERR_INVALID, "pitch smaller than the row width");
  if (stream)
    SMM_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice, (hipStream_t)stream));
  else
    SMM_HIP(hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyHostToDevice));
  return SMM_OK;
}
int smm_memcpy2d_d2h(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, size_t height,
                     void* stream) {
  if (width == 0 || height == 0) return SMM_OK;
  if (dpitch < width || spitch < width) return fail(SMM_ERR_INVALID, "pitch smaller than the row width");
  if (stream)
    SMM_HIP(hipMemcpy2DAsync(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost, (hipStream_t)stream));
  else
    SMM_HIP(hipMemcpy2D(dst, dpitch, src, spitch, width, height, hipMemcpyDeviceToHost));
  return SMM_OK;
}
int smm_debug_set_grid_limit(int64_t max_blocks) {
  if (max_blocks < 0) return fail(SMM_ERR_INVALID, "negative grid limit");
  g_grid_limit.store(max_blocks == 0 || max_blocks > 0x7fffffffLL ? 0x7fffffffLL : max_blocks);
  return SMM_OK;
}

int smm_debug_set_tuning(int knob, int value, int* previous) {
  if (knob < 0 || knob >= SMM_TUNE_COUNT) return fail(SMM_ERR_INVALID, "unknown tuning knob " + std::to_string(knob));
  const int prev = g_tuning[knob].exchange(value);
  if (previous) *previous = prev;
  return SMM_OK;
}

int smm_set_host_threads(int n, int* previous) {
  if (n < 0) return fail(SMM_ERR_INVALID, "negative thread count");
  const int prev = smm::set_host_threads(n);
  if (previous) *previous = prev;
  return SMM_OK;
}

int smm_debug_host_stats(double* out, int n, int reset) {
  if (n < 0 || (n > 0 && !out)) return fail(SMM_ERR_INVALID, "bad stats buffer");
  std::lock_guard<std::mutex> lock(g_host_stats.mu);
  for (int i = 0; i < n; ++i) out[i] = i < SMM_HOST_STAT_COUNT ? g_host_stats.v[i] : 0.0;
  if (reset)
    for (double& v : g_host_stats.v) v = 0.0;
  return SMM_OK;
}

int smm_debug_staging_faults(int no_threads, int64_t throw_in_task) {
  smm::debug_pool_faults(no_threads != 0, throw_in_task < 0 ? -1 : throw_in_task);
  return SMM_OK;
}

int smm_debug_fail_at_chunk(int64_t chunk) {
  g_fail_at_chunk.store(chunk < 0 ? -1 : chunk, std::memory_order_relaxed);
  return SMM_OK;
}
int smm_memset(void* dst, int value, size_t bytes, void* stream) {
  if (bytes == 0) return SMM_OK;
  SMM_HIP(hipMemsetAsync(dst, value, bytes, (hipStream_t)stream));
  return SMM_OK;
}
int smm_stream_create(void** stream) {
  if (!stream) return fail(SMM_ERR_INVALID, "null stream");
  hipStream_t s;
  SMM_HIP(hipStreamCreateWithFlags(&s, hipStreamNonBlocking));
  *stream = (void*)s;
  return SMM_OK;
}
int smm_stream_destroy(void* stream) {
  if (stream) SMM_HIP(hipStreamDestroy((hipStream_t)stream));
  return SMM_OK;
}
int smm_stream_sync(void* stream) {
  SMM_HIP(hipStreamSynchronize((hipStream_t)stream));
  return SMM_OK;
}
int smm_device_sync(void) {
  SMM_HIP(hipDeviceSynchronize());
  return SMM_OK;
}
int smm_event_create(void** event) {
  if (!event) return fail(SMM_ERR_INVALID, "null event");
  hipEvent_t e;
  SMM_HIP(hipEventCreate(&e));
  *event = (void*)e;
  return SMM_OK;
}
int smm_event_destroy(void* event) {
  if (event) SMM_HIP(hipEventDestroy((hipEvent_t)event));
  return SMM_OK;
}
int smm_event_record(void* event, void* stream) {
  SMM_HIP(hipEventRecord((hipEvent_t)event, (hipStream_t)stream));
  return SMM_OK;
}
int smm_event_sync(void* event) {
  SMM_HIP(hipEventSynchronize((hipEvent_t)event));
  return SMM_OK;
}
int smm_stream_wait_event(void* stream, void* event) {
  SMM_HIP(hipStreamWaitEvent((hipStream_t)stream, (hipEvent_t)event, 0));
  return SMM_OK;
}
int smm_event_elapsed_ms(void* start, void* stop, float* ms) {
  if (!ms) return fail(SMM_ERR_INVALID, "null ms");
  SMM_HIP(hipEventElapsedTime(ms, (hipEvent_t)start, (hipEvent_t)stop));
  return SMM_OK;
}

int smm_fill_random(void* dst, int dtype, int64_t n, uint64_t seed, double mean, double sigma,
                    void* stream) {
  if (n <= 0) return SMM_OK;
  if (!dst) return fail(SMM_ERR_INVALID, "null destination");
  const unsigned blocks = (unsigned)std::min<int64_t>((n + 255) / 256, 256 * 32);
  if (dtype == SMM_F64)
    hipLaunchKernelGGL(smm_fill_random_kernel<double>, dim3(blocks), dim3(256), 0,
                       (hipStream_t)stream, (double*)dst, n, seed, mean, sigma);
  else if (dtype == SMM_F32)
    hipLaunchKernelGGL(smm_fill_random_kernel<float>, dim3(blocks), dim3(256), 0,
                       (hipStream_t)stream, (float*)dst, n, seed, mean, sigma);
  else
    return fail(SMM_ERR_UNSUPPORTED, "dtype must be SMM_F32 or SMM_F64");
  SMM_HIP(hipGetLastError());
  return SMM_OK;
}

// ---- operators

// Shared by the two constructors: `fill_csr` builds op->csr (false + err on invalid input).
extern "C++" {
template <typename F>
static int create_operator(int device, smm_operator_t* out, F fill_csr, unsigned options = 0u,
                           std::vector<std::vector<double>>* extra_cols = nullptr) {
  if (!out) return fail(SMM_ERR_INVALID, "null out handle");
  *out = nullptr;
  if (options & ~(unsigned)SMM_CREATE_PRUNE_ZEROS) return fail(SMM_ERR_INVALID, "unknown create option bits");
  int ndev = 0;
  {
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev == 0) {
      (void)hipGetLastError();
      return fail(SMM_ERR_NO_DEVICE,
                  "no HIP device: libsmmregrid_hip has no CPU fallback (hipGetDeviceCount: " +
                      std::string(hipGetErrorString(e)) + ")");
    }
  }
  if (device < 0 || device >= ndev)
    return fail(SMM_ERR_NO_DEVICE, "device ordinal " + std::to_string(device) + " out of range");

  std::unique_ptr<smm_operator> owner(new (std::nothrow) smm_operator());   // freed on every early return and throw
  if (!owner) return fail(SMM_ERR_ALLOC, "out of host memory");
  smm_operator* op = owner.get();
  op->device = device;
  try {
    std::string err;
    if (!fill_csr(op->csr, err)) return fail(SMM_ERR_INVALID, err);
    if (extra_cols) {   // smm_operator_create_cols: fill_csr left the weight columns 1.. there
      op->csr_xval = std::move(*extra_cols);
      op->n_cols = 1 + (int)op->csr_xval.size();
    }
    if (options & SMM_CREATE_PRUNE_ZEROS) op->pruned_links = smm::prune_zero_links_cols(op->csr, op->csr_xval);
    const smm::HostCsr& kc = op->csr;
    smm::HostSell sell;
    smm::build_sell(kc, sell);
    std::vector<double> xval;
    if (!op->csr_xval.empty()) smm::build_sell_cols(kc, sell, op->csr_xval, xval);

    DeviceGuard guard(device);
    if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select device " + std::to_string(device));
    op->n_slices = sell.n_slices;
    op->n_slots = sell.n_slots;
    int rc = SMM_OK;
    if ((rc = upload(op->d_slice_off, sell.slice_off)) || (rc = upload(op->d_col, sell.col)) ||
        (rc = upload(op->d_val, sell.val)) || (rc = upload(op->d_rowlen, sell.rowlen)))
      return rc;
    if (!xval.empty() && (rc = upload(op->d_xval, xval))) return rc;
    op->sell_shape.n_slices = sell.n_slices;
    op->sell_shape.n_slots = sell.n_slots;
    op->sell_shape.slice_off = std::move(sell.slice_off);
    op->sell_shape.rowlen = std::move(sell.rowlen);
    // own block shape: 256 rows for rows of <= 16 links; else one slice, or the largest part of a
    // slice whose footprint fits the LDS budget and is used well enough (plan valid and preferred)
    op->native = kc.max_row_nnz > 16 ? 1 : 0;
    if ((rc = ensure_plan(op, op->native))) return rc;
    if (op->native == 1) {
      // rows beyond 48 links: start at the shape whose lane groups can keep the whole row in
      // registers (split rows) -- streaming the links from L2 is ~2x slower; else from one slice
      int w_first = 1;
      while (w_first < kNumShapes - 1 && kc.max_row_nnz > 48ll << (w_first - 1)) ++w_first;
      bool found = false;
      for (int pass = 0; pass < 2 && !found; ++pass) {
        for (int w = pass == 0 ? w_first : 1; w < (pass == 0 ? kNumShapes : w_first) && !found; ++w) {
          if ((rc = ensure_plan(op, w))) return rc;
          if (op->plan[w].valid && op->plan[w].preferred) {
            op->native = w;
            found = true;
          }
        }
      }
      for (int w = 1; w < kNumShapes; ++w)   // plans tried on the way are rebuilt on demand
        if (w != op->native) op->plan[w] = smm_operator::TilePlan();
    }
    if ((rc = refresh_desc(op))) return rc;
  } catch (const std::bad_alloc&) {
    return fail(SMM_ERR_ALLOC, "out of host memory while building the operator");
  } catch (const std::exception& e) {   // nothing may cross the extern "C" boundary
    return fail(SMM_ERR_INTERNAL, std::string("operator build failed: ") + e.what());
  } catch (...) {
    return fail(SMM_ERR_INTERNAL, "operator build failed");
  }
  *out = owner.release();
  return SMM_OK;
}
}  // extern "C++"

int smm_operator_create(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src_addr_1based,
                        const int32_t* dst_addr_1based, const double* w, int device,
                        smm_operator_t* out) {
  return create_operator(device, out, [&](smm::HostCsr& csr, std::string& err) {
    return smm::build_csr(n_src, n_dst, nnz, src_addr_1based, dst_addr_1based, w, csr, err);
  });
}

int smm_operator_create_opt(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src_addr_1based,
                            const int32_t* dst_addr_1based, const double* w, unsigned options, int device,
                            smm_operator_t* out) {
  return create_operator(device, out, [&](smm::HostCsr& csr, std::string& err) {
    return smm::build_csr(n_src, n_dst, nnz, src_addr_1based, dst_addr_1based, w, csr, err);
  }, options);
}

int smm_operator_create_cols(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src_addr_1based,
                             const int32_t* dst_addr_1based, const double* w, int n_cols, unsigned options, int device,
                             smm_operator_t* out) {
  std::vector<std::vector<double>> extra;
  return guarded([&]() -> int {
    return create_operator(device, out, [&](smm::HostCsr& csr, std::string& err) {
      return smm::build_csr_cols(n_src, n_dst, nnz, src_addr_1based, dst_addr_1based, w, n_cols, csr, extra, err);
    }, options, &extra);
  });
}

int smm_operator_cols(smm_operator_t op, int* n_cols) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_cols) *n_cols = op->n_cols;
  return SMM_OK;
}

int smm_operator_export_cols(smm_operator_t op, double* val) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (!val && op->csr.nnz > 0) return fail(SMM_ERR_INVALID, "null output");
  const size_t K = (size_t)op->n_cols;
  for (int64_t p = 0; p < op->csr.nnz; ++p) {
    val[(size_t)p * K] = op->csr.val[(size_t)p];
    for (size_t k = 1; k < K; ++k) val[(size_t)p * K + k] = op->csr_xval[k - 1][(size_t)p];
  }
  return SMM_OK;
}

int smm_operator_create_csr(int64_t n_src, int64_t n_dst, const int64_t* rowptr, const int32_t* col,
                            const double* val, int device, smm_operator_t* out) {
  return create_operator(device, out, [&](smm::HostCsr& csr, std::string& err) {
    return smm::adopt_csr(n_src, n_dst, rowptr, col, val, csr, err);
  });
}

int smm_operator_destroy(smm_operator_t op) {
  if (!op) return SMM_OK;
  if (op->group_refs.load() > 0)
    return fail(SMM_ERR_INVALID, "operator still belongs to a group: destroy the group first");
  DeviceGuard guard(op->device);
  delete op;   // also when the device could not be selected
  return SMM_OK;
}

int smm_operator_info(smm_operator_t op, int64_t* n_src, int64_t* n_dst, int64_t* nnz,
                      int64_t* n_used_src, int64_t* max_row_nnz) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_src) *n_src = op->csr.n_src;
  if (n_dst) *n_dst = op->csr.n_dst;
  if (nnz) *nnz = op->csr.nnz;
  if (n_used_src) *n_used_src = op->csr.n_used_src;
  if (max_row_nnz) *max_row_nnz = op->csr.max_row_nnz;
  return SMM_OK;
}

static int smm_operator_export_csr_impl(smm_operator_t op, int64_t* rowptr, int32_t* col, double* val) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (rowptr) memcpy(rowptr, op->csr.rowptr.data(), op->csr.rowptr.size() * sizeof(int64_t));
  if (col && op->csr.nnz) memcpy(col, op->csr.col.data(), (size_t)op->csr.nnz * sizeof(int32_t));
  if (val && op->csr.nnz) memcpy(val, op->csr.val.data(), (size_t)op->csr.nnz * sizeof(double));
  return SMM_OK;
}

static int smm_operator_set_epilogue_impl(smm_operator_t op, const int32_t* dst_imask, const double* dst_frac) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  // a group's level descriptors hold this operator's imask / frac device pointers
  if (op->group_refs.load() > 0)
    return fail(SMM_ERR_INVALID,
                "operator belongs to a group: set the epilogue vectors before smm_group_create");
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  const size_t n = (size_t)op->csr.n_dst;
  // upload the new vectors first: on failure the operator keeps its old state untouched.  The two locals hold the new
  // vectors, after the swap the old ones, and free whichever pair the operator does not keep (imask, then frac)
  DeviceBuf<double> frac;
  DeviceBuf<uint8_t> imask;
  if (dst_imask) {
    std::vector<uint8_t> m(n);
    for (size_t i = 0; i < n; ++i) m[i] = dst_imask[i] != 0;  // .astype(bool), regrid.py:557
    if (int rc = upload(imask, m)) return rc;
  }
  if (dst_frac) {
    std::vector<double> f(dst_frac, dst_frac + n);
    if (int rc = upload(frac, f)) return rc;
  }
  std::swap(op->d_imask, imask);
  std::swap(op->d_frac, frac);
  int rc = refresh_desc(op);
  if (rc) {  // the device descriptor still names the old vectors: keep them
    std::swap(op->d_imask, imask);
    std::swap(op->d_frac, frac);
  }
  return rc;
}

static int smm_operator_plan_info_impl(smm_operator_t op, int* kernel_kind, int64_t* lds_bytes,
                           int64_t* staged_src_elems) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  const smm_operator::TilePlan& pl = op->plan[op->native_plan()];
  if (kernel_kind)
    *kernel_kind = (pl.valid ? 1 : 0) | (pl.preferred ? 2 : 0) | (shape_rows(op->native_plan()) << 8);
  if (lds_bytes) *lds_bytes = pl.valid ? pl.max_chunks * kChunkElems * 8 : 0;
  if (staged_src_elems) *staged_src_elems = pl.valid ? pl.total_lines * 16 : 0;   // whole 128-B lines of f64
  return SMM_OK;
}

static int smm_apply_impl(smm_operator_t op, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t n_batch,
                          void* stream, const CallDesc& call) {
  if (int frc = check_flags(call.flags)) return frc;
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_batch > 0 && (ldx < op->csr.n_src || ldy < op->csr.n_dst))
    return fail(SMM_ERR_INVALID, "ldx/ldy smaller than the grid size");
  if (int erc = check_epilogue(op, call.flags & SMM_APPLY_MASKED, call.area_min, "the operator")) return erc;
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  return run_apply(target_of(op), nullptr, nullptr, x, ldx, 0, 0, y, ldy, 0, 0, n_batch, 1, 1, call, (hipStream_t)stream);
}

static int smm_operator_prepare_sb_impl(smm_operator_t op) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  return ensure_sb(op);
}

static int smm_operator_used_sources_impl(smm_operator_t op, int32_t* used) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (!used && op->csr.n_used_src > 0) return fail(SMM_ERR_INVALID, "null output");
  std::vector<uint8_t> seen((size_t)std::max<int64_t>(op->csr.n_src, 1), 0);
  for (int32_t s : op->csr.col) seen[(size_t)s] = 1;
  int64_t k = 0;
  for (int64_t s = 0; s < op->csr.n_src; ++s)
    if (seen[(size_t)s]) used[k++] = (int32_t)s;
  return SMM_OK;
}

static int smm_apply_sb_impl(smm_operator_t op, const void* x, int64_t ldx, void* y, int64_t ldy, int64_t n_batch,
                             void* stream, const CallDesc& call) {
  const unsigned flags = call.flags;
  const double remap_area_min = call.area_min;
  if (int frc = check_flags(flags)) return frc;
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (n_batch == 0 || op->csr.n_dst == 0) return SMM_OK;
  if (!x || !y) return fail(SMM_ERR_INVALID, "null field pointer");
  if (int drc = check_x_dtype(call)) return drc;
  if (ldx < n_batch || ldy < ((flags & SMM_APPLY_SB_Y_SB) ? n_batch : op->csr.n_dst))
    return fail(SMM_ERR_INVALID, "ldx smaller than the batch or ldy smaller than a row of Y");
  if (int arc = check_area_min(remap_area_min)) return arc;
  if (int erc = check_epilogue(op, flags & SMM_APPLY_MASKED, remap_area_min, "the operator")) return erc;
  const size_t xsz = dtype_size(call.x_dtype), ysz = dtype_size(call.y_dtype);
  if ((uintptr_t)x % xsz || (uintptr_t)y % ysz) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  int rc = ensure_sb(op);   // first call uploads the CSR (smm_operator_prepare_sb does it ahead of time)
  if (rc) return rc;
  SbArgs a{};
  a.rowptr = op->d_csr_rowptr.get();
  a.col = (flags & SMM_APPLY_SB_PACKED) ? op->d_csr_colp.get() : op->d_csr_col.get();
  a.val = op->d_csr_val.get();
  a.imask = op->d_imask.get();
  a.frac = op->d_frac.get();
  a.x = x;
  a.y = y;
  a.ldx = ldx;
  a.ldy = ldy;
  a.n_batch = n_batch;
  a.n_dst = op->csr.n_dst;
  a.area_min = remap_area_min;
  a.masked = (flags & SMM_APPLY_MASKED) ? 1 : 0;
  if (call.packed_x()) a.cf = call.cf;
  if (call.has_enc) a.cfo = call.enc;
  const bool fill = !(flags & SMM_APPLY_NO_FILL);
  hipStream_t s = (hipStream_t)stream;
  // grid = destination tiles x batch tiles of 128 entries: beyond the limit the batch is cut into runs of
  // whole batch tiles, launched one after the other
  const int64_t td = smm_launch::sb_tile_rows(ysz);
  const int64_t n_dtiles = (a.n_dst + td - 1) / td;
  const int64_t limit = grid_limit();
  if (n_dtiles > limit)
    return fail(SMM_ERR_INVALID, "one batch tile alone needs a launch grid beyond " + std::to_string(limit) + " workgroups");
  const int64_t part = std::max<int64_t>(1, limit / n_dtiles) * 128;
  for (int64_t b0 = 0; b0 < n_batch; b0 += part) {
    a.x = (const char*)x + b0 * (int64_t)xsz;
    a.y = (char*)y + ((flags & SMM_APPLY_SB_Y_SB) ? b0 : b0 * ldy) * (int64_t)ysz;
    a.n_batch = std::min(part, n_batch - b0);
    rc = call.dispatch([&](auto b) {
      using B = decltype(b);
      return launch_sb<typename B::XT, typename B::YT, B::skipna>(a, fill, flags, s);
    });
    if (rc) return rc;
  }
  return SMM_OK;
}

// ---- host-buffer path: chunked, double-buffered H2D -> kernel -> D2H pipeline

static int smm_apply_host_impl(smm_operator_t op, const void* x_host, int64_t ldx, void* y_host, int64_t ldy,
                               int64_t n_batch, int64_t chunk_rows, const CallDesc& call) {
  const int x_dtype = call.x_dtype, y_dtype = call.y_dtype;
  const unsigned flags = call.flags;
  const bool enc = call.has_enc;
  if (int frc = check_flags(flags)) return frc;
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (n_batch == 0 || op->csr.n_dst == 0) return SMM_OK;
  if (!x_host || !y_host) return fail(SMM_ERR_INVALID, "null field pointer");
  if (int drc = check_x_dtype(call)) return drc;
  if ((uintptr_t)x_host % dtype_size(x_dtype)) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
  if ((enc || is_half_dtype(y_dtype)) && (uintptr_t)y_host % 2) return fail(SMM_ERR_INVALID, "result pointer is not element aligned");
  const int64_t S = op->csr.n_src, D = op->csr.n_dst;
  if (ldx < S || ldy < D) return fail(SMM_ERR_INVALID, "ldx/ldy smaller than the grid size");
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");

  // packed X is staged, packed and shipped raw: 2 B per cell; a packed Y (enc) comes back, is staged and copied out raw too;
  // half-precision X and Y travel as their 2-byte elements the same way
  const size_t xsz = dtype_size(x_dtype), ysz = dtype_size(y_dtype);
  const size_t xrow = (size_t)ldx * xsz, yrow = (size_t)ldy * ysz;   // host row pitches
  // device rows start on 128-B lines: the tile plan stages whole lines of a row, and a row that
  // starts mid-line makes every staged run of chunks straddle one line more (config 3's 1442x1021
  // source: +17 % fetched bytes when its rows are packed back to back)
  const size_t xrow_d = (((size_t)S * xsz + 127) / 128) * 128;
  const int64_t ldx_d = (int64_t)(xrow_d / xsz);
  // Operators that use at most four fifths of their source cells (round 6: half before; bilinear / nearest downsampling: config 2
  // uses a quarter) do not ship the whole field over PCIe: the staging copy packs the used cells of a
  // chunk batch-fastest (host_pack) and the chunk runs through the batch-fastest kernel.  Same bits.
  const int64_t U = op->csr.n_used_src;
  const bool may_pack = !(flags & (SMM_APPLY_HOST_NO_PACK | SMM_APPLY_KERNEL_SELL | SMM_APPLY_KERNEL_TILE)) &&
                        U > 0 && U * 5 <= S * 4;
  // Chunk size from the X AND Y bytes of a row (an operator with few used cells and a large target
  // is bound by its Y staging), clamped to a quarter of the free device memory: smm_internal.h
  const smm::HostChunk hc = smm::host_chunk_units(n_batch, xrow_d, (size_t)D * ysz, may_pack ? (size_t)U * xsz : 0,
                                                  8, 128, chunk_rows, free_device_bytes());   // packing pays from 8 rows on (24 rows: 4.2 -> 1.9 ms)
  const bool pack = hc.pack;
  chunk_rows = hc.units;
  if (pack) {
    int prc = ensure_sb(op);
    if (prc) return prc;
  }
  const bool x_pinned = is_pinned(x_host), y_pinned = is_pinned(y_host);
  // a pinned source with the device pitch can be DMA'd row-block-wise without staging
  const bool x_direct = x_pinned && !pack, y_direct = y_pinned;

  std::lock_guard<std::mutex> pipe_lock(op->pipe_mu);
  HostPipe& pipe = op->pipe;
  const size_t x_chunk_d = pack ? (size_t)chunk_rows * U * xsz : (size_t)chunk_rows * xrow_d;
  SMM_HIP(pipe.ensure(x_chunk_d, (size_t)chunk_rows * D * ysz,
                      x_direct ? 0 : (pack ? x_chunk_d : (size_t)chunk_rows * S * xsz),
                      y_direct ? 0 : (size_t)chunk_rows * D * ysz));

  const int64_t n_chunks = (n_batch + chunk_rows - 1) / chunk_rows;
  CallStats st;
  auto deliver = [&](int64_t c, int b) -> int {  // results of chunk c: pinned -> user rows
    if (y_direct) return SMM_OK;
    StageTimer t(st.v[SMM_HOST_STAT_COPY_OUT_MS]);
    const int64_t r0 = c * chunk_rows, rows = std::min(chunk_rows, n_batch - r0);
    if (ldy == D) return host_copy((char*)y_host + (size_t)r0 * yrow, pipe.hy[b].get(), (size_t)rows * D * ysz);
    for (int64_t r = 0; r < rows; ++r)
      memcpy((char*)y_host + (size_t)(r0 + r) * yrow, (char*)pipe.hy[b].get() + (size_t)r * D * ysz, (size_t)D * ysz);
    return SMM_OK;
  };
  auto launch = [&](int64_t c, int b) -> int {
    const int64_t r0 = c * chunk_rows, rows = std::min(chunk_rows, n_batch - r0);
    const char* xsrc = (const char*)x_host + (size_t)r0 * xrow;
    if (pack) {
      {
        StageTimer t(st.v[SMM_HOST_STAT_STAGE_IN_MS]);
        int rc = host_pack(pipe.hx[b].get(), xsrc, xsz, ldx, op->h_used, rows);
        if (rc) return rc;
      }
      SMM_HIP(pipe.mark(b, 0));
      SMM_HIP(hipMemcpyAsync(pipe.dx[b].get(), pipe.hx[b].get(), (size_t)U * rows * xsz, hipMemcpyHostToDevice,
                             pipe.stream[b]));
      st.v[SMM_HOST_STAT_H2D_BYTES] += (double)((size_t)U * rows * xsz);
    } else if (!x_direct) {
      {
        StageTimer t(st.v[SMM_HOST_STAT_STAGE_IN_MS]);
        if (ldx == S) {
          int rc = host_copy(pipe.hx[b].get(), xsrc, (size_t)rows * S * xsz);
          if (rc) return rc;
        } else {
          for (int64_t r = 0; r < rows; ++r)
            memcpy((char*)pipe.hx[b].get() + (size_t)r * S * xsz, xsrc + (size_t)r * xrow, (size_t)S * xsz);
        }
      }
      SMM_HIP(pipe.mark(b, 0));
      SMM_HIP(hipMemcpy2DAsync(pipe.dx[b].get(), xrow_d, pipe.hx[b].get(), (size_t)S * xsz, (size_t)S * xsz,
                               (size_t)rows, hipMemcpyHostToDevice, pipe.stream[b]));
    } else {
      SMM_HIP(pipe.mark(b, 0));
      SMM_HIP(hipMemcpy2DAsync(pipe.dx[b].get(), xrow_d, xsrc, xrow, (size_t)S * xsz, (size_t)rows,
                               hipMemcpyHostToDevice, pipe.stream[b]));
    }
    if (!pack) st.v[SMM_HOST_STAT_H2D_BYTES] += (double)((size_t)S * rows * xsz);
    SMM_HIP(pipe.mark(b, 1));
    int rc = SMM_OK;
    if (pack)
      rc = smm_apply_sb_impl(op, pipe.dx[b].get(), rows, pipe.dy[b].get(), D, rows, pipe.stream[b],
                             call.with_flags((flags & (SMM_APPLY_MASKED | SMM_APPLY_NO_FILL | SMM_APPLY_SKIPNA)) |
                                             SMM_APPLY_SB_PACKED));
    else
      rc = run_apply(target_of(op), nullptr, nullptr, pipe.dx[b].get(), ldx_d, 0, 0, pipe.dy[b].get(), D, 0, 0, rows, 1, 1,
                     call, pipe.stream[b]);
    if (rc) return rc;
    st.v[SMM_HOST_STAT_D2H_BYTES] += (double)((size_t)rows * D * ysz);
    SMM_HIP(pipe.mark(b, 2));
    if (!y_direct) {
      SMM_HIP(hipMemcpyAsync(pipe.hy[b].get(), pipe.dy[b].get(), (size_t)rows * D * ysz, hipMemcpyDeviceToHost,
                             pipe.stream[b]));
    } else {
      SMM_HIP(hipMemcpy2DAsync((char*)y_host + (size_t)r0 * yrow, yrow, pipe.dy[b].get(), (size_t)D * ysz,
                               (size_t)D * ysz, (size_t)rows, hipMemcpyDeviceToHost, pipe.stream[b]));
    }
    SMM_HIP(pipe.mark(b, 3));
    return SMM_OK;
  };
  return run_host_pipeline(pipe, n_chunks, st, launch, deliver);
}

static int smm_operator_mask_apply_impl(smm_operator_t op, const int32_t* src_imask, int32_t* dst_imask) {
  if (!op || !src_imask || !dst_imask) return fail(SMM_ERR_INVALID, "null argument");
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  const int64_t S = op->csr.n_src, D = op->csr.n_dst;
  if (D == 0) return SMM_OK;
  // int32 mask promoted to f64 for the product (weights.py:50)
  std::vector<double> xs((size_t)std::max<int64_t>(S, 1));
  for (int64_t i = 0; i < S; ++i) xs[(size_t)i] = (double)src_imask[i];
  DeviceBuf<int32_t> dm;   // freed on every return, in the order dx, dy, dm
  DeviceBuf<double> dy, dx;
  if (dx.alloc(xs.size()) != hipSuccess || dy.alloc((size_t)D) != hipSuccess || dm.alloc((size_t)D) != hipSuccess)
    return fail(SMM_ERR_HIP, "device allocation failed in smm_operator_mask_apply");
  if (hipMemcpy(dx.get(), xs.data(), xs.size() * 8, hipMemcpyHostToDevice) != hipSuccess)
    return fail(SMM_ERR_HIP, "hipMemcpy failed in smm_operator_mask_apply");
  ApplyTarget sell_only = target_of(op);   // one row: kernel A whatever the plan
  sell_only.tile_ok = false;
  int rc = run_apply(sell_only, nullptr, nullptr, dx.get(), std::max<int64_t>(S, 1), 0, 0, dy.get(), D, 0, 0, 1, 1, 1,
                     CallDesc{SMM_F64, SMM_F64, SMM_APPLY_NO_FILL, 0.0}, nullptr);
  if (rc == SMM_OK) {
    const int threads = 256;
    hipLaunchKernelGGL(smm_mask_threshold_kernel, dim3((unsigned)((D + threads - 1) / threads)),
                       dim3(threads), 0, nullptr, dy.get(), dm.get(), D);
    if (hipGetLastError() != hipSuccess ||
        hipMemcpy(dst_imask, dm.get(), (size_t)D * 4, hipMemcpyDeviceToHost) != hipSuccess) {
      rc = fail(SMM_ERR_HIP, "mask threshold kernel / copy failed");
    }
  }
  return rc;
}

// ---- groups

static int smm_group_create_impl(const smm_operator_t* ops, int n_ops, smm_group_t* out) {
  if (!out) return fail(SMM_ERR_INVALID, "null out handle");
  *out = nullptr;
  if (!ops || n_ops <= 0) return fail(SMM_ERR_INVALID, "a group needs at least one operator");
  for (int i = 0; i < n_ops; ++i) {
    if (!ops[i]) return fail(SMM_ERR_INVALID, "null operator in group");
    if (ops[i]->device != ops[0]->device || ops[i]->csr.n_src != ops[0]->csr.n_src ||
        ops[i]->csr.n_dst != ops[0]->csr.n_dst)
      return fail(SMM_ERR_INVALID, "group members must share device and grid sizes");
  }
  std::unique_ptr<smm_group> owner(new (std::nothrow) smm_group());   // freed on every early return and on a throw
  if (!owner) return fail(SMM_ERR_ALLOC, "out of host memory");
  smm_group* g = owner.get();
  g->device = ops[0]->device;
  g->ops.assign(ops, ops + n_ops);
  g->tile_valid = true;
  // one launch covers all levels: one plan shape for all members (single-wave blocks as soon as
  // any level has rows longer than 16 links), and the links' majority decides tile vs SELL
  for (int i = 0; i < n_ops; ++i) g->tile_which = std::max(g->tile_which, ops[i]->native_plan());
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select device");
  int64_t nnz_all = 0, nnz_pref = 0;
  std::vector<LevelDesc> descs((size_t)n_ops);
  for (int i = 0; i < n_ops; ++i) {
    int prc = ensure_plan(ops[i], g->tile_which);
    if (prc) return prc;
    const smm_operator::TilePlan& pl = ops[i]->plan[g->tile_which];
    descs[(size_t)i] = ops[i]->desc(g->tile_which);
    g->tile_valid = g->tile_valid && pl.valid;
    nnz_all += ops[i]->csr.nnz;
    if (pl.preferred) nnz_pref += ops[i]->csr.nnz;
    g->tile_reuse = g->tile_reuse || pl.reuse;
    g->tile_max_chunks = std::max(g->tile_max_chunks, pl.max_chunks);
    g->max_row_nnz = std::max(g->max_row_nnz, ops[i]->csr.max_row_nnz);
  }
  g->tile_preferred = 2 * nnz_pref >= nnz_all;
  int rc = upload(g->d_descs, descs);
  if (rc) return rc;
  for (int i = 0; i < n_ops; ++i) ops[i]->group_refs.fetch_add(1);
  *out = owner.release();
  return SMM_OK;
}

int smm_group_plan_info(smm_group_t g, int* kernel_kind, int* slices_per_block) {
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  if (kernel_kind) *kernel_kind = (g->tile_valid ? 1 : 0) | (g->tile_preferred ? 2 : 0);
  if (slices_per_block) *slices_per_block = g->tile_which ? 1 : kWavesPerBlock;   // 1 also for parts of a slice
  return SMM_OK;
}

int smm_group_destroy(smm_group_t g) {
  if (!g) return SMM_OK;
  DeviceGuard guard(g->device);
  for (smm_operator_t op : g->ops) op->group_refs.fetch_sub(1);
  delete g;
  return SMM_OK;
}

extern "C++" {
int smm::group_level_cfg(smm_group_t g, int64_t n_lev, const int32_t* level_index,
                         const uint8_t* masked_levels, double remap_area_min, unsigned flags,
                         const int32_t** d_map, const uint8_t** d_masked) {   // smm_device.hpp
  *d_map = nullptr;
  *d_masked = nullptr;
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  if (n_lev < 0) return fail(SMM_ERR_INVALID, "negative level count");
  if (int vrc = check_levels(g, n_lev, level_index, masked_levels, remap_area_min, flags)) return vrc;
  if (n_lev == 0) return SMM_OK;
  const int n_ops = (int)g->ops.size();

  // key: level count, then the map, then (if given) one masked flag per member -- unambiguous
  std::string key((const char*)&n_lev, sizeof(n_lev));
  key.append((const char*)level_index, (size_t)n_lev * sizeof(int32_t));
  key.push_back(masked_levels ? 1 : 0);
  if (masked_levels) key.append((const char*)masked_levels, (size_t)n_ops);
  const char* d_cfg = nullptr;
  const size_t map_bytes = ((size_t)n_lev * 4 + 15) & ~(size_t)15;
  {
    std::lock_guard<std::mutex> lock(g->mu);
    auto it = g->cfg_cache.find(key);
    if (it != g->cfg_cache.end()) {
      d_cfg = it->second.get();
    } else {
      // first sight of this configuration (smm_group_prepare does this ahead of time): one small
      // allocation + blocking copy, no device-wide synchronisation, nothing is ever evicted
      std::vector<char> buf(map_bytes + (size_t)n_ops, 0);
      memcpy(buf.data(), level_index, (size_t)n_lev * 4);
      if (masked_levels) memcpy(buf.data() + map_bytes, masked_levels, (size_t)n_ops);
      DeviceBuf<char> cfg;   // filled before it enters the map
      SMM_HIP(cfg.upload(buf));
      d_cfg = cfg.get();
      g->cfg_cache.emplace(std::move(key), std::move(cfg));
    }
  }
  *d_map = (const int32_t*)d_cfg;
  *d_masked = masked_levels ? (const uint8_t*)(d_cfg + map_bytes) : nullptr;
  return SMM_OK;
}
}  // extern "C++"

static int smm_group_prepare_impl(smm_group_t g, int64_t n_lev, const int32_t* level_index,
                      const uint8_t* masked_levels) {
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  const int32_t* d_map;
  const uint8_t* d_masked;
  return group_level_cfg(g, n_lev, level_index, masked_levels, 0.0, 0u, &d_map, &d_masked);
}

static int smm_group_apply_impl(smm_group_t g, const void* x, int64_t xs_outer, int64_t xs_lev, int64_t xs_inner, void* y,
                                int64_t ys_outer, int64_t ys_lev, int64_t ys_inner, int64_t n_outer, int64_t n_lev,
                                int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels, void* stream,
                                const CallDesc& call) {
  if (int frc = check_flags(call.flags)) return frc;
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  const int32_t* d_map;
  const uint8_t* d_masked;
  int rc = group_level_cfg(g, n_lev, level_index, masked_levels, call.area_min, call.flags, &d_map, &d_masked);
  if (rc || n_lev == 0) return rc;
  return run_apply(target_of(g), d_map, d_masked, x, xs_outer, xs_lev, xs_inner, y, ys_outer, ys_lev, ys_inner, n_outer,
                   n_lev, n_inner, call, (hipStream_t)stream);
}

static int smm_group_prepare_sb_impl(smm_group_t g) {
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  for (smm_operator* op : g->ops) {
    int rc = ensure_sb(op);
    if (rc) return rc;
  }
  return SMM_OK;
}

// All data levels in ONE launch of the batch-fastest kernel (smm_group_apply_sb_kernel): the levels' CSR / epilogue
// pointers travel by value in the kernel arguments (a pointer table in device memory made the column / weight /
// row-pointer streams vector loads, 162 instead of 88 VGPRs; through kernarg + constant-address-space views they
// stay scalar), so the dispatcher balances thin deep levels against the surface ones and there is no ramp-up and
// tail per level.  Groups of more than kSbGroupLevels data levels take several launches on the caller's stream.
// BASELINE config 3 kept batch-fastest, same box: 9.51 ms against 10.24 ms for one launch per level dealt over a
// pool of 8 streams (round 4's form, removed: profiles/r05_cfg3sb_grouped_vs_stream_pool.txt) and 14.4 ms for one
// launch per level on one stream (still there: SMM_TUNE_SB_LEVEL_LAUNCHES, and for levels beyond the grid limit).
static int smm_group_apply_sb_impl(smm_group_t g, const void* x, int64_t xs_lev, int64_t ldx, void* y, int64_t ys_lev,
                                   int64_t ys_batch, int64_t n_batch, int64_t n_lev, const int32_t* level_index,
                                   const uint8_t* masked_levels, void* stream, const CallDesc& call) {
  const unsigned flags = call.flags;
  const double remap_area_min = call.area_min;
  if (int frc = check_flags(flags)) return frc;
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  if (n_batch < 0 || n_lev < 0) return fail(SMM_ERR_INVALID, "negative batch size / level count");
  if (flags & SMM_APPLY_SB_PACKED)
    return fail(SMM_ERR_UNSUPPORTED, "packed fields are per operator: a group takes whole (S, B) slabs");
  if (int drc = check_x_dtype(call)) return drc;
  if (int irc = check_levels(g, n_lev, level_index, nullptr, 0.0, 0u)) return irc;   // an empty call answers for these only
  if (n_lev == 0 || n_batch == 0 || g->ops[0]->csr.n_dst == 0) return SMM_OK;
  if (!x || !y) return fail(SMM_ERR_INVALID, "null field pointer");
  const size_t xsz = dtype_size(call.x_dtype), ysz = dtype_size(call.y_dtype);
  // the whole call is validated before the first launch (as smm_group_apply does): a later level's
  // missing dst_imask / dst_frac or a bad stride must not surface after earlier levels wrote part of Y
  if (ldx < n_batch) return fail(SMM_ERR_INVALID, "ldx smaller than the batch");
  if (ys_batch < ((flags & SMM_APPLY_SB_Y_SB) ? n_batch : g->ops[0]->csr.n_dst))
    return fail(SMM_ERR_INVALID, "ys_batch smaller than a row of Y");
  if ((uintptr_t)x % xsz || (uintptr_t)y % ysz) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
  if (int arc = check_area_min(remap_area_min)) return arc;
  if (int vrc = check_levels(g, n_lev, level_index, masked_levels, remap_area_min, flags)) return vrc;
  const bool per_level_launches = smm::tuning(SMM_TUNE_SB_LEVEL_LAUNCHES) == 1;
  hipStream_t caller = (hipStream_t)stream;
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  const int64_t n_dst = g->ops[0]->csr.n_dst;
  const int64_t td = smm_launch::sb_tile_rows(ysz);   // the tile height launch_sb_group takes (a packed Y: 64 or 16)
  const int64_t per_level = ((n_dst + td - 1) / td) * ((n_batch + 127) / 128);
  if (!per_level_launches && per_level <= grid_limit()) {
    // grouped launches of as many levels as the kernel arguments (and the launch grid) hold
    for (smm_operator* op : g->ops) {          // the canonical CSR copies the kernel reads (uploaded once)
      int erc = ensure_sb(op);
      if (erc) return erc;
    }
    const int64_t max_lev = std::max<int64_t>(1, std::min<int64_t>(kSbGroupLevels, grid_limit() / per_level));
    const bool fill = !(flags & SMM_APPLY_NO_FILL);
    for (int64_t l0 = 0; l0 < n_lev; l0 += max_lev) {
      SbGroupArgs a{};
      a.n_lev = (int)std::min<int64_t>(max_lev, n_lev - l0);
      a.x = (const char*)x + (size_t)l0 * xs_lev * xsz;
      a.y = (char*)y + (size_t)l0 * ys_lev * ysz;
      a.xs_lev = xs_lev;
      a.ys_lev = ys_lev;
      a.ldx = ldx;
      a.ldy = ys_batch;
      a.n_batch = n_batch;
      a.n_dst = n_dst;
      a.area_min = remap_area_min;
      for (int i = 0; i < a.n_lev; ++i) {
        const int w = level_index[l0 + i];
        const smm_operator* op = g->ops[(size_t)w];
        a.lev[i] = SbLevelPtrs{op->d_csr_rowptr.get(), op->d_csr_col.get(), op->d_csr_val.get(),
                               level_masked(flags, masked_levels, w) ? op->d_imask.get() : nullptr, op->d_frac.get()};
      }
      if (call.packed_x()) a.cf = call.cf;      // CF-packed: raw 2-byte slabs, one decode rule for every level
      if (call.has_enc) a.cfo = call.enc;       // one encode rule for every level
      const int rc = call.dispatch([&](auto b) {
        using B = decltype(b);
        return launch_sb_group<typename B::XT, typename B::YT, B::skipna>(a, fill, flags, caller);
      });
      if (rc) return rc;
    }
    return SMM_OK;
  }
  // A level whose own grid exceeds the launch limit (smm_apply_sb cuts its batch into parts), or the tuning knob
  // SMM_TUNE_SB_LEVEL_LAUNCHES: one launch per data level on the caller's stream.
  int status = SMM_OK;
  for (int64_t l = 0; l < n_lev && status == SMM_OK; ++l) {
    const int w = level_index[l];
    unsigned fl = flags & ~(unsigned)SMM_APPLY_MASKED;
    if (level_masked(flags, masked_levels, w)) fl |= SMM_APPLY_MASKED;
    status = smm_apply_sb_impl(g->ops[(size_t)w], (const char*)x + (size_t)l * xs_lev * xsz, ldx,
                               (char*)y + (size_t)l * ys_lev * ysz, ys_batch, n_batch, caller, call.with_flags(fl));
  }
  return status;
}

extern "C++" {
// The call the *_launch_info entries describe: an f64 result; a packed x_dtype answers for the _cf entries (the
// geometry does not depend on the rule)
static CallDesc info_call(int x_dtype, unsigned flags) {
  CallDesc c{x_dtype, SMM_F64, flags, 0.0};
  c.has_cf = c.packed_x();
  return c;
}
static void fill_launch_info(const LaunchInfo& li, int* kernel, int* j_per_block, int* rows_per_step,
                             int* rows_per_block, int64_t* n_blocks, int64_t* lds_bytes, int* big_operator) {
  if (kernel) *kernel = li.tile ? (li.dma ? 2 : 1) : 0;
  if (j_per_block) *j_per_block = li.j_per_block;
  if (rows_per_step) *rows_per_step = li.rows_per_step;
  if (rows_per_block) *rows_per_block = li.rows_per_block;
  if (n_blocks) *n_blocks = li.n_blocks;
  if (lds_bytes) *lds_bytes = li.lds_bytes;
  if (big_operator) *big_operator = li.big_operator ? 1 : 0;
}
}  // extern "C++"

static int smm_operator_launch_info_impl(smm_operator_t op, int x_dtype, int64_t n_batch, unsigned flags, int* kernel,
                             int* j_per_block, int* rows_per_step, int* rows_per_block, int64_t* n_blocks,
                             int64_t* lds_bytes, int* big_operator) {
  if (int frc = check_flags(flags)) return frc;
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  LaunchInfo li;
  int rc = run_apply(target_of(op), nullptr, nullptr, nullptr, op->csr.n_src, 0, 0, nullptr, op->csr.n_dst, 0, 0, n_batch,
                     1, 1, info_call(x_dtype, flags), nullptr, &li);
  if (rc) return rc;
  fill_launch_info(li, kernel, j_per_block, rows_per_step, rows_per_block, n_blocks, lds_bytes, big_operator);
  return SMM_OK;
}

static int smm_group_launch_info_impl(smm_group_t g, int x_dtype, int64_t n_outer, int64_t n_lev, int64_t n_inner,
                          unsigned flags, int* kernel, int* j_per_block, int* rows_per_step,
                          int* rows_per_block, int64_t* n_blocks, int64_t* lds_bytes, int* big_operator) {
  if (int frc = check_flags(flags)) return frc;
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  LaunchInfo li;
  int rc = run_apply(target_of(g), nullptr, nullptr, nullptr, 0, 0, 0, nullptr, 0, 0, 0, n_outer, n_lev, n_inner,
                     info_call(x_dtype, flags), nullptr, &li);
  if (rc) return rc;
  fill_launch_info(li, kernel, j_per_block, rows_per_step, rows_per_block, n_blocks, lds_bytes, big_operator);
  return SMM_OK;
}

// Host-buffer variant of smm_group_apply: X host (n_outer, n_lev, n_inner, S) C-contiguous,
// Y host (n_outer, n_inner, n_lev, D) when transpose != 0 (regrid.py:420-427), else
// (n_lev, n_outer, n_inner, D) (concat order, regrid.py:410).  Chunks of the outer axis
// stream through the group's double-buffered H2D / kernel / D2H pipeline.
static int smm_group_apply_host_impl(smm_group_t g, const void* x_host, void* y_host, int64_t n_outer, int64_t n_lev,
                                     int64_t n_inner, int transpose, const int32_t* level_index,
                                     const uint8_t* masked_levels, int64_t chunk_outer, const CallDesc& call) {
  const int x_dtype = call.x_dtype, y_dtype = call.y_dtype;
  const unsigned flags = call.flags;
  const bool enc = call.has_enc;
  if (int frc = check_flags(flags)) return frc;
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  if (n_outer < 0 || n_lev < 0 || n_inner < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (int drc = check_x_dtype(call)) return drc;
  const bool packed = call.packed_x();
  if (call.half() && (flags & SMM_APPLY_KERNEL_TILE))
    return fail(SMM_ERR_UNSUPPORTED, "the LDS tile kernel is not built for half-precision fields or results (SMM_F16 / SMM_BF16)");
  if ((packed || enc) && (flags & SMM_APPLY_KERNEL_TILE))
    return fail(SMM_ERR_UNSUPPORTED, "the LDS tile kernel is not built for packed fields or results (SMM_I16 / SMM_U16)");
  const int64_t S = g->ops[0]->csr.n_src, D = g->ops[0]->csr.n_dst;
  if (n_outer == 0 || n_lev == 0 || n_inner == 0 || D == 0) return SMM_OK;
  if (!x_host || !y_host) return fail(SMM_ERR_INVALID, "null field pointer");
  if ((packed || is_half_dtype(x_dtype)) && (uintptr_t)x_host % 2) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
  if ((enc || is_half_dtype(y_dtype)) && (uintptr_t)y_host % 2) return fail(SMM_ERR_INVALID, "result pointer is not element aligned");
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");

  // every selected level is checked before anything is staged or launched (as smm_group_apply does): a level that
  // lacks dst_imask / dst_frac must not surface after earlier levels have written part of Y
  if (int arc = check_area_min(call.area_min)) return arc;
  if (int vrc = check_levels(g, n_lev, level_index, masked_levels, call.area_min, flags)) return vrc;

  // The chunks of the pipeline (smm::plan_group_chunks): whole rows, or each level's used cells packed batch-fastest.
  // The slabs of a packed chunk lie back to back (level l's at the running sum of U_l * batch * xsz): kernel C's
  // 4-B-per-lane loads of 2-byte elements only assume element alignment (xvec_u, smm_kernels.hpp), and a slab can start
  // on an odd element only when the batch count is odd -- when every other row of every slab starts on one anyway -- so
  // no padding is added.  The pinned staging and both host layouts of a chunk's level range follow xsz / ysz too.
  const size_t xsz = dtype_size(x_dtype), ysz = dtype_size(y_dtype);
  const int64_t rows_per_outer = n_lev * n_inner;
  std::vector<int64_t> used_per_level((size_t)n_lev);
  for (int64_t l = 0; l < n_lev; ++l) used_per_level[(size_t)l] = g->ops[(size_t)level_index[l]]->csr.n_used_src;
  const smm::GroupChunkPlan plan = smm::plan_group_chunks(
      n_outer, n_lev, n_inner, S, D, xsz, ysz, used_per_level.data(),
      !(flags & (SMM_APPLY_HOST_NO_PACK | SMM_APPLY_KERNEL_SELL | SMM_APPLY_KERNEL_TILE)), chunk_outer,
      free_device_bytes(), smm::tuning(SMM_TUNE_HOST_CHUNK_KB));
  using GChunk = smm::GroupChunk;
  const std::vector<GChunk>& chunks = plan.chunks;
  const bool pack = plan.pack;
  const size_t xrow_d = plan.x_row;
  const int64_t ldx_d = (int64_t)(xrow_d / xsz);
  if (pack)
    if (int prc = smm_group_prepare_sb(g)) return prc;
  const bool x_direct = is_pinned(x_host) && !pack, y_direct = is_pinned(y_host);

  std::lock_guard<std::mutex> pipe_lock(g->pipe_mu);
  HostPipe& pipe = g->pipe;
  SMM_HIP(pipe.ensure(plan.max_x, plan.max_y, x_direct ? 0 : (pack ? plan.max_x : plan.max_rows * S * xsz),
                      y_direct ? 0 : plan.max_y));

  const int64_t n_chunks = (int64_t)chunks.size();
  CallStats st;
  // Y of a chunk on the device: (no, n_inner, nl, D) when transpose, else (nl, no, n_inner, D); on the host the chunk is
  // the level range [l0, l0 + nl) of rows [o0, o0 + no): `rows` runs of nl * D values at a pitch of n_lev * D (transpose),
  // nl runs of no * n_inner * D values (else).  whole = the chunk holds every level: one contiguous block when transpose.
  auto y_to_host = [&](const GChunk& c, const char* src, bool async, hipStream_t stream) -> int {
    const int64_t bc = c.no * n_inner;
    if (transpose) {
      char* dst = (char*)y_host + ((size_t)c.o0 * n_inner * n_lev + (size_t)c.l0) * D * ysz;
      const size_t width = (size_t)c.nl * D * ysz, pitch = (size_t)n_lev * D * ysz;
      if (async) {
        if (c.nl == n_lev)
          SMM_HIP(hipMemcpyAsync(dst, src, (size_t)bc * width, hipMemcpyDeviceToHost, stream));
        else
          SMM_HIP(hipMemcpy2DAsync(dst, pitch, src, width, width, (size_t)bc, hipMemcpyDeviceToHost, stream));
      } else if (c.nl == n_lev) {
        int rc = host_copy(dst, src, (size_t)bc * width);
        if (rc) return rc;
      } else {
        int rc = stage_status(smm::host_copy_2d(dst, pitch, src, width, width, bc), "host copy");
        if (rc) return rc;
      }
    } else {  // device chunk is (nl, no, n_inner, D); host is (n_lev, n_outer, n_inner, D)
      const size_t blk = (size_t)bc * D * ysz;
      for (int64_t ll = 0; ll < c.nl; ++ll) {
        char* dst = (char*)y_host + (((size_t)(c.l0 + ll)) * n_outer + (size_t)c.o0) * n_inner * D * ysz;
        if (async) {
          SMM_HIP(hipMemcpyAsync(dst, src + (size_t)ll * blk, blk, hipMemcpyDeviceToHost, stream));
        } else {
          int rc = host_copy(dst, src + (size_t)ll * blk, blk);
          if (rc) return rc;
        }
      }
    }
    return SMM_OK;
  };
  auto deliver = [&](int64_t c, int b) -> int {
    if (y_direct) return SMM_OK;
    StageTimer t(st.v[SMM_HOST_STAT_COPY_OUT_MS]);
    return y_to_host(chunks[(size_t)c], (const char*)pipe.hy[b].get(), false, nullptr);
  };
  auto launch = [&](int64_t c, int b) -> int {
    const GChunk& ck = chunks[(size_t)c];
    const int64_t o0 = ck.o0, no = ck.no;
    const char* xsrc = (const char*)x_host + (size_t)o0 * rows_per_outer * S * xsz;
    int rc = SMM_OK;
    if (pack) {
      const int64_t bc = no * n_inner;   // batch entries per level in this chunk: b = (o - o0) * n_inner + i
      size_t off = 0;                    // bytes
      {
        StageTimer t(st.v[SMM_HOST_STAT_STAGE_IN_MS]);
        for (int64_t l = ck.l0; l < ck.l0 + ck.nl; ++l) {
          smm_operator* op = g->ops[(size_t)level_index[l]];
          int hrc = host_pack((char*)pipe.hx[b].get() + off, xsrc + (size_t)l * n_inner * S * xsz, xsz, n_inner,
                              rows_per_outer * S, S, op->h_used, bc);
          if (hrc) return hrc;
          off += (size_t)op->csr.n_used_src * bc * xsz;
        }
      }
      SMM_HIP(pipe.mark(b, 0));
      SMM_HIP(hipMemcpyAsync(pipe.dx[b].get(), pipe.hx[b].get(), off, hipMemcpyHostToDevice, pipe.stream[b]));
      st.v[SMM_HOST_STAT_H2D_BYTES] += (double)off;
      SMM_HIP(pipe.mark(b, 1));
      off = 0;
      for (int64_t ll = 0; ll < ck.nl && !rc; ++ll) {
        const int w = level_index[ck.l0 + ll];
        smm_operator* op = g->ops[(size_t)w];
        unsigned fl = (flags & (SMM_APPLY_NO_FILL | SMM_APPLY_SKIPNA)) | SMM_APPLY_SB_PACKED;
        if (level_masked(flags, masked_levels, w)) fl |= SMM_APPLY_MASKED;
        // Y of the chunk: entry (b, ll, d) at (b * nl + ll) * D + d when transpose, at (ll * bc + b) * D + d else
        rc = smm_apply_sb_impl(op, (char*)pipe.dx[b].get() + off, bc,
                               (char*)pipe.dy[b].get() + (size_t)ll * (transpose ? D : bc * D) * ysz,
                               transpose ? ck.nl * D : D, bc, pipe.stream[b], call.with_flags(fl));
        off += (size_t)op->csr.n_used_src * bc * xsz;
      }
    } else {
      const int64_t rows = no * rows_per_outer;
      int64_t ys_o, ys_l, ys_i;
      if (transpose) {
        ys_o = n_inner * n_lev * D, ys_l = D, ys_i = n_lev * D;
      } else {
        ys_o = n_inner * D, ys_l = no * n_inner * D, ys_i = D;
      }
      const void* h2d_src = xsrc;
      if (!x_direct) {
        StageTimer t(st.v[SMM_HOST_STAT_STAGE_IN_MS]);
        int hrc = host_copy(pipe.hx[b].get(), xsrc, (size_t)rows * S * xsz);
        if (hrc) return hrc;
        h2d_src = pipe.hx[b].get();
      }
      SMM_HIP(pipe.mark(b, 0));
      SMM_HIP(hipMemcpy2DAsync(pipe.dx[b].get(), xrow_d, h2d_src, (size_t)S * xsz, (size_t)S * xsz, (size_t)rows,
                               hipMemcpyHostToDevice, pipe.stream[b]));
      st.v[SMM_HOST_STAT_H2D_BYTES] += (double)((size_t)S * xsz * (size_t)rows);
      SMM_HIP(pipe.mark(b, 1));
      rc = smm_group_apply_impl(g, pipe.dx[b].get(), rows_per_outer * ldx_d, n_inner * ldx_d, ldx_d, pipe.dy[b].get(),
                                ys_o, ys_l, ys_i, no, n_lev, n_inner, level_index, masked_levels, pipe.stream[b], call);
    }
    if (rc) return rc;
    SMM_HIP(pipe.mark(b, 2));
    st.v[SMM_HOST_STAT_D2H_BYTES] += (double)((size_t)no * n_inner * ck.nl * D * ysz);
    if (!y_direct) {
      SMM_HIP(hipMemcpyAsync(pipe.hy[b].get(), pipe.dy[b].get(), (size_t)no * n_inner * ck.nl * D * ysz,
                             hipMemcpyDeviceToHost, pipe.stream[b]));
    } else {
      int yrc = y_to_host(ck, (const char*)pipe.dy[b].get(), true, pipe.stream[b]);
      if (yrc) return yrc;
    }
    SMM_HIP(pipe.mark(b, 3));
    return SMM_OK;
  };
  return run_host_pipeline(pipe, n_chunks, st, launch, deliver);
}

}  // extern "C"

// ---- the guarded entry points: whatever an implementation above throws (std::bad_alloc from a plan vector, a
// std::system_error) becomes a status here -- nothing crosses the extern "C" boundary (include/smmregrid_amd.h)
extern "C" {

int smm_operator_set_epilogue(smm_operator_t op, const int32_t* dst_imask, const double* dst_frac) {
  return guarded([&] { return smm_operator_set_epilogue_impl(op, dst_imask, dst_frac); });
}

int smm_operator_mask_apply(smm_operator_t op, const int32_t* src_imask, int32_t* dst_imask) {
  return guarded([&] { return smm_operator_mask_apply_impl(op, src_imask, dst_imask); });
}

int smm_operator_prepare_sb(smm_operator_t op) {
  return guarded([&] { return smm_operator_prepare_sb_impl(op); });
}

int smm_operator_used_sources(smm_operator_t op, int32_t* used) {
  return guarded([&] { return smm_operator_used_sources_impl(op, used); });
}

}  // extern "C"

namespace {
// smm_cf_decode_t -> the call's decode rule.  A plain float call (cf == NULL) is left as it is.
int make_cf(const smm_cf_decode_t* cf, CallDesc& c) {
  if (!c.packed_x()) {
    if (cf && is_float_dtype(c.x_dtype))
      return fail(SMM_ERR_INVALID, "a decode rule was given with a float field: pass cf = NULL, or the raw 16-bit field");
    if (cf && is_half_dtype(c.x_dtype))
      return fail(SMM_ERR_INVALID, "a decode rule was given with an SMM_F16 / SMM_BF16 field: half-precision fields take the plain entries");
    return SMM_OK;   // float: the plain entry; anything else: refused by the dtype check
  }
  if (!cf) return fail(SMM_ERR_INVALID, "SMM_I16 / SMM_U16 fields need a decode rule (cf is NULL)");
  if (cf->decode_dtype != SMM_F32 && cf->decode_dtype != SMM_F64)
    return fail(SMM_ERR_INVALID, "cf->decode_dtype must be SMM_F32 or SMM_F64");
  if (cf->n_fill < 0 || cf->n_fill > 2) return fail(SMM_ERR_INVALID, "cf->n_fill must be 0, 1 or 2");
  const int32_t lo = c.x_dtype == SMM_I16 ? -32768 : 0, hi = c.x_dtype == SMM_I16 ? 32767 : 65535;
  for (int i = 0; i < cf->n_fill; ++i)
    if (cf->fill[i] < lo || cf->fill[i] > hi)
      return fail(SMM_ERR_INVALID, "cf->fill[" + std::to_string(i) + "] is not representable in the raw type");
  if (cf->n_fill > 0 && (c.flags & SMM_APPLY_NO_FILL))
    return fail(SMM_ERR_INVALID, "SMM_APPLY_NO_FILL with fill values: the decode makes NaN");
  const int32_t none = 0x7fffffff;   // no 16-bit element compares equal
  c.cf.scale = cf->scale;
  c.cf.offset = cf->offset;
  c.cf.fill0 = cf->n_fill > 0 ? cf->fill[0] : none;
  c.cf.fill1 = cf->n_fill > 1 ? cf->fill[1] : c.cf.fill0;
  c.decode_dtype = cf->decode_dtype;
  c.has_cf = true;
  return SMM_OK;
}

// smm_cf_encode_t -> the call's encode rule, with every refusal of the _pk entries that needs no device.  enc == NULL
// with a float y_dtype: the _cf entry unchanged.
int make_enc(const smm_cf_encode_t* enc, CallDesc& c) {
  if (!enc) {
    if (is_packed_dtype(c.y_dtype))
      return fail(SMM_ERR_INVALID, "SMM_I16 / SMM_U16 results need an encode rule (enc is NULL)");
    return SMM_OK;
  }
  if (!is_packed_dtype(c.y_dtype))
    return fail(SMM_ERR_INVALID, "an encode rule was given with a float y_dtype: pass enc = NULL, or y_dtype SMM_I16 / SMM_U16");
  if (enc->reserved != 0) return fail(SMM_ERR_INVALID, "enc->reserved must be 0");
  if (!std::isfinite(enc->scale) || enc->scale == 0.0) return fail(SMM_ERR_INVALID, "enc->scale must be finite and non-zero");
  if (!std::isfinite(enc->offset)) return fail(SMM_ERR_INVALID, "enc->offset must be finite");
  const int32_t lo = c.y_dtype == SMM_I16 ? -32768 : 0, hi = c.y_dtype == SMM_I16 ? 32767 : 65535;
  if (enc->fill < lo || enc->fill > hi) return fail(SMM_ERR_INVALID, "enc->fill is not representable in the raw type");
  if (c.flags & SMM_APPLY_KERNEL_TILE)
    return fail(SMM_ERR_UNSUPPORTED, "the LDS tile kernel is not built for packed results (SMM_I16 / SMM_U16)");
  c.enc = CfOutParams{enc->scale, enc->offset, enc->fill, 0};
  c.has_enc = true;
  return SMM_OK;
}

// The preamble of every apply entry: the plain ones take no rule (16-bit dtypes are then refused by the dtype check),
// the _cf ones a decode rule, the _pk ones both -- the encode rule is validated first, before the handle is looked at.
enum class Entry { plain, cf, pk };
template <typename F>
int apply_entry(Entry kind, int x_dtype, int y_dtype, double remap_area_min, unsigned flags, const smm_cf_decode_t* cf,
                const smm_cf_encode_t* enc, F&& body) {
  return guarded([&] {
    CallDesc c{x_dtype, y_dtype, flags, remap_area_min};
    if (kind == Entry::pk)
      if (int rc = make_enc(enc, c)) return rc;
    if (kind != Entry::plain)
      if (int rc = make_cf(cf, c)) return rc;
    return body(c);
  });
}
}  // namespace

extern "C" {

int smm_apply(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
              int64_t n_batch, double remap_area_min, unsigned flags, void* stream) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_apply_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_cf(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_apply_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_pk(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf,
                 const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_apply_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_sb(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_apply_sb_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_sb_cf(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
                    int64_t n_batch, double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_apply_sb_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_sb_pk(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int y_dtype, int64_t ldy,
                    int64_t n_batch, double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf,
                    const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_apply_sb_impl(op, x, ldx, y, ldy, n_batch, stream, c);
  });
}

int smm_apply_host(smm_operator_t op, const void* x_host, int x_dtype, int64_t ldx, void* y_host, int y_dtype,
                   int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_apply_host_impl(op, x_host, ldx, y_host, ldy, n_batch, chunk_rows, c);
  });
}

int smm_apply_host_cf(smm_operator_t op, const void* x_host, int x_dtype, int64_t ldx, void* y_host, int y_dtype,
                      int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows,
                      const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_apply_host_impl(op, x_host, ldx, y_host, ldy, n_batch, chunk_rows, c);
  });
}

int smm_apply_host_pk(smm_operator_t op, const void* x_host, int x_dtype, int64_t ldx, void* y_host, int y_dtype,
                      int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows,
                      const smm_cf_decode_t* cf, const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_apply_host_impl(op, x_host, ldx, y_host, ldy, n_batch, chunk_rows, c);
  });
}

int smm_group_create(const smm_operator_t* ops, int n_ops, smm_group_t* out) {
  return guarded([&] { return smm_group_create_impl(ops, n_ops, out); });
}

int smm_group_prepare(smm_group_t g, int64_t n_lev, const int32_t* level_index, const uint8_t* masked_levels) {
  return guarded([&] { return smm_group_prepare_impl(g, n_lev, level_index, masked_levels); });
}

int smm_group_prepare_sb(smm_group_t g) {
  return guarded([&] { return smm_group_prepare_sb_impl(g); });
}

// the group entries: one decode rule / encode rule for every level
int smm_group_apply(smm_group_t g, const void* x, int x_dtype, int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                    void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner, int64_t n_outer,
                    int64_t n_lev, int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                    double remap_area_min, unsigned flags, void* stream) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_impl(g, x, xs_outer, xs_lev, xs_inner, y, ys_outer, ys_lev, ys_inner, n_outer, n_lev,
                                n_inner, level_index, masked_levels, stream, c);
  });
}

int smm_group_apply_cf(smm_group_t g, const void* x, int x_dtype, int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                       void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner, int64_t n_outer,
                       int64_t n_lev, int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                       double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_impl(g, x, xs_outer, xs_lev, xs_inner, y, ys_outer, ys_lev, ys_inner, n_outer, n_lev,
                                n_inner, level_index, masked_levels, stream, c);
  });
}

int smm_group_apply_pk(smm_group_t g, const void* x, int x_dtype, int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                       void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner, int64_t n_outer,
                       int64_t n_lev, int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                       double remap_area_min, unsigned flags, void* stream, const smm_cf_decode_t* cf,
                       const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_group_apply_impl(g, x, xs_outer, xs_lev, xs_inner, y, ys_outer, ys_lev, ys_inner, n_outer, n_lev,
                                n_inner, level_index, masked_levels, stream, c);
  });
}

int smm_group_apply_sb(smm_group_t g, const void* x, int x_dtype, int64_t xs_lev, int64_t ldx, void* y, int y_dtype,
                       int64_t ys_lev, int64_t ys_batch, int64_t n_batch, int64_t n_lev, const int32_t* level_index,
                       const uint8_t* masked_levels, double remap_area_min, unsigned flags, void* stream) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_sb_impl(g, x, xs_lev, ldx, y, ys_lev, ys_batch, n_batch, n_lev, level_index,
                                   masked_levels, stream, c);
  });
}

int smm_group_apply_sb_cf(smm_group_t g, const void* x, int x_dtype, int64_t xs_lev, int64_t ldx, void* y,
                          int y_dtype, int64_t ys_lev, int64_t ys_batch, int64_t n_batch, int64_t n_lev,
                          const int32_t* level_index, const uint8_t* masked_levels, double remap_area_min,
                          unsigned flags, void* stream, const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_sb_impl(g, x, xs_lev, ldx, y, ys_lev, ys_batch, n_batch, n_lev, level_index,
                                   masked_levels, stream, c);
  });
}

int smm_group_apply_sb_pk(smm_group_t g, const void* x, int x_dtype, int64_t xs_lev, int64_t ldx, void* y,
                          int y_dtype, int64_t ys_lev, int64_t ys_batch, int64_t n_batch, int64_t n_lev,
                          const int32_t* level_index, const uint8_t* masked_levels, double remap_area_min,
                          unsigned flags, void* stream, const smm_cf_decode_t* cf, const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_group_apply_sb_impl(g, x, xs_lev, ldx, y, ys_lev, ys_batch, n_batch, n_lev, level_index,
                                   masked_levels, stream, c);
  });
}

int smm_group_apply_host(smm_group_t g, const void* x_host, int x_dtype, void* y_host, int y_dtype, int64_t n_outer,
                         int64_t n_lev, int64_t n_inner, int transpose, const int32_t* level_index,
                         const uint8_t* masked_levels, double remap_area_min, unsigned flags, int64_t chunk_outer) {
  return apply_entry(Entry::plain, x_dtype, y_dtype, remap_area_min, flags, nullptr, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_host_impl(g, x_host, y_host, n_outer, n_lev, n_inner, transpose, level_index,
                                     masked_levels, chunk_outer, c);
  });
}

int smm_group_apply_host_cf(smm_group_t g, const void* x_host, int x_dtype, void* y_host, int y_dtype,
                            int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                            const int32_t* level_index, const uint8_t* masked_levels, double remap_area_min,
                            unsigned flags, int64_t chunk_outer, const smm_cf_decode_t* cf) {
  return apply_entry(Entry::cf, x_dtype, y_dtype, remap_area_min, flags, cf, nullptr, [&](const CallDesc& c) {
    return smm_group_apply_host_impl(g, x_host, y_host, n_outer, n_lev, n_inner, transpose, level_index,
                                     masked_levels, chunk_outer, c);
  });
}

int smm_group_apply_host_pk(smm_group_t g, const void* x_host, int x_dtype, void* y_host, int y_dtype,
                            int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                            const int32_t* level_index, const uint8_t* masked_levels, double remap_area_min,
                            unsigned flags, int64_t chunk_outer, const smm_cf_decode_t* cf, const smm_cf_encode_t* enc) {
  return apply_entry(Entry::pk, x_dtype, y_dtype, remap_area_min, flags, cf, enc, [&](const CallDesc& c) {
    return smm_group_apply_host_impl(g, x_host, y_host, n_outer, n_lev, n_inner, transpose, level_index,
                                     masked_levels, chunk_outer, c);
  });
}

int smm_operator_launch_info(smm_operator_t op, int x_dtype, int64_t n_batch, unsigned flags, int* kernel,
                             int* j_per_block, int* rows_per_step, int* rows_per_block, int64_t* n_blocks,
                             int64_t* lds_bytes, int* big_operator) {
  return guarded([&] {
    return smm_operator_launch_info_impl(op, x_dtype, n_batch, flags, kernel, j_per_block, rows_per_step, rows_per_block,
                                         n_blocks, lds_bytes, big_operator);
  });
}

int smm_group_launch_info(smm_group_t g, int x_dtype, int64_t n_outer, int64_t n_lev, int64_t n_inner, unsigned flags,
                          int* kernel, int* j_per_block, int* rows_per_step, int* rows_per_block, int64_t* n_blocks,
                          int64_t* lds_bytes, int* big_operator) {
  return guarded([&] {
    return smm_group_launch_info_impl(g, x_dtype, n_outer, n_lev, n_inner, flags, kernel, j_per_block, rows_per_step,
                                      rows_per_block, n_blocks, lds_bytes, big_operator);
  });
}

int smm_operator_plan_info(smm_operator_t op, int* kernel_kind, int64_t* lds_bytes, int64_t* staged_src_elems) {
  return guarded([&] { return smm_operator_plan_info_impl(op, kernel_kind, lds_bytes, staged_src_elems); });
}

int smm_operator_export_csr(smm_operator_t op, int64_t* rowptr, int32_t* col, double* val) {
  return guarded([&] { return smm_operator_export_csr_impl(op, rowptr, col, val); });
}

}  // extern "C"
