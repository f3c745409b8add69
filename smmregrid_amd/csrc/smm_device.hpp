// What the translation units of the device side share (smm_device.hip: the float / packed / half apply paths and the
// handles' lifetime; smm_grib_host.hip: the GRIB entries): the handles, the status and error plumbing, the checks every
// apply entry makes and the host-buffer pipeline.  Not part of the ABI.  Everything in the unnamed namespace is stateless;
// process-wide state -- the thread's error text, the tuning knobs, the grid limit, the fail-at-chunk hook and the host
// statistics -- is defined once, in smm_device.hip, and reached through the functions declared in namespace smm.
#pragma once

#include <hip/hip_runtime.h>

#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstring>
#include <map>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "smm_internal.h"
#include "smm_devmem.hpp"
#include "smm_grib.hpp"
#include "smm_grib_codec.hpp"
#include "smm_launch.hpp"

using smm::DeviceBuf;   // every HBM / page-locked block the library owns (smm_devmem.hpp)
using smm::PinnedBuf;

namespace smm {
// smm_launch.hpp declares fail_msg (sets the thread's error text, returns code) and tuning
int64_t grid_limit();        // largest 1-D launch grid (workgroups); smm_debug_set_grid_limit lowers it so that tests reach the split path
int64_t test_fail_chunk();   // smm_debug_fail_at_chunk: chunk c of the next host-pipeline calls fails; -1 (the default) = off
void add_host_stats(const double* v);   // one call's SMM_HOST_STAT_COUNT figures into the process's sums (smm_debug_host_stats)
// Validates (level_index, masked_levels) against the group and returns the device copy of that configuration, uploading
// it on first sight.  Entries live until smm_group_destroy.
int group_level_cfg(smm_group* g, int64_t n_lev, const int32_t* level_index, const uint8_t* masked_levels,
                    double remap_area_min, unsigned flags, const int32_t** d_map, const uint8_t** d_masked);
}

namespace {

inline int fail(int code, const std::string& msg) { return smm::fail_msg(code, msg); }
using smm::grid_limit;
using smm::test_fail_chunk;
using smm::group_level_cfg;

inline int check_area_min(double area_min) {
  if (!(area_min >= 0.0 && area_min <= 1.0))
    return fail(SMM_ERR_INVALID, "remap_area_min must be within [0, 1]");  // regrid.py:124-125
  return SMM_OK;
}

#define SMM_HIP(call)                                                                   \
  do {                                                                                  \
    hipError_t e_ = (call);                                                             \
    if (e_ != hipSuccess) {                                                             \
      (void)hipGetLastError();                                                          \
      return fail(e_ == hipErrorNoDevice || e_ == hipErrorInvalidDevice                 \
                      ? SMM_ERR_NO_DEVICE                                               \
                      : SMM_ERR_HIP,                                                    \
                  std::string(#call) + ": " + hipGetErrorString(e_));                   \
    }                                                                                   \
  } while (0)

}  // namespace

// Staging resources of the host-buffer pipeline, cached per operator (allocation costs
// milliseconds, a small regrid microseconds): two streams, two device X/Y chunk buffers,
// two pinned X/Y staging buffers, grown on demand.
struct HostPipe {
  hipStream_t stream[2] = {nullptr, nullptr};
  DeviceBuf<char> dx[2], dy[2];
  PinnedBuf hx[2], hy[2];
  // per buffer: before the H2D, after it, after the kernel(s), after the D2H -- the stage times of a chunk
  // (smm_debug_host_stats) are read from them once the chunk has been drained
  hipEvent_t ev[2][4] = {{nullptr, nullptr, nullptr, nullptr}, {nullptr, nullptr, nullptr, nullptr}};
  hipError_t ensure(size_t need_dx, size_t need_dy, size_t need_hx, size_t need_hy) {
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && e == hipSuccess; ++i)
      if (!stream[i]) e = hipStreamCreateWithFlags(&stream[i], hipStreamNonBlocking);
    for (int i = 0; i < 2; ++i)
      for (int k = 0; k < 4 && e == hipSuccess; ++k)
        if (!ev[i][k]) e = hipEventCreate(&ev[i][k]);
    // a pair's capacity is that of its smaller buffer: zero after a failed allocation (alloc frees first)
    auto grow = [&](auto(&buf)[2], size_t need) {
      if (need <= std::min(buf[0].bytes(), buf[1].bytes())) return;
      for (int i = 0; i < 2 && e == hipSuccess; ++i) e = buf[i].alloc(need);
    };
    grow(dx, need_dx);
    grow(dy, need_dy);
    grow(hx, need_hx);
    grow(hy, need_hy);
    return e;
  }
  hipError_t mark(int b, int k) { return hipEventRecord(ev[b][k], stream[b]); }   // stage boundary k of buffer b
  // After a failed chunk: wait for whatever is still queued on both streams (an async D2H into the
  // caller's Y of the previous chunk), so that nothing writes into caller memory after the return.
  void quiesce() {
    for (int i = 0; i < 2; ++i)
      if (stream[i]) (void)hipStreamSynchronize(stream[i]);
    (void)hipGetLastError();
  }
  ~HostPipe() {
    for (int i = 0; i < 2; ++i) {
      if (stream[i]) (void)hipStreamDestroy(stream[i]);
      for (int k = 0; k < 4; ++k)
        if (ev[i][k]) (void)hipEventDestroy(ev[i][k]);
    }
  }
};

// ------------------------------------------------------------------ handles

constexpr int kNumShapes = 5;
constexpr int shape_rows(int which) { return which == 0 ? 256 : (64 >> (which - 1)); }

// Device buffers of the GRIB entries of one handle (an operator or a group), grown on demand.  The device entries, under
// mu (calls on one handle take turns filling them): the call's row table, and when some row has a bitmap the rows' bitmap
// records and the rank tables of the bitmapped ones with their segment totals behind them.  The host entries, under the
// handle's pipe_mu: the device-only rank buffer of each pipeline slot.
struct GribState {
  std::mutex mu;
  DeviceBuf<smm_grib_row_t> d_rows;
  DeviceBuf<GribRowBitmap> d_bm;
  DeviceBuf<char> d_rank, d_pipe_rank[2];
  // smm_apply_host_grib_pk, per pipeline slot: the chunk's packed result (records, then slots) and the pack's scratch
  DeviceBuf<char> d_pipe_pk[2], d_pipe_scratch[2];
};

struct smm_operator {
  int device = -1;
  smm::HostCsr csr;          // canonical: row = destination cell
  int64_t pruned_links = 0;  // exact-zero links dropped at create time (SMM_CREATE_PRUNE_ZEROS)
  int64_t n_slices = 0, n_slots = 0;
  DeviceBuf<int64_t> d_slice_off;
  DeviceBuf<int32_t> d_col;
  DeviceBuf<double> d_val;
  DeviceBuf<int32_t> d_rowlen;
  // smm_operator_create_cols: weight columns 1 .. n_cols - 1 (gradient weights; column 0 is csr.val / d_val and every
  // other entry sees that alone) -- per column the values of the canonical CSR's links, and on the device SELL slot
  // planes of n_slots each beside d_val, padded slots +0.0 (smm_apply_cols)
  int n_cols = 1;
  std::vector<std::vector<double>> csr_xval;
  DeviceBuf<double> d_xval;
  DeviceBuf<uint8_t> d_imask;
  DeviceBuf<double> d_frac;
  // LDS tile plans by block shape: [0] = 4 slices (256 rows) per block, [1] = 1 slice (heavy rows),
  // [2..4] = 32 / 16 / 8 rows of a slice (rows so long -- high-resolution source, coarse target --
  // that a whole slice's footprint exceeds the LDS budget).  The operator's own shape is built at
  // create time, the others on demand when it joins a group of another shape.
  struct TilePlan {
    bool built = false, valid = false;
    int64_t max_chunks = 0, total_chunks = 0, total_lines = 0;
    bool preferred = false;  // staged lines are used well enough to beat direct gathers
    bool reuse = false;      // some staged lines are shared by several blocks (keep them cacheable)
    DeviceBuf<int64_t> d_blk_chunk_off;
    DeviceBuf<int32_t> d_chunk_src;
    DeviceBuf<int32_t> d_lcol;
    DeviceBuf<uint8_t> d_blk_direct;
  } plan[kNumShapes];
  smm::HostSell sell_shape;  // slice_off / rowlen only (col/val dropped after upload)
  std::mutex plan_mu;
  std::mutex pipe_mu;        // smm_apply_host calls on one operator take turns
  HostPipe pipe;
  // plain canonical CSR on the device for the batch-fastest kernel, uploaded on first use
  bool sb_ready = false;
  std::vector<int32_t> h_used;        // ascending used source cells (host pack of the pipeline)
  DeviceBuf<int64_t> d_csr_rowptr;
  DeviceBuf<int32_t> d_csr_col;       // source cell
  DeviceBuf<int32_t> d_csr_colp;      // rank of the source cell among the used cells (packed X)
  DeviceBuf<double> d_csr_val;
  GribState grib;            // smm_apply_grib(_bm) / smm_apply_host_grib(_bm)
  std::atomic<int> group_refs{0};  // groups borrowing this operator (their descriptors hold its device pointers)
  int native = 0;            // shape of the operator's own plan (choose_native_plan)
  int native_plan() const { return native; }
  DeviceBuf<LevelDesc> d_desc;  // one-element device copy (native plan)
  LevelDesc desc(int which) const {
    LevelDesc L;
    L.slice_off = d_slice_off.get();
    L.col = d_col.get();
    L.val = d_val.get();
    L.rowlen = d_rowlen.get();
    L.imask = d_imask.get();
    L.frac = d_frac.get();
    L.blk_chunk_off = plan[which].d_blk_chunk_off.get();
    L.chunk_src = plan[which].d_chunk_src.get();
    L.lcol = plan[which].d_lcol.get();
    L.blk_direct = plan[which].d_blk_direct.get();
    return L;
  }
};

struct smm_group {
  int device = -1;
  std::vector<smm_operator_t> ops;
  DeviceBuf<LevelDesc> d_descs;
  int tile_which = 0;  // plan shape shared by all members
  bool tile_valid = false;
  bool tile_preferred = false;
  bool tile_reuse = false;
  int64_t tile_max_chunks = 0;
  int64_t max_row_nnz = 0;
  // uploaded (level_index, masked_levels) configurations, keyed by content.  An entry lives until
  // smm_group_destroy: a kernel enqueued by another thread may still read it, so nothing is ever
  // evicted (an entry is n_lev * 4 + n_ops bytes; callers cycle through a few level subsets).
  std::mutex mu;
  std::map<std::string, DeviceBuf<char>> cfg_cache;
  std::mutex pipe_mu;  // smm_group_apply_host calls on one group take turns
  HostPipe pipe;
  GribState grib;      // smm_group_apply_grib / smm_group_apply_host_grib
};

namespace {

struct DeviceGuard {
  int prev = -1;
  bool ok = false;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) {
      (void)hipGetLastError();
      return;
    }
    if (prev == dev) {
      ok = true;
      return;
    }
    ok = hipSetDevice(dev) == hipSuccess;
  }
  ~DeviceGuard() {
    if (ok && prev >= 0) (void)hipSetDevice(prev);
  }
};

// Staging stages of the two host pipelines (smm_hostpool.cpp: one persistent worker pool, nothing throws):
// their int results become statuses here.
int stage_status(int rc, const char* what) {
  if (rc == 0) return SMM_OK;
  return fail(rc == 1 ? SMM_ERR_ALLOC : SMM_ERR_INTERNAL,
              std::string(what) + (rc == 1 ? ": out of host memory in a staging task" : ": a staging task failed"));
}
int host_copy(void* dst, const void* src, size_t bytes) { return stage_status(smm::host_copy(dst, src, bytes), "host copy"); }

inline double wall_ms() {
  return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// one call's share: host-side stages by the wall clock of the calling thread, device-side stages from the
// chunk's four events once its stream has been synchronised
struct CallStats {
  double v[SMM_HOST_STAT_COUNT] = {};
  double t_call = wall_ms();
  void chunk_done(HostPipe& pipe, int b) {
    float ms = 0.f;
    if (hipEventElapsedTime(&ms, pipe.ev[b][0], pipe.ev[b][1]) == hipSuccess) v[SMM_HOST_STAT_H2D_MS] += ms;
    if (hipEventElapsedTime(&ms, pipe.ev[b][1], pipe.ev[b][2]) == hipSuccess) v[SMM_HOST_STAT_KERNEL_MS] += ms;
    if (hipEventElapsedTime(&ms, pipe.ev[b][2], pipe.ev[b][3]) == hipSuccess) v[SMM_HOST_STAT_D2H_MS] += ms;
    (void)hipGetLastError();
    v[SMM_HOST_STAT_CHUNKS] += 1;
  }
  ~CallStats() {
    v[SMM_HOST_STAT_CALLS] = 1;
    v[SMM_HOST_STAT_TOTAL_MS] = wall_ms() - t_call;
    smm::add_host_stats(v);
  }
};
struct StageTimer {   // adds the scope's wall time to one entry
  double& acc;
  double t0 = wall_ms();
  explicit StageTimer(double& a) : acc(a) {}
  ~StageTimer() { acc += wall_ms() - t0; }
};

bool is_pinned(const void* p) {
  hipPointerAttribute_t attr;
  if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
    (void)hipGetLastError();
    return false;
  }
  return attr.type == hipMemoryTypeHost;
}

// The loop both host pipelines share; chunk c runs in buffer c & 1.  launch(c, b) stages chunk c, enqueues its H2D, its
// kernels and its D2H on pipe.stream[b] and marks the four stage boundaries between them (pipe.mark: the first lies
// between the host staging and the H2D, so the marks cannot sit out here); deliver(c, b) copies the chunk's results out
// of the pinned buffer once its stream has drained.  Buffer b is free again once chunk c-2 has been delivered.  Any
// failure first waits for the copies still in flight into the caller's buffers (chunk c-1's D2H) before it is returned.
template <typename Launch, typename Deliver>
int run_host_pipeline(HostPipe& pipe, int64_t n_chunks, CallStats& st, Launch&& launch, Deliver&& deliver) {
  auto drain = [&](int64_t c) -> int {
    const int b = (int)(c & 1);
    {
      StageTimer t(st.v[SMM_HOST_STAT_WAIT_MS]);
      SMM_HIP(hipStreamSynchronize(pipe.stream[b]));
    }
    st.chunk_done(pipe, b);
    return deliver(c, b);
  };
  const int64_t fail_at = test_fail_chunk();
  auto loop = [&]() -> int {
    for (int64_t c = 0; c < n_chunks; ++c) {
      if (c >= 2)
        if (int rc = drain(c - 2)) return rc;
      if (c == fail_at) return fail(SMM_ERR_HIP, "injected failure (smm_debug_fail_at_chunk)");
      if (int rc = launch(c, (int)(c & 1))) return rc;
    }
    for (int64_t c = std::max<int64_t>(0, n_chunks - 2); c < n_chunks; ++c)
      if (int rc = drain(c)) return rc;
    return SMM_OK;
  };
  const int rc = loop();
  if (rc) pipe.quiesce();   // keeps the thread's error message of the first failure
  return rc;
}

// Every extern "C" entry that can reach an allocation runs its body through this: the header promises an int
// status, never an exception.  (fail() assigns a std::string and may itself run out of memory: then the status
// alone has to do.)
template <typename F>
int guarded(F&& body) noexcept {
  try {
    return body();
  } catch (const std::bad_alloc&) {
    try {
      return fail(SMM_ERR_ALLOC, "out of host memory");
    } catch (...) {
      return SMM_ERR_ALLOC;
    }
  } catch (const std::exception& e) {
    try {
      return fail(SMM_ERR_INTERNAL, std::string("unexpected failure: ") + e.what());
    } catch (...) {
      return SMM_ERR_INTERNAL;
    }
  } catch (...) {
    try {
      return fail(SMM_ERR_INTERNAL, "unexpected failure (unknown exception)");
    } catch (...) {
      return SMM_ERR_INTERNAL;
    }
  }
}

// apply flags the ABI defines; anything else (ABI v4 callers encoded kernel variants in bits 16..23) is refused
constexpr unsigned kApplyFlagMask = SMM_APPLY_MASKED | SMM_APPLY_NO_FILL | SMM_APPLY_SB_PACKED | SMM_APPLY_HOST_NO_PACK |
                                    SMM_APPLY_SB_Y_SB | SMM_APPLY_SKIPNA | SMM_APPLY_KERNEL_SELL |
                                    SMM_APPLY_KERNEL_TILE;
inline int check_flags(unsigned flags) {
  if (flags & ~kApplyFlagMask)
    return fail(SMM_ERR_INVALID, "unknown apply flag bits 0x" + [](unsigned v) {
             char buf[16];
             snprintf(buf, sizeof(buf), "%x", v);
             return std::string(buf);
           }(flags & ~kApplyFlagMask) + " (launch-shape knobs are smm_debug_set_tuning entries, not flags)");
  if ((flags & SMM_APPLY_SKIPNA) && (flags & SMM_APPLY_NO_FILL))
    return fail(SMM_ERR_INVALID, "SMM_APPLY_SKIPNA tests every source value: it cannot take SMM_APPLY_NO_FILL");
  return SMM_OK;
}

// ---- what an apply refuses about its epilogue and its levels, written once for every entry (check_area_min is with
// check_x_dtype).  what: "the operator" or "a level"
inline int check_epilogue(const smm_operator* op, bool masked, double area_min, const char* what) {
  if (masked && !op->d_imask.get())
    return fail(SMM_ERR_INVALID, std::string("masked apply requested but ") + what + " has no dst_imask");
  if (area_min > 0.0 && !op->d_frac.get())
    return fail(SMM_ERR_INVALID, std::string("remap_area_min > 0 requested but ") + what + " has no dst_frac");
  return SMM_OK;
}
// member w of a group takes the masked epilogue: the call asks for it and the member is not exempt (regrid.py:405)
inline bool level_masked(unsigned flags, const uint8_t* masked_levels, int w) {
  return (flags & SMM_APPLY_MASKED) && (!masked_levels || masked_levels[w]);
}
// Every selected level of a group call, before anything is uploaded or launched: a later level's missing dst_imask /
// dst_frac must not surface after earlier levels have written part of Y.  flags 0 and area_min 0 ask about level_index only.
inline int check_levels(const smm_group* g, int64_t n_lev, const int32_t* level_index, const uint8_t* masked_levels,
                        double area_min, unsigned flags) {
  if (n_lev > 0 && !level_index) return fail(SMM_ERR_INVALID, "null level_index");
  for (int64_t l = 0; l < n_lev; ++l) {
    const int w = level_index[l];
    if (w < 0 || w >= (int)g->ops.size())
      return fail(SMM_ERR_INVALID, "level_index[" + std::to_string(l) + "]=" + std::to_string(w) + " outside the group");
    if (int rc = check_epilogue(g->ops[(size_t)w], level_masked(flags, masked_levels, w), area_min, "a level")) return rc;
  }
  return SMM_OK;
}
inline size_t free_device_bytes() {   // 0 when it cannot be told (the error is cleared)
  size_t free_b = 0, total_b = 0;
  if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) return free_b;
  (void)hipGetLastError();
  return 0;
}

}  // namespace
