// What the four device transcoders beside the GRIB gather share (smm_grib_aec.hip, smm_grib_aec_pack.hip,
// smm_grib_cpx.hip, smm_grib_cpx_pack.hip), each thing written once:
//   pure C++   cut_grid (a launch cut at the grid limit) and Arena (the offsets of one scratch allocation): no HIP call
//              in them, tests/cpp/grib_xcode_harness.cpp checks them on the CPU
//   device     the workgroup's place in a cut launch (row_part), prefix sums (group_scan / wave_scan, block_scan,
//              scan_parts), the packers' input (RowBits), guarded atomic min / max (lower / raise), the packers' LDS
//              windows (win_put, win_flush, zero_ends) and the unpackers' store (store_row_word)
//   host       for_grid / launch_flat, run_transcode (guard, allocation, copies up, launches, copy down, synchronise and
//              the error tidy-up) and what the entries refuse alike (check_unpack_call, check_pack_call, offsets_entry)
// The formats themselves are the text of smm_grib_aec.hpp and smm_grib_cpx.hpp.  Not part of the ABI.
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>

namespace smm_xcode {

// [0, total) cut into pieces of at most `limit` (taken into 1 .. 2^31 - 1): piece(b0, nb) in ascending order until one
// returns non-zero, which is returned.  Workgroup numbers are flat and 64-bit, so a cut may fall anywhere: a kernel
// finds its row and its part of the row from b0 + blockIdx.x (row_part below).
template <class F>
int cut_grid(int64_t total, int64_t limit, F&& piece) {
  limit = std::min<int64_t>(std::max<int64_t>(limit, 1), 0x7fffffffLL);
  for (int64_t b0 = 0; b0 < total; b0 += limit)
    if (int rc = piece(b0, (unsigned)std::min(limit, total - b0))) return rc;
  return 0;
}

// A bump arena over one allocation whose base is aligned for every member (hipMalloc's is): add<T>(count) gives the
// byte offset of `count` elements of T, aligned for T and to 16 bytes at least; bytes() is the allocation's size.
class Arena {
 public:
  template <class T>
  size_t add(size_t count) {
    constexpr size_t align = alignof(T) > 16 ? alignof(T) : 16;
    const size_t at = (end_ + align - 1) / align * align;
    end_ = at + count * sizeof(T);
    return at;
  }
  size_t bytes() const { return end_; }
  template <class T>
  static T* at(char* base, size_t off) {
    return reinterpret_cast<T*>(base + off);
  }

 private:
  size_t end_ = 0;
};

}  // namespace smm_xcode

#if defined(__HIPCC__)

#include <initializer_list>

#include "smm_device.hpp"

namespace {

using smm_xcode::Arena;
constexpr int kWave = 64;

// ------------------------------------------------------------------ device

// the row and the part of the row of this workgroup: workgroup b0 + blockIdx.x of a launch of per_row parts a row
struct RowPart {
  int64_t j;
  uint32_t part;
};
__device__ __forceinline__ RowPart row_part(int64_t b0, uint32_t per_row) {
  const int64_t id = b0 + blockIdx.x;
  return RowPart{id / per_row, (uint32_t)(id % per_row)};
}

// Inclusive prefix sum over each group of `width` (a power of two <= 64) neighbouring lanes of a wave; every lane of the
// wave calls it.  wave_scan: over the wave's 64 lanes; wave_last: the last lane's value, the sum after a wave_scan.
template <class T>
__device__ __forceinline__ T group_scan(T v, uint32_t width) {
  const uint32_t p = threadIdx.x & (width - 1u);
  for (uint32_t o = 1; o < width; o <<= 1) {
    const T up = __shfl_up(v, o, kWave);
    if (p >= o) v += up;
  }
  return v;
}
__device__ __forceinline__ uint32_t wave_scan(uint32_t v) { return group_scan(v, (uint32_t)kWave); }
__device__ __forceinline__ uint64_t wave_scan(uint64_t v) {
  return group_scan((unsigned long long)v, (uint32_t)kWave);
}
__device__ __forceinline__ uint64_t wave_last(uint64_t v) { return __shfl((unsigned long long)v, kWave - 1, kWave); }

// inclusive prefix sum over the N lanes of a workgroup through N elements of LDS; every lane of the workgroup calls it
template <int N, class T>
__device__ __forceinline__ T block_scan(T v, T* lds, uint32_t tid) {
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < N; o <<= 1) {
    const T t = (int)tid >= o ? lds[tid - o] : T(0);
    __syncthreads();
    lds[tid] += t;
    __syncthreads();
  }
  const T incl = lds[tid];
  __syncthreads();   // lds is free again
  return incl;
}

// One wave scans a run of n parts, 64 at a step with a carry: put(i, the sum of the parts before part i) for every
// part, the sum of all of them returned in every lane.  T: uint64_t, or a type with +, - and its own wave_scan /
// wave_last.  get and put see each i < n once; a put may overwrite what get(i) read.
template <class T, class I, class Get, class Put>
__device__ __forceinline__ T scan_parts(I n, Get&& get, Put&& put) {
  const uint32_t lane = threadIdx.x & (kWave - 1);
  T carry{};
  for (I i0 = 0; i0 < n; i0 += kWave) {
    const I i = i0 + lane;
    const T v = i < n ? get(i) : T{};
    const T incl = wave_scan(v);
    if (i < n) put(i, carry + incl - v);
    carry = carry + wave_last(incl);
  }
  return carry;
}

// a row's integers, read from its simple-packed stream at byte in_off of x; last_word: the index of the last word of x,
// no load goes past it
struct RowBits {
  const uint32_t* words;
  uint32_t bit0, last;
  int nbits;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const {
    return smm_grib::grib_extract(words, (uint64_t)bit0 + (uint64_t)i * (uint32_t)nbits, nbits, last);
  }
};
__device__ __forceinline__ RowBits row_bits(const uint32_t* x, uint64_t last_word, uint64_t in_off, int nbits) {
  const uint64_t w = std::min<uint64_t>(in_off >> 2, last_word);
  return RowBits{x + w, 8u * (uint32_t)(in_off & 3), (uint32_t)std::min<uint64_t>(last_word - w, 0xfffffffeull), nbits};
}

// an atomic min / max onto a word that only falls / grows: a look at it first spares the atomic that cannot change it (a
// stale look costs an atomic that changes nothing, never a missed one)
template <class T>
__device__ __forceinline__ void lower(T* at, T v) {
  if (v < __atomic_load_n(at, __ATOMIC_RELAXED)) atomicMin(at, v);
}
template <class T>
__device__ __forceinline__ void raise(T* at, T v) {
  if (v > __atomic_load_n(at, __ATOMIC_RELAXED)) atomicMax(at, v);
}

// ---- the packers' windows.  A workgroup assembles its share [first, end) of out's bits in LDS; the window's word 0 is
// the word of out that holds bit `first`.  The first and the last word of a share may hold bits of its neighbours: an
// earlier kernel zeroes them (zero_ends) and the flush ORs into them; the words between are stored whole.
// n (1..32) bits at bit `at` of the window; nothing goes past its n_words words
__device__ __forceinline__ void win_put(uint32_t* win, uint32_t n_words, uint32_t at, uint32_t v, uint32_t n) {
  const uint32_t w = at >> 5;
  const uint64_t both = (uint64_t)v << (64u - (at & 31u) - n);   // the shift is 1..63
  const uint32_t hi = (uint32_t)(both >> 32), lo = (uint32_t)both;
  if (hi != 0u && w < n_words) atomicOr(&win[w], hi);
  if (lo != 0u && w + 1u < n_words) atomicOr(&win[w + 1u], lo);
}
// the window's words to out from word w0 on, big-endian, by the THREADS lanes of the workgroup; no store goes to or
// past word out_words
template <int THREADS>
__device__ __forceinline__ void win_flush(uint32_t* out, uint64_t out_words, const uint32_t* win, uint32_t n_words,
                                          uint64_t w0, uint32_t tid) {
  for (uint32_t w = tid; w < n_words; w += THREADS) {
    const uint64_t at = w0 + w;
    if (at >= out_words) continue;
    const uint32_t word = __builtin_bswap32(win[w]);
    if (w == 0u || w == n_words - 1u)
      atomicOr(&out[at], word);
    else
      out[at] = word;
  }
}
__device__ __forceinline__ void zero_ends(uint32_t* out, uint64_t out_words, uint64_t first, uint64_t end) {
  if (end <= first) return;
  if ((first >> 5) < out_words) out[first >> 5] = 0u;
  if (((end - 1) >> 5) < out_words) out[(end - 1) >> 5] = 0u;
}

// ---- the unpackers' store.  Word w of a row's simple-packed stream of n_values values of `width` bits at byte out_off
// of out: the values that overlap the word, value(i) each, put in place as smm_grib_codec.hpp's grib_word_part has it.
// Words the values do not reach are stored as zero; a thread past the row's words, or of a row of width 0, leaves.
template <class V>
__device__ __forceinline__ void store_row_word(uint32_t* out, uint64_t out_off, uint32_t w, int width, uint32_t n_values,
                                               V&& value) {
  if (width == 0 || w >= (smm_grib::align4(smm_grib::row_bytes(n_values, width)) >> 2)) return;
  uint64_t i = 0, end = 0;
  smm_grib::grib_word_values(w, width, n_values, &i, &end);
  uint32_t word = 0;
  for (; i < end; ++i) word |= smm_grib::grib_word_part(value(i), i, width, w);
  out[(out_off >> 2) + w] = __builtin_bswap32(word);
}

// ------------------------------------------------------------------ host

// launches `total` workgroups as grids of at most grid_limit(), the first workgroup's number handed to the kernel
template <class F>
int for_grid(int64_t total, F&& launch) {
  return smm_xcode::cut_grid(total, grid_limit(), [&](int64_t b0, unsigned nb) -> int {
    launch(b0, nb);
    SMM_HIP(hipGetLastError());
    return SMM_OK;
  });
}
// kernel(a, b0, extra...) over `total` workgroups of `threads` lanes
template <class K, class A, class... X>
int launch_flat(K kernel, int threads, int64_t total, hipStream_t s, const A& a, X... extra) {
  return for_grid(total, [&](int64_t b0, unsigned nb) {
    hipLaunchKernelGGL(kernel, dim3(nb), dim3((unsigned)threads), 0, s, a, b0, extra...);
  });
}

// a piece of the arena and its copy on the host
struct Span {
  size_t off;
  void* host;
  size_t bytes;
};
// One transcoding call on the device: select it, allocate the arena, copy the `up` pieces in, launch(base, stream),
// copy the `down` piece -- the rows' `what` -- out and wait.  The arena is in use until the stream has been waited for,
// so a failed copy or launch still synchronises; the HIP error is then cleared and the first failure returned.
template <class L>
int run_transcode(int device, void* stream, size_t arena_bytes, std::initializer_list<Span> up, L&& launch, Span down,
                  const char* what) {
  DeviceGuard guard(device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the device");
  hipStream_t s = (hipStream_t)stream;
  DeviceBuf<char> d;
  SMM_HIP(d.alloc(arena_bytes));
  auto enqueue = [&]() -> int {
    for (const Span& u : up) SMM_HIP(hipMemcpyAsync(d.get() + u.off, u.host, u.bytes, hipMemcpyHostToDevice, s));
    if (int rc = launch(d.get(), s)) return rc;
    const hipError_t e = hipMemcpyAsync(down.host, d.get() + down.off, down.bytes, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) return fail(SMM_ERR_HIP, std::string("copying the rows' ") + what + ": " + hipGetErrorString(e));
    return SMM_OK;
  };
  const int rc = enqueue();
  const hipError_t e = hipStreamSynchronize(s);
  if (rc != SMM_OK) {
    (void)hipGetLastError();
    return rc;
  }
  SMM_HIP(e);
  return SMM_OK;
}

// The body of the entries that give every row its offset and the total (smm_grib_*_layout, smm_grib_*_pack_bound):
// check(recs, n_batch) refuses, row_bytes(rec) is what a row takes.  sum_rows is their loop.
template <class Rec, class B>
uint64_t sum_rows(const Rec* recs, int64_t n_batch, uint64_t* byte_off, B&& row_bytes) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (byte_off) byte_off[b] = at;
    at += row_bytes(recs[b]);
  }
  return at;
}
template <class Rec, class C, class P>
int offsets_entry(const Rec* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes, C&& check, P&& place) {
  return guarded([&] {
    if (!total_bytes) return fail(SMM_ERR_INVALID, "null total pointer");
    if (int rc = check(recs, n_batch)) return rc;
    *total_bytes = place(recs, n_batch, byte_off);
    return (int)SMM_OK;
  });
}

// What smm_grib_*_unpack refuses once its records have passed, in this order.  offs[b] = layout(recs, n_batch, offs):
// the rows' places in out, the total behind them; row(b): what the codec refuses about row b (0: nothing).
template <class Rec, class P, class R>
int check_unpack_call(const void* x, const Rec* recs, const smm_grib_row_t* rows_in, int64_t n_batch, const void* out,
                      int64_t out_bytes, const smm_grib_row_t* rows_out, std::vector<uint64_t>& offs, P&& layout, R&& row) {
  if (n_batch > 0 && (!rows_in || !rows_out)) return fail(SMM_ERR_INVALID, "null row-table pointer");
  if (out_bytes < 0) return fail(SMM_ERR_INVALID, "negative out_bytes");
  offs.resize((size_t)n_batch + 1);
  const uint64_t total = offs[(size_t)n_batch] = layout(recs, n_batch, offs.data());
  for (int64_t b = 0; b < n_batch; ++b)
    if (int rc = row(b)) return rc;
  if ((uint64_t)out_bytes < total)
    return fail(SMM_ERR_INVALID, "out_bytes " + std::to_string(out_bytes) + " is below the layout's " + std::to_string(total) + " bytes");
  if (total > 0 && (!x || !out)) return fail(SMM_ERR_INVALID, "null field or output pointer");
  if ((uintptr_t)x % 4) return fail(SMM_ERR_INVALID, "field pointer is not 4-byte aligned");
  if ((uintptr_t)out % 4) return fail(SMM_ERR_INVALID, "output pointer is not 4-byte aligned");
  return SMM_OK;
}
// rows_in[b].nbits is the width the record says
template <class Rec>
int check_row_width(const smm_grib_row_t* rows_in, const Rec* recs, int64_t b) {
  if (rows_in[b].nbits != recs[b].nbits)
    return fail(SMM_ERR_INVALID, "rows_in[" + std::to_string(b) + "].nbits differs from recs[" + std::to_string(b) + "].nbits");
  return SMM_OK;
}

// What smm_grib_*_pack refuses once its "wanted" records have passed, in this order; a record's n_values and nbits
// say which bytes of x its row reads, bound(recs, n_batch, nullptr) how many bytes out must have.
template <class Rec, class P>
int check_pack_call(const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const Rec* recs, int64_t n_batch,
                    const void* out, int64_t out_bytes, const Rec* recs_out, const uint64_t* used_bytes, P&& bound) {
  if (n_batch > 0 && (!rows_in || !recs_out)) return fail(SMM_ERR_INVALID, "null row-table or result pointer");
  if (!used_bytes) return fail(SMM_ERR_INVALID, "null used_bytes pointer");
  if (x_bytes < 0) return fail(SMM_ERR_INVALID, "negative x_bytes");
  if (out_bytes < 0) return fail(SMM_ERR_INVALID, "negative out_bytes");
  bool streams = false;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (int rc = check_row_width(rows_in, recs, b)) return rc;
    const uint64_t off = rows_in[b].byte_off, len = smm_grib::row_bytes(recs[b].n_values, recs[b].nbits);
    if (len > 0 && (off > (uint64_t)x_bytes || len > (uint64_t)x_bytes - off))
      return fail(SMM_ERR_INVALID, "rows_in[" + std::to_string(b) + "]: bytes [" + std::to_string(off) + ", " + std::to_string(off) +
                                       " + " + std::to_string(len) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes");
    streams = streams || len > 0;
  }
  const uint64_t need = bound(recs, n_batch, nullptr);
  if ((uint64_t)out_bytes < need)
    return fail(SMM_ERR_INVALID, "out_bytes " + std::to_string(out_bytes) + " is below the bound of " + std::to_string(need) + " bytes");
  if (streams && (!x || !out)) return fail(SMM_ERR_INVALID, "null field or output pointer");
  if ((uintptr_t)x % 4) return fail(SMM_ERR_INVALID, "field pointer is not 4-byte aligned");
  if ((uintptr_t)out % 4) return fail(SMM_ERR_INVALID, "output pointer is not 4-byte aligned");
  return SMM_OK;
}

}  // namespace

#endif  // __HIPCC__
