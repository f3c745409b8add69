// smm_grib_cpx_pack (gfx950): simple-packed streams on the device coded as the complex-packed streams of GRIB-2
// templates 5.2 / 5.3 -- the mirror of smm_grib_cpx_unpack -- and the two host-only entries beside it
// (smm_grib_cpx_pack_bound, smm_grib_cpx_encode_host).  THE RULE OF THIS ENCODER is the text of smm_grib_cpx.hpp; the
// kernels take a row's order with its decide(), a value's z with its z_of() and a row's record with its coded_row(): what
// encode_row writes on the host they write byte for byte.  A row is cut into tiles of 1024 values; 1024, 256 and 64 are
// multiples of every group length L, so a group lies in one wave and in one tile.  Seven kernels in stream order -- a
// kernel boundary is the only ordering between passes:
//   diff     a lane per value: X and its one or two predecessors from the simple-packed stream's bits, d; min d and
//            max d reduced over the wave by shuffles, then at most one 64-bit atomic min / max per wave onto the row's
//            pair (the word is looked at first)
//   decide   a thread per row: rule 1 -- the effective order, g, n_oct
//   groups   a lane per value again: z, its group's min and max over L lanes by shuffles -> ref_g, w_g; a workgroup scan
//            of w_g L_g gives every group its bit offset in the tile (8 B per group), the tile its bits; the extremes of
//            ref_g and w_g go to the row by one 32-bit atomic per wave
//   rows     a wave per row scans its tiles' bits, 64 at a step: tile offsets, the three table widths, the row's record
//   layout   one wave scans the rows' lengths, 64 at a step: each row's 4-byte-aligned place in out, the bytes used
//   edges    a thread per tile zeroes the words its part of the references, the widths and the data bits may share with
//            its neighbours (the first and the last of each), tile 0 also the descriptors' words
//   emit     a workgroup per tile assembles its references, stored widths and data bits in three LDS windows (z is
//            recomputed: three extracts from lines the groups kernel just read, rather than 4 B per value of scratch),
//            stores the whole words big-endian and ORs the shared ones onto the zeros
// Vector stores and vector atomics (LDS OR, global OR / min / max) only.  They commute: the bytes do not depend on the
// order.  Every bit position is 64-bit; no store goes to or past out_words, no load past the last word of x.
#include "smm_device.hpp"

#include <algorithm>

#include "smm_grib_cpx.hpp"

namespace {

constexpr int kWave = 64;
constexpr int kPackThreads = 256;
constexpr int kPerLane = 4;
constexpr uint32_t kTile = kPackThreads * kPerLane;       // values of a tile
constexpr uint32_t kTileGroups = kTile / 8;           // groups of a tile at the shortest group length
constexpr uint32_t kDataWords = kTile + 2;            // a tile's data bits: 1024 values of 32 bits, begun anywhere in a word
constexpr uint32_t kRefWords = kTileGroups + 2;       // its references: 128 of 32 bits
constexpr uint32_t kWidthWords = kTileGroups * 6 / 32 + 2;   // its stored widths: 128 of 6 bits
constexpr uint32_t kHeadWords = 4;                    // three descriptors of 4 octets, from a word's start
constexpr unsigned long long kBias = 1ull << 40;      // d + kBias > 0: |d| < 2^34

struct PackRow {          // what a row of the call brings to the device; 48 B
  uint64_t in_off;        // the row's simple-packed stream in x, bytes
  uint64_t group_off;     // the row's first group record
  uint64_t tile_off;      // the row's first tile record
  uint32_t n_values, n_groups, n_tiles, L;   // nbits == 0: all three are 0, nothing is done
  int32_t nbits, order;   // the input width, the wanted order
};
static_assert(sizeof(PackRow) == 48, "a plain table, 8-byte aligned");
struct RowStats {         // reduced by atomics; the host sets the identities
  unsigned long long dmin, dmax;   // of d + kBias
  uint32_t ref_max, w_min, w_max, pad;
};
struct PackArgs {
  const uint32_t* x;
  uint64_t last_word;     // index of the last word of x: no load goes past it
  const PackRow* rows;
  RowStats* stats;
  smm_cpx::Decision* plans;   // per row, from the decide kernel
  smm_cpx::Row* recs;         // per row: the record of the stream (rows kernel; byte_off: layout kernel)
  uint2* groups;          // per group: ref_g, w_g | bit offset in the tile << 8
  uint32_t* tile_bits;    // per tile: its data bits
  uint64_t* tile_at;      // per tile: its first data bit in the row's data part
  uint64_t* used;         // the bytes used
  uint32_t* out;
  uint64_t out_words;     // no store goes to or past this word of out
};

// the row's integers, read from its simple-packed stream
struct RowBits {
  const uint32_t* words;
  uint32_t bit0, last;
  int nbits;
  __device__ __forceinline__ uint32_t operator()(uint32_t i) const {
    return smm_grib::grib_extract(words, (uint64_t)bit0 + (uint64_t)i * (uint32_t)nbits, nbits, last);
  }
};
__device__ __forceinline__ RowBits row_bits(const PackArgs& a, const PackRow& r) {
  const uint64_t w = std::min<uint64_t>(r.in_off >> 2, a.last_word);
  return RowBits{a.x + w, 8u * (uint32_t)(r.in_off & 3), (uint32_t)std::min<uint64_t>(a.last_word - w, 0xfffffffeull), r.nbits};
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
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// inclusive prefix sum over the 256 lanes of a workgroup through LDS; every lane of the workgroup calls it
__device__ __forceinline__ uint32_t block_scan(uint32_t v, uint32_t* lds, uint32_t tid) {
  lds[tid] = v;
  __syncthreads();
#pragma unroll
  for (int o = 1; o < kPackThreads; o <<= 1) {
    const uint32_t t = (int)tid >= o ? lds[tid - o] : 0u;
    __syncthreads();
    lds[tid] += t;
    __syncthreads();
  }
  const uint32_t incl = lds[tid];
  __syncthreads();
  return incl;
}

// ---- 1: diff.  Workgroup (row, tile); only rows whose wanted order can hold (order > 0, n > order) take part.
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_diff_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const int64_t id = b0 + blockIdx.x;
  const int64_t j = id / per_row;
  const uint32_t tile = (uint32_t)(id % per_row), tid = threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || r.order <= 0 || r.n_values <= (uint32_t)r.order || tile >= r.n_tiles) return;
  const RowBits q = row_bits(a, r);
  unsigned long long lo = ~0ull, hi = 0ull;
#pragma unroll
  for (int p = 0; p < kPerLane; ++p) {
    const uint32_t i = tile * kTile + (uint32_t)p * kPackThreads + tid;
    if (i < r.n_values && i >= (uint32_t)r.order) {
      const unsigned long long d = (unsigned long long)(smm_cpx::difference(q, i, r.order) + (int64_t)kBias);
      lo = d < lo ? d : lo;
      hi = d > hi ? d : hi;
    }
  }
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const unsigned long long l2 = __shfl_xor(lo, o, kWave), h2 = __shfl_xor(hi, o, kWave);
    lo = l2 < lo ? l2 : lo;
    hi = h2 > hi ? h2 : hi;
  }
  if (tid % kWave == 0 && lo <= hi) {
    lower(&a.stats[j].dmin, lo);
    raise(&a.stats[j].dmax, hi);
  }
}

// ---- 2: decide.  A thread per row.
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_decide_kernel(PackArgs a, int64_t n_j) {
  const int64_t j = (int64_t)blockIdx.x * kPackThreads + threadIdx.x;
  if (j >= n_j) return;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  smm_cpx::Decision dec{0, 0, 0};
  if (r.nbits != 0 && r.order > 0 && r.n_values > (uint32_t)r.order) {
    const RowBits q = row_bits(a, r);
    const RowStats st = a.stats[j];
    dec = smm_cpx::decide(r.n_values, r.order, q(0), r.order > 1 ? q(1) : 0u, (int64_t)(st.dmin - kBias), (int64_t)(st.dmax - kBias));
  }
  a.plans[j] = dec;
}

// ---- 3: groups.  Workgroup (row, tile).  Lanes past the row's end hold the identities: the shuffles stay whole.
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_groups_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t s_ref[kTileGroups], s_w[kTileGroups], lds[kPackThreads];
  const int64_t id = b0 + blockIdx.x;
  const int64_t j = id / per_row;
  const uint32_t tile = (uint32_t)(id % per_row), tid = threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || tile >= r.n_tiles) return;
  const smm_cpx::Decision dec = a.plans[j];
  const RowBits q = row_bits(a, r);
  const uint32_t L = r.L, per_tile = kTile / L;
#pragma unroll
  for (int p = 0; p < kPerLane; ++p) {
    const uint32_t in_tile = (uint32_t)p * kPackThreads + tid, i = tile * kTile + in_tile;
    const bool valid = i < r.n_values;
    const uint32_t z = valid ? smm_cpx::z_of(q, i, dec) : 0u;
    uint32_t lo = valid ? z : 0xffffffffu, hi = z;
    for (uint32_t o = L >> 1; o > 0; o >>= 1) {
      lo = umin32(lo, __shfl_xor(lo, (int)o, kWave));
      hi = umax32(hi, __shfl_xor(hi, (int)o, kWave));
    }
    if (tid % L == 0) {   // a group whose first value is past the end does not exist
      s_ref[in_tile / L] = valid ? lo : 0u;
      s_w[in_tile / L] = valid ? (uint32_t)smm_cpx::bit_length(hi - lo) : 0u;
    }
  }
  __syncthreads();
  const uint32_t g = tile * per_tile + tid;
  const bool exists = tid < per_tile && g < r.n_groups;
  const uint32_t ref = exists ? s_ref[tid] : 0u, w = exists ? s_w[tid] : 0u;
  const uint32_t len = exists ? umin32(L, r.n_values - g * L) : 0u, bits = w * len;
  const uint32_t incl = block_scan(bits, lds, tid);
  if (exists) a.groups[r.group_off + g] = make_uint2(ref, w | ((incl - bits) << 8));   // the offset is below 2^15
  if (tid == kPackThreads - 1) a.tile_bits[r.tile_off + tile] = incl;
  uint32_t ref_max = ref, w_min = exists ? w : 64u, w_max = w;
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    ref_max = umax32(ref_max, __shfl_xor(ref_max, o, kWave));
    w_min = umin32(w_min, __shfl_xor(w_min, o, kWave));
    w_max = umax32(w_max, __shfl_xor(w_max, o, kWave));
  }
  if (tid % kWave == 0 && tid < per_tile) {
    raise(&a.stats[j].ref_max, ref_max);
    lower(&a.stats[j].w_min, w_min);
    raise(&a.stats[j].w_max, w_max);
  }
}

// ---- 4: rows.  A wave per row: the exclusive scan of its tiles' bits, 64 at a step, and the row's record.
__global__ __launch_bounds__(kWave) void smm_grib_cpx_rows_kernel(PackArgs a, int64_t b0) {
  const int64_t j = b0 + blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  unsigned long long carry = 0;
  for (uint32_t t0 = 0; t0 < r.n_tiles; t0 += kWave) {
    const uint32_t t = t0 + lane;
    const unsigned long long v = t < r.n_tiles ? a.tile_bits[r.tile_off + t] : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, kWave);
      if ((int)lane >= o) incl += up;
    }
    if (t < r.n_tiles) a.tile_at[r.tile_off + t] = carry + incl - v;
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) {
    smm_cpx::Row rec{};
    rec.n_values = r.n_values;
    if (r.nbits != 0 && r.n_values != 0) {
      const RowStats st = a.stats[j];
      rec = smm_cpx::coded_row(r.n_values, r.L, a.plans[j], st.ref_max, st.w_min, st.w_max, carry);
    }
    a.recs[j] = rec;
  }
}

// ---- 5: layout.  One wave: rows back to back in row order, each at a 4-byte-aligned offset.
__global__ __launch_bounds__(kWave) void smm_grib_cpx_layout_kernel(PackArgs a, int64_t n_j) {
  const uint32_t lane = threadIdx.x;
  unsigned long long carry = 0;
  for (int64_t b0 = 0; b0 < n_j; b0 += kWave) {
    const int64_t b = b0 + lane;
    const unsigned long long v = b < n_j ? smm_grib::align4(a.recs[b].byte_len) : 0ull;
    unsigned long long incl = v;
#pragma unroll
    for (int o = 1; o < kWave; o <<= 1) {
      const unsigned long long up = __shfl_up(incl, o, kWave);
      if ((int)lane >= o) incl += up;
    }
    if (b < n_j) a.recs[b].byte_off = carry + incl - v;
    carry += __shfl(incl, kWave - 1, kWave);
  }
  if (lane == 0) *a.used = carry;
}

// where a tile's share of the three parts lies in out, as bit positions counted from out's first bit: [first, end) each
struct TileBits {
  uint64_t refs0, refs1, widths0, widths1, data0, data1;
  uint32_t g0;   // the tile's first group
};
__device__ __forceinline__ TileBits tile_bits_of(const PackArgs& a, const PackRow& r, const smm_cpx::Row& rec, uint32_t tile) {
  const smm_cpx::Sections sec = smm_cpx::sections(rec);
  const uint32_t per_tile = kTile / r.L, g0 = tile * per_tile, g1 = umin32(r.n_groups, g0 + per_tile);
  TileBits t;
  t.g0 = g0;
  t.refs0 = sec.refs_bit + (uint64_t)g0 * (uint64_t)rec.nbits;
  t.refs1 = sec.refs_bit + (uint64_t)g1 * (uint64_t)rec.nbits;
  t.widths0 = sec.widths_bit + (uint64_t)g0 * (uint64_t)rec.width_bits;
  t.widths1 = sec.widths_bit + (uint64_t)g1 * (uint64_t)rec.width_bits;
  t.data0 = sec.data_bit + a.tile_at[r.tile_off + tile];
  t.data1 = t.data0 + a.tile_bits[r.tile_off + tile];
  return t;
}
__device__ __forceinline__ uint32_t head_words(const smm_cpx::Row& rec) {
  return rec.order > 0 ? ((uint32_t)(rec.order + 1) * (uint32_t)rec.n_oct + 3u) / 4u : 0u;
}

// ---- 6: edges.  A thread per tile.  A row begins and ends on a word of its own; inside it every part begins on an
// octet, so the first and the last word of a tile's share of a part may hold bits of its neighbours: they are zeroed
// here and ORed into by the emit kernel, as are the words of the descriptors.
__device__ __forceinline__ void zero_ends(const PackArgs& a, uint64_t first, uint64_t end) {
  if (end <= first) return;
  if ((first >> 5) < a.out_words) a.out[first >> 5] = 0u;
  if (((end - 1) >> 5) < a.out_words) a.out[(end - 1) >> 5] = 0u;
}
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_edges_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const int64_t id = b0 + blockIdx.x;
  const int64_t j = id / per_row;
  const uint32_t tile = (uint32_t)(id % per_row) * kPackThreads + threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || tile >= r.n_tiles) return;
  const smm_cpx::Row rec = a.recs[j];
  const TileBits t = tile_bits_of(a, r, rec, tile);
  zero_ends(a, t.refs0, t.refs1);
  zero_ends(a, t.widths0, t.widths1);
  zero_ends(a, t.data0, t.data1);
  if (tile == 0u)
    for (uint32_t w = 0; w < head_words(rec); ++w)
      if ((rec.byte_off >> 2) + w < a.out_words) a.out[(rec.byte_off >> 2) + w] = 0u;
}

// ---- 7: emit.  A workgroup per tile.  A window's word 0 is the word of out that holds the first bit of the tile's
// share.  n (1..32) bits at bit `at` of a window; nothing goes past its n_words words.
__device__ __forceinline__ void win_put(uint32_t* win, uint32_t n_words, uint32_t at, uint32_t v, uint32_t n) {
  const uint32_t w = at >> 5;
  const uint64_t both = (uint64_t)v << (64u - (at & 31u) - n);   // the shift is 1..63
  const uint32_t hi = (uint32_t)(both >> 32), lo = (uint32_t)both;
  if (hi != 0u && w < n_words) atomicOr(&win[w], hi);
  if (lo != 0u && w + 1u < n_words) atomicOr(&win[w + 1u], lo);
}
// words of a window whose share is [first, end), cut to the window
__device__ __forceinline__ uint32_t win_words(uint64_t first, uint64_t end, uint32_t cap) {
  if (end <= first) return 0u;
  const uint64_t n = ((first & 31u) + (end - first) + 31u) / 32u;
  return n < cap ? (uint32_t)n : cap;
}
// the window's words to out: whole words stored, the first and the last ORed onto the zeros
__device__ __forceinline__ void win_flush(const PackArgs& a, const uint32_t* win, uint32_t n_words, uint64_t w0, uint32_t tid) {
  for (uint32_t w = tid; w < n_words; w += kPackThreads) {
    const uint64_t at = w0 + w;
    if (at >= a.out_words) continue;
    const uint32_t word = __builtin_bswap32(win[w]);
    if (w == 0u || w == n_words - 1u)
      atomicOr(&a.out[at], word);
    else
      a.out[at] = word;
  }
}
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_emit_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t win_d[kDataWords], win_r[kRefWords], win_w[kWidthWords], win_h[kHeadWords];
  const int64_t id = b0 + blockIdx.x;
  const int64_t j = id / per_row;
  const uint32_t tile = (uint32_t)(id % per_row), tid = threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || tile >= r.n_tiles) return;
  const smm_cpx::Row rec = a.recs[j];
  const smm_cpx::Decision dec = a.plans[j];
  const TileBits t = tile_bits_of(a, r, rec, tile);
  const uint32_t n_d = win_words(t.data0, t.data1, kDataWords), n_r = win_words(t.refs0, t.refs1, kRefWords);
  const uint32_t n_w = win_words(t.widths0, t.widths1, kWidthWords), n_h = tile == 0u ? head_words(rec) : 0u;
  for (uint32_t w = tid; w < n_d; w += kPackThreads) win_d[w] = 0u;
  if (tid < n_r) win_r[tid] = 0u;
  if (tid < n_w) win_w[tid] = 0u;
  if (tid < n_h) win_h[tid] = 0u;
  __syncthreads();
  const RowBits q = row_bits(a, r);
  const uint32_t L = r.L, rel_d = (uint32_t)(t.data0 & 31u), rel_r = (uint32_t)(t.refs0 & 31u), rel_w = (uint32_t)(t.widths0 & 31u);
  const uint2* __restrict__ groups = a.groups + r.group_off;
#pragma unroll
  for (int p = 0; p < kPerLane; ++p) {
    const uint32_t in_tile = (uint32_t)p * kPackThreads + tid, i = tile * kTile + in_tile;
    if (i >= r.n_values) continue;
    const uint32_t gl = in_tile / L, k = in_tile % L;
    const uint2 grp = groups[t.g0 + gl];
    const uint32_t ref = grp.x, w = grp.y & 255u, at = grp.y >> 8;
    if (w != 0u) win_put(win_d, n_d, rel_d + at + k * w, smm_cpx::z_of(q, i, dec) - ref, w);
    if (k == 0u) {
      if (rec.nbits > 0) win_put(win_r, n_r, rel_r + gl * (uint32_t)rec.nbits, ref, (uint32_t)rec.nbits);
      if (rec.width_bits > 0) win_put(win_w, n_w, rel_w + gl * (uint32_t)rec.width_bits, w - rec.width_ref, (uint32_t)rec.width_bits);
    }
  }
  if (n_h != 0u && tid == 0u) {   // h_1 .. h_order and g from the row's first bit on, a word of the row's own
    const uint32_t nb = 8u * (uint32_t)dec.n_oct;
    win_put(win_h, n_h, 0u, smm_cpx::sign_magnitude_of((int64_t)q(0), dec.n_oct), nb);
    if (dec.order > 1) win_put(win_h, n_h, nb, smm_cpx::sign_magnitude_of((int64_t)q(1), dec.n_oct), nb);
    win_put(win_h, n_h, (uint32_t)dec.order * nb, smm_cpx::sign_magnitude_of(dec.g, dec.n_oct), nb);
  }
  __syncthreads();
  win_flush(a, win_d, n_d, t.data0 >> 5, tid);
  win_flush(a, win_r, n_r, t.refs0 >> 5, tid);
  win_flush(a, win_w, n_w, t.widths0 >> 5, tid);
  if (tid < n_h && (rec.byte_off >> 2) + tid < a.out_words) atomicOr(&a.out[(rec.byte_off >> 2) + tid], __builtin_bswap32(win_h[tid]));
}

// launches `total` workgroups as grids of at most grid_limit(), the first workgroup's number handed to the kernel
template <class F>
int for_grid(int64_t total, F&& launch) {
  const int64_t limit = std::min<int64_t>(std::max<int64_t>(grid_limit(), 1), 0x7fffffffLL);
  for (int64_t b0 = 0; b0 < total; b0 += limit) {
    launch(b0, (unsigned)std::min(limit, total - b0));
    SMM_HIP(hipGetLastError());
  }
  return SMM_OK;
}

int launch_cpx_pack(const PackArgs& a, int64_t n_j, uint32_t max_tiles, bool any_order, hipStream_t s) {
  const int64_t tiles = n_j * (int64_t)max_tiles;
  const uint32_t edge_groups = (max_tiles + kPackThreads - 1) / kPackThreads;
  if (any_order)
    if (int rc = for_grid(tiles, [&](int64_t b0, unsigned nb) {
          hipLaunchKernelGGL(smm_grib_cpx_diff_kernel, dim3(nb), dim3(kPackThreads), 0, s, a, b0, max_tiles);
        }))
      return rc;
  // one launch: a grid of n_j / 256 workgroups stays below every limit a test sets and the device has
  hipLaunchKernelGGL(smm_grib_cpx_decide_kernel, dim3((unsigned)((n_j + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, s, a, n_j);
  SMM_HIP(hipGetLastError());
  if (int rc = for_grid(tiles, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(smm_grib_cpx_groups_kernel, dim3(nb), dim3(kPackThreads), 0, s, a, b0, max_tiles);
      }))
    return rc;
  if (int rc = for_grid(n_j, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(smm_grib_cpx_rows_kernel, dim3(nb), dim3(kWave), 0, s, a, b0);
      }))
    return rc;
  hipLaunchKernelGGL(smm_grib_cpx_layout_kernel, dim3(1), dim3(kWave), 0, s, a, n_j);
  SMM_HIP(hipGetLastError());
  if (int rc = for_grid(n_j * (int64_t)edge_groups, [&](int64_t b0, unsigned nb) {
        hipLaunchKernelGGL(smm_grib_cpx_edges_kernel, dim3(nb), dim3(kPackThreads), 0, s, a, b0, edge_groups);
      }))
    return rc;
  return for_grid(tiles, [&](int64_t b0, unsigned nb) {
    hipLaunchKernelGGL(smm_grib_cpx_emit_kernel, dim3(nb), dim3(kPackThreads), 0, s, a, b0, max_tiles);
  });
}

// What the entries with "wanted" records refuse about them; nothing but n_values, nbits, order, length_ref and reserved
// is read.
int check_pack_records(const smm_grib_cpx_t* recs, int64_t n_batch) {
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (!recs && n_batch > 0) return fail(SMM_ERR_INVALID, "null record pointer");
  for (int64_t b = 0; b < n_batch; ++b) {
    const smm_grib_cpx_t& c = recs[b];
    const std::string at = "recs[" + std::to_string(b) + "]";
    if (c.order < 0 || c.order > 2) return fail(SMM_ERR_INVALID, at + ".order (of spatial differencing) must be 0, 1 or 2");
    if (c.length_ref != 8 && c.length_ref != 16 && c.length_ref != 32 && c.length_ref != 64)
      return fail(SMM_ERR_INVALID, at + ".length_ref (the group length) must be 8, 16, 32 or 64");
    if (c.nbits < 0 || c.nbits > 32) return fail(SMM_ERR_INVALID, at + ".nbits must be within 0..32");
    if (c.n_values >= ((uint64_t)1 << 31)) return fail(SMM_ERR_INVALID, at + ".n_values must be below 2^31");
    if (c.reserved != 0) return fail(SMM_ERR_INVALID, at + ".reserved must be 0");
  }
  return SMM_OK;
}

uint64_t pack_bound(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (byte_off) byte_off[b] = at;
    at += smm_cpx::pack_bound_bytes(recs[b].n_values, recs[b].nbits, recs[b].order, recs[b].length_ref);
  }
  return at;
}

int smm_grib_cpx_pack_impl(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const smm_grib_cpx_t* recs,
                           int64_t n_batch, void* out, int64_t out_bytes, smm_grib_cpx_t* recs_out, uint64_t* used_bytes,
                           void* stream) {
  const size_t n = (size_t)n_batch;
  std::vector<PackRow> table(n);
  std::vector<RowStats> stats(n, RowStats{~0ull, 0ull, 0u, 64u, 0u, 0u});
  uint64_t groups = 0, tiles = 0;
  uint32_t max_tiles = 0;
  bool any_order = false;
  for (size_t b = 0; b < n; ++b) {
    const smm_grib_cpx_t& c = recs[b];
    PackRow& r = table[b];
    r = PackRow{rows_in[b].byte_off, groups, tiles, (uint32_t)c.n_values, 0u, 0u, c.length_ref, c.nbits, c.order};
    if (c.nbits == 0) continue;
    r.n_groups = smm_cpx::groups_of(r.n_values, r.L);
    r.n_tiles = (uint32_t)(((uint64_t)r.n_values + kTile - 1) / kTile);
    groups += r.n_groups;
    tiles += r.n_tiles;
    max_tiles = std::max(max_tiles, r.n_tiles);
    any_order = any_order || (c.order > 0 && r.n_values > (uint32_t)c.order);
  }
  *used_bytes = 0;
  if (n == 0) return SMM_OK;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the device");
  hipStream_t s = (hipStream_t)stream;
  auto align8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
  const size_t table_at = 0, stats_at = table_at + n * sizeof(PackRow), plans_at = stats_at + n * sizeof(RowStats),
               recs_at = plans_at + n * sizeof(smm_cpx::Decision), used_at = recs_at + n * sizeof(smm_cpx::Row),
               groups_at = used_at + 8, tile_at_at = groups_at + (size_t)groups * sizeof(uint2),
               tile_bits_at = tile_at_at + (size_t)tiles * sizeof(uint64_t), bytes = align8(tile_bits_at + (size_t)tiles * sizeof(uint32_t));
  static_assert(sizeof(smm_cpx::Row) % 8 == 0 && sizeof(smm_cpx::Decision) % 8 == 0 && sizeof(RowStats) % 8 == 0, "8-byte aligned tables");
  DeviceBuf<char> d;   // table, stats, plans, records, bytes used, group records, tile offsets, tile bits
  SMM_HIP(d.alloc(bytes));
  SMM_HIP(hipMemcpyAsync(d.get() + table_at, table.data(), n * sizeof(PackRow), hipMemcpyHostToDevice, s));
  SMM_HIP(hipMemcpyAsync(d.get() + stats_at, stats.data(), n * sizeof(RowStats), hipMemcpyHostToDevice, s));
  PackArgs a{};
  a.x = (const uint32_t*)x;
  a.last_word = x_bytes > 0 ? smm_grib::align4((uint64_t)x_bytes) / 4 - 1 : 0;
  a.rows = (const PackRow*)(d.get() + table_at);
  a.stats = (RowStats*)(d.get() + stats_at);
  a.plans = (smm_cpx::Decision*)(d.get() + plans_at);
  a.recs = (smm_cpx::Row*)(d.get() + recs_at);
  a.used = (uint64_t*)(d.get() + used_at);
  a.groups = (uint2*)(d.get() + groups_at);
  a.tile_at = (uint64_t*)(d.get() + tile_at_at);
  a.tile_bits = (uint32_t*)(d.get() + tile_bits_at);
  a.out = (uint32_t*)out;
  a.out_words = (uint64_t)out_bytes / 4;
  std::vector<smm_cpx::Row> got(n + 1);   // the records, then the bytes used in the place of one more
  static_assert(sizeof(smm_cpx::Row) >= 8, "the bytes used lie behind the records");
  int rc = launch_cpx_pack(a, n_batch, max_tiles, any_order, s);
  if (rc == SMM_OK) {
    const hipError_t e = hipMemcpyAsync(got.data(), a.recs, n * sizeof(smm_cpx::Row) + 8, hipMemcpyDeviceToHost, s);
    if (e != hipSuccess) rc = fail(SMM_ERR_HIP, std::string("copying the rows' records: ") + hipGetErrorString(e));
  }
  const hipError_t e = hipStreamSynchronize(s);   // the tables and the scratch are in use until here
  if (rc != SMM_OK) {
    (void)hipGetLastError();
    return rc;
  }
  SMM_HIP(e);
  for (size_t b = 0; b < n; ++b)
    recs_out[b] = recs[b].nbits == 0 ? smm_cpx::simple_record(recs[b].n_values, got[b].byte_off) : smm_cpx::record_of(got[b]);
  *used_bytes = got[n].byte_off;
  return SMM_OK;
}

}  // namespace

extern "C" {

int smm_grib_cpx_pack_bound(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes) {
  return guarded([&] {
    if (!total_bytes) return fail(SMM_ERR_INVALID, "null total pointer");
    if (int rc = check_pack_records(recs, n_batch)) return rc;
    *total_bytes = pack_bound(recs, n_batch, byte_off);
    return (int)SMM_OK;
  });
}

int smm_grib_cpx_pack(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const smm_grib_cpx_t* recs,
                      int64_t n_batch, void* out, int64_t out_bytes, smm_grib_cpx_t* recs_out, uint64_t* used_bytes,
                      void* stream) {
  return guarded([&] {
    if (int rc = check_pack_records(recs, n_batch)) return rc;
    if (n_batch > 0 && (!rows_in || !recs_out)) return fail(SMM_ERR_INVALID, "null row-table or result pointer");
    if (!used_bytes) return fail(SMM_ERR_INVALID, "null used_bytes pointer");
    if (x_bytes < 0) return fail(SMM_ERR_INVALID, "negative x_bytes");
    if (out_bytes < 0) return fail(SMM_ERR_INVALID, "negative out_bytes");
    bool streams = false;
    for (int64_t b = 0; b < n_batch; ++b) {
      const std::string at = "rows_in[" + std::to_string(b) + "]";
      if (rows_in[b].nbits != recs[b].nbits)
        return fail(SMM_ERR_INVALID, at + ".nbits differs from recs[" + std::to_string(b) + "].nbits");
      const uint64_t len = smm_grib::row_bytes(recs[b].n_values, recs[b].nbits);
      if (len > 0 && (rows_in[b].byte_off > (uint64_t)x_bytes || len > (uint64_t)x_bytes - rows_in[b].byte_off))
        return fail(SMM_ERR_INVALID, at + ": bytes [" + std::to_string(rows_in[b].byte_off) + ", " +
                                         std::to_string(rows_in[b].byte_off) + " + " + std::to_string(len) +
                                         ") leave the buffer of " + std::to_string(x_bytes) + " bytes");
      streams = streams || len > 0;
    }
    const uint64_t bound = pack_bound(recs, n_batch, nullptr);
    if ((uint64_t)out_bytes < bound)
      return fail(SMM_ERR_INVALID, "out_bytes " + std::to_string(out_bytes) + " is below the bound of " + std::to_string(bound) +
                                       " bytes");
    if (streams && (!x || !out)) return fail(SMM_ERR_INVALID, "null field or output pointer");
    if ((uintptr_t)x % 4) return fail(SMM_ERR_INVALID, "field pointer is not 4-byte aligned");
    if ((uintptr_t)out % 4) return fail(SMM_ERR_INVALID, "output pointer is not 4-byte aligned");
    return smm_grib_cpx_pack_impl(device, x, x_bytes, rows_in, recs, n_batch, out, out_bytes, recs_out, used_bytes, stream);
  });
}

int smm_grib_cpx_encode_host(const uint32_t* values, int64_t n_values, const smm_grib_cpx_t* rec, void* out, int64_t out_cap,
                             uint64_t* byte_len, smm_grib_cpx_t* rec_out) {
  return guarded([&] {
    if (!rec || !byte_len || !rec_out) return fail(SMM_ERR_INVALID, "null record, length or result pointer");
    if (int rc = check_pack_records(rec, 1)) return rc;
    if (n_values < 0 || (uint64_t)n_values != rec->n_values) return fail(SMM_ERR_INVALID, "n_values differs from rec.n_values");
    if (out_cap < 0) return fail(SMM_ERR_INVALID, "negative out_cap");
    *byte_len = 0;
    if (n_values > 0 && !values) return fail(SMM_ERR_INVALID, "null values pointer");
    const uint32_t xmax = smm_aec::sample_max(rec->nbits);
    for (int64_t i = 0; i < n_values; ++i)
      if (values[i] > xmax)
        return fail(SMM_ERR_INVALID, "values[" + std::to_string(i) + "] does not fit into " + std::to_string(rec->nbits) + " bits");
    if (rec->nbits == 0) {   // rule 6: not coded
      *rec_out = smm_cpx::simple_record(rec->n_values, 0);
      return (int)SMM_OK;
    }
    const uint64_t bound = smm_cpx::pack_bound_bytes(rec->n_values, rec->nbits, rec->order, rec->length_ref);
    if ((uint64_t)out_cap < bound)
      return fail(SMM_ERR_INVALID, "out_cap " + std::to_string(out_cap) + " is below the bound of " + std::to_string(bound) + " bytes");
    if (bound > 0 && !out) return fail(SMM_ERR_INVALID, "null output pointer");
    if (bound > 0) std::fill((uint8_t*)out, (uint8_t*)out + bound, (uint8_t)0);
    smm_cpx::Row row{};
    const smm_cpx::Want want{(uint32_t)rec->n_values, rec->nbits, rec->order, rec->length_ref};
    const uint64_t len = smm_cpx::encode_row([&](uint32_t i) { return values[i]; }, want, (uint8_t*)out, bound, &row);
    if (len == UINT64_MAX) return fail(SMM_ERR_INTERNAL, "the stream passed its bound");
    *byte_len = len;
    *rec_out = smm_cpx::record_of(row);
    return (int)SMM_OK;
  });
}

}  // extern "C"
