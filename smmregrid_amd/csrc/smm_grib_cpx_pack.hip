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
// order.  Every bit position is 64-bit; no store goes to or past out_words, no load past the last word of x.  The row's
// input (RowBits), lower / raise, the scans, the LDS windows (win_put / win_flush / zero_ends), the cut launches, the
// host shell and the entry checks are smm_grib_xcode.hpp's, shared with the other transcoders.
#include "smm_grib_xcode.hpp"

#include "smm_grib_cpx.hpp"

namespace {

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
  smm_cpx::Row* recs;         // per row: the record of the stream (rows kernel; byte_off: layout kernel); one more
                              // behind them, whose byte_off takes the bytes used
  uint2* groups;          // per group: ref_g, w_g | bit offset in the tile << 8
  uint32_t* tile_bits;    // per tile: its data bits
  uint64_t* tile_at;      // per tile: its first data bit in the row's data part
  uint32_t* out;
  uint64_t out_words;     // no store goes to or past this word of out
};

// the row's integers, read from its simple-packed stream
__device__ __forceinline__ RowBits row_bits(const PackArgs& a, const PackRow& r) {
  return row_bits(a.x, a.last_word, r.in_off, r.nbits);
}
__device__ __forceinline__ uint32_t umin32(uint32_t a, uint32_t b) { return a < b ? a : b; }
__device__ __forceinline__ uint32_t umax32(uint32_t a, uint32_t b) { return a > b ? a : b; }

// ---- 1: diff.  Workgroup (row, tile); only rows whose wanted order can hold (order > 0, n > order) take part.
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_diff_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part, tid = threadIdx.x;
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
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part, tid = threadIdx.x;
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
  const uint32_t incl = block_scan<kPackThreads>(bits, lds, tid);
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
  const uint64_t bits = scan_parts<uint64_t>(
      r.n_tiles, [&](uint32_t t) { return (uint64_t)a.tile_bits[r.tile_off + t]; },
      [&](uint32_t t, uint64_t before) { a.tile_at[r.tile_off + t] = before; });
  if (lane == 0) {
    smm_cpx::Row rec{};
    rec.n_values = r.n_values;
    if (r.nbits != 0 && r.n_values != 0) {
      const RowStats st = a.stats[j];
      rec = smm_cpx::coded_row(r.n_values, r.L, a.plans[j], st.ref_max, st.w_min, st.w_max, bits);
    }
    a.recs[j] = rec;
  }
}

// ---- 5: layout.  One wave: rows back to back in row order, each at a 4-byte-aligned offset.
__global__ __launch_bounds__(kWave) void smm_grib_cpx_layout_kernel(PackArgs a, int64_t n_j) {
  const uint64_t used = scan_parts<uint64_t>(
      n_j, [&](int64_t b) { return smm_grib::align4(a.recs[b].byte_len); },
      [&](int64_t b, uint64_t before) { a.recs[b].byte_off = before; });
  if (threadIdx.x == 0) a.recs[n_j].byte_off = used;
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
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_edges_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part * kPackThreads + threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || tile >= r.n_tiles) return;
  const smm_cpx::Row rec = a.recs[j];
  const TileBits t = tile_bits_of(a, r, rec, tile);
  zero_ends(a.out, a.out_words, t.refs0, t.refs1);
  zero_ends(a.out, a.out_words, t.widths0, t.widths1);
  zero_ends(a.out, a.out_words, t.data0, t.data1);
  if (tile == 0u)
    for (uint32_t w = 0; w < head_words(rec); ++w)
      if ((rec.byte_off >> 2) + w < a.out_words) a.out[(rec.byte_off >> 2) + w] = 0u;
}

// ---- 7: emit.  A workgroup per tile, a window for each of its three shares and one for the descriptors.
// words of a window whose share is [first, end), cut to the window
__device__ __forceinline__ uint32_t win_words(uint64_t first, uint64_t end, uint32_t cap) {
  if (end <= first) return 0u;
  const uint64_t n = ((first & 31u) + (end - first) + 31u) / 32u;
  return n < cap ? (uint32_t)n : cap;
}
__global__ __launch_bounds__(kPackThreads) void smm_grib_cpx_emit_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t win_d[kDataWords], win_r[kRefWords], win_w[kWidthWords], win_h[kHeadWords];
  const RowPart where = row_part(b0, per_row);
  const int64_t j = where.j;
  const uint32_t tile = where.part, tid = threadIdx.x;
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
  win_flush<kPackThreads>(a.out, a.out_words, win_d, n_d, t.data0 >> 5, tid);
  win_flush<kPackThreads>(a.out, a.out_words, win_r, n_r, t.refs0 >> 5, tid);
  win_flush<kPackThreads>(a.out, a.out_words, win_w, n_w, t.widths0 >> 5, tid);
  if (tid < n_h && (rec.byte_off >> 2) + tid < a.out_words) atomicOr(&a.out[(rec.byte_off >> 2) + tid], __builtin_bswap32(win_h[tid]));
}

int launch_cpx_pack(const PackArgs& a, int64_t n_j, uint32_t max_tiles, bool any_order, hipStream_t s) {
  const int64_t tiles = n_j * (int64_t)max_tiles;
  const uint32_t edge_groups = (max_tiles + kPackThreads - 1) / kPackThreads;
  if (int rc = launch_flat(smm_grib_cpx_diff_kernel, kPackThreads, any_order ? tiles : 0, s, a, max_tiles)) return rc;
  // one launch: a grid of n_j / 256 workgroups stays below every limit a test sets and the device has
  hipLaunchKernelGGL(smm_grib_cpx_decide_kernel, dim3((unsigned)((n_j + kPackThreads - 1) / kPackThreads)), dim3(kPackThreads), 0, s, a, n_j);
  SMM_HIP(hipGetLastError());
  if (int rc = launch_flat(smm_grib_cpx_groups_kernel, kPackThreads, tiles, s, a, max_tiles)) return rc;
  if (int rc = launch_flat(smm_grib_cpx_rows_kernel, kWave, n_j, s, a)) return rc;
  hipLaunchKernelGGL(smm_grib_cpx_layout_kernel, dim3(1), dim3(kWave), 0, s, a, n_j);
  SMM_HIP(hipGetLastError());
  if (int rc = launch_flat(smm_grib_cpx_edges_kernel, kPackThreads, n_j * (int64_t)edge_groups, s, a, edge_groups)) return rc;
  return launch_flat(smm_grib_cpx_emit_kernel, kPackThreads, tiles, s, a, max_tiles);
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
  return sum_rows(recs, n_batch, byte_off, [](const smm_grib_cpx_t& c) {
    return smm_cpx::pack_bound_bytes(c.n_values, c.nbits, c.order, c.length_ref);
  });
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
  Arena arena;   // table, stats, plans, records and the bytes used, group records, tile offsets, tile bits
  const size_t table_at = arena.add<PackRow>(n), stats_at = arena.add<RowStats>(n), plans_at = arena.add<smm_cpx::Decision>(n),
               recs_at = arena.add<smm_cpx::Row>(n + 1), groups_at = arena.add<uint2>(groups), tile_at_at = arena.add<uint64_t>(tiles),
               tile_bits_at = arena.add<uint32_t>(tiles);
  std::vector<smm_cpx::Row> got(n + 1);   // the records, then the bytes used in the byte_off of one more
  if (int rc = run_transcode(
          device, stream, arena.bytes(),
          {Span{table_at, table.data(), n * sizeof(PackRow)}, Span{stats_at, stats.data(), n * sizeof(RowStats)}},
          [&](char* d, hipStream_t s) {
            PackArgs a{};
            a.x = (const uint32_t*)x;
            a.last_word = x_bytes > 0 ? smm_grib::align4((uint64_t)x_bytes) / 4 - 1 : 0;
            a.rows = Arena::at<PackRow>(d, table_at);
            a.stats = Arena::at<RowStats>(d, stats_at);
            a.plans = Arena::at<smm_cpx::Decision>(d, plans_at);
            a.recs = Arena::at<smm_cpx::Row>(d, recs_at);
            a.groups = Arena::at<uint2>(d, groups_at);
            a.tile_at = Arena::at<uint64_t>(d, tile_at_at);
            a.tile_bits = Arena::at<uint32_t>(d, tile_bits_at);
            a.out = (uint32_t*)out;
            a.out_words = (uint64_t)out_bytes / 4;
            return launch_cpx_pack(a, n_batch, max_tiles, any_order, s);
          },
          Span{recs_at, got.data(), (n + 1) * sizeof(smm_cpx::Row)}, "records"))
    return rc;
  for (size_t b = 0; b < n; ++b)
    recs_out[b] = recs[b].nbits == 0 ? smm_cpx::simple_record(recs[b].n_values, got[b].byte_off) : smm_cpx::record_of(got[b]);
  *used_bytes = got[n].byte_off;
  return SMM_OK;
}

}  // namespace

extern "C" {

int smm_grib_cpx_pack_bound(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes) {
  return offsets_entry(recs, n_batch, byte_off, total_bytes, check_pack_records, pack_bound);
}

int smm_grib_cpx_pack(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const smm_grib_cpx_t* recs,
                      int64_t n_batch, void* out, int64_t out_bytes, smm_grib_cpx_t* recs_out, uint64_t* used_bytes,
                      void* stream) {
  return guarded([&] {
    if (int rc = check_pack_records(recs, n_batch)) return rc;
    if (int rc = check_pack_call(x, x_bytes, rows_in, recs, n_batch, out, out_bytes, recs_out, used_bytes, pack_bound)) return rc;
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
    const uint32_t xmax = smm_grib::sample_max(rec->nbits);
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
