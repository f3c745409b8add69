// smm_grib_aec_pack (gfx950): simple-packed streams on the device coded as the CCSDS streams of GRIB-2 template 5.42 --
// the mirror of smm_grib_aec_unpack -- and the two host-only entries beside it (smm_grib_aec_pack_bound,
// smm_grib_aec_encode_host).  THE RULE OF THIS ENCODER is the text of smm_grib_aec.hpp; the kernels compute a sample's
// symbol with its symbol() / map(), pick a block's option with its choose_option() and code zero runs with its
// zero_run_fs(): what encode_row writes on the host they write byte for byte.  Unlike the decoder nothing here is serial
// in a row's blocks.  Six kernels in stream order:
//   cost    a lane per sample, J lanes a block: the symbol from q[i] and q[i - 1] (the simple-packed stream's bits),
//           every option's bits reduced over the J lanes by shuffles, 8 B per block: the option and its bits
//   scan    a wave per 64-block segment of an RSI, a lane per block: a ballot of the zero-block flags gives the runs
//           (start, length, ROS), a wave scan the blocks' bit offsets in the segment
//   rows    a wave per row scans its segments' bits: segment offsets, the row's byte length
//   layout  one wave scans the rows' lengths: each row's 4-byte-aligned place in out, the bytes used
//   edges   a thread per segment zeroes the two words its stream shares with its neighbours
//   emit    a workgroup per segment assembles its bits in LDS (a lane per sample again; the symbols are recomputed, two
//           extracts from lines the cost kernel just read, rather than kept in 4 B per sample of scratch that would be
//           written and read once each), stores the whole words big-endian and ORs the two shared ones onto the zeros
// Vector stores and vector atomics (LDS and global OR) only.  OR commutes: the bytes do not depend on the order.  The
// row's input (RowBits), the scans, the LDS window (win_put / win_flush / zero_ends), the cut launches, the host shell
// and the entry checks are smm_grib_xcode.hpp's, shared with the other transcoders.
#include "smm_grib_xcode.hpp"

#include "smm_grib_aec.hpp"

namespace {

constexpr int kPackThreads = 256;
constexpr uint32_t kSeg = smm_aec::kSegmentBlocks;
// the emit kernel's window: a segment of 64 blocks of 5 + 1 + 32 + 64 * 32 bits, begun anywhere in a word
constexpr uint32_t kWinWords = (31u + kSeg * (5u + 1u + 32u + 64u * 32u) + 31u) / 32u + 1u;
constexpr uint32_t kSkip = 127;   // the fs field of a zero block inside a run: it has no bits of its own

struct PackRow {          // what a row of the call brings to the device; 56 B
  uint64_t in_off;        // the row's simple-packed stream in x, bytes
  uint64_t blk_off;       // the row's first block record
  uint64_t seg_off;       // the row's first segment record
  uint32_t n_values, n_blocks, n_segs, segs_per_rsi;
  int32_t nbits, block, rsi;   // nbits == 0: the row has no stream, nothing is done
  uint32_t preprocess;
};
static_assert(sizeof(PackRow) == 56, "a plain table, 8-byte aligned");
struct PackArgs {
  const uint32_t* x;
  uint64_t last_word;     // index of the last word of x: no load goes past it
  const PackRow* rows;
  uint32_t* blocks;       // per block 2 words: option | bits << 8, then bit offset in the segment | fs << 20
  uint32_t* seg_bits;     // per segment: its bits
  uint64_t* seg_at;       // per segment: its first bit in the row's stream
  uint64_t* row_out;      // [2 n + 1]: byte_off, byte_len per row; the bytes used
  uint32_t* out;
  uint64_t out_words;     // no store goes to or past this word of out
};

// the row's samples, read from its simple-packed stream
__device__ __forceinline__ RowBits row_bits(const PackArgs& a, const PackRow& r) {
  return row_bits(a.x, a.last_word, r.in_off, r.nbits);
}
// where segment s of the row begins and how many blocks it has: block `first` of the row = block b0 of its RSI;
// `full` blocks to the segment's or the RSI's end, `cnt` of them inside the data
struct SegGeom {
  uint32_t first, b0, full, cnt;
};
__device__ __forceinline__ SegGeom seg_geom(const PackRow& r, uint32_t s) {
  const uint32_t rsi = (uint32_t)r.rsi, b0 = (s % r.segs_per_rsi) * kSeg, first = (s / r.segs_per_rsi) * rsi + b0;
  const uint32_t full = std::min(kSeg, rsi - b0);
  return SegGeom{first, b0, full, std::min(full, r.n_blocks - first)};
}
__device__ __forceinline__ uint32_t group_sum(uint32_t v, uint32_t J) {
  for (uint32_t o = J >> 1; o > 0; o >>= 1) v += __shfl_xor(v, (int)o, kWave);
  return v;
}

// ---- 1: cost.  Workgroup (row, c) takes samples [256 c, 256 c + 256) of the row's blocks; 256 and 64 are multiples of
// J, so a block lies in one wave and a group of J lanes is valid or surplus as a whole (surplus lanes redo block 0 and
// store nothing: the shuffles stay whole).
__global__ __launch_bounds__(kPackThreads) void smm_grib_aec_cost_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const uint32_t chunk = at.part;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[at.j];
  if (r.nbits == 0) return;
  const uint32_t J = (uint32_t)r.block, total = r.n_blocks * J;   // < 2^31 + 64
  if ((uint64_t)chunk * kPackThreads >= total) return;
  const uint32_t t = chunk * kPackThreads + threadIdx.x;
  const bool valid = t < total;
  const uint32_t i = valid ? t : threadIdx.x % J, p = i % J, blk = i / J;
  const bool pp = r.preprocess != 0u, ref = pp && blk % (uint32_t)r.rsi == 0u, coded = !(ref && p == 0u);
  const uint32_t xmax = smm_grib::sample_max(r.nbits);
  const uint32_t d = smm_aec::symbol(row_bits(a, r), i, r.n_values, J * (uint32_t)r.rsi, pp, xmax);
  const uint32_t dz = coded ? d : 0u;
  // the pairs of the second extension sit on the even lanes: (dz, the next lane's symbol)
  const uint32_t next = __shfl_down(dz, 1, kWave);
  const uint32_t m = (p & 1u) ? 0u : smm_aec::second_ext_value(dz, next);
  const uint32_t se_sum = group_sum((p & 1u) ? 0u : m == smm_aec::kNoSecondExt ? 1u << 20 : m + 1u, J);
  const uint32_t any = group_sum(dz != 0u ? 1u : 0u, J);
  smm_aec::Choice ch = smm_aec::choose_option(r.nbits, J, ref, (se_sum >> 20) ? smm_aec::kNoSecondExt : se_sum,
                                              [&](uint32_t k) { return group_sum(coded ? smm_aec::fs_len(d, k) : 0u, J); });
  if (any == 0u) ch = smm_aec::Choice{smm_aec::kEncZero, 0u};
  if (valid && p == 0u) {
    uint32_t* rec = a.blocks + 2 * (r.blk_off + blk);
    rec[0] = ch.option | (ch.bits << 8);
  }
}

// ---- 2: scan.  A wave per segment, four to a workgroup.  Lane l holds block l of the segment; Z has a bit per zero
// block.  A run starts where a zero block has no zero block before it in the segment, and runs as far as Z has ones.
__global__ __launch_bounds__(kPackThreads) void smm_grib_aec_scan_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const uint32_t lane = threadIdx.x % kWave;
  const uint32_t s = at.part * (kPackThreads / kWave) + threadIdx.x / kWave;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[at.j];
  if (r.nbits == 0 || s >= r.n_segs) return;   // the same in all lanes of a wave
  const SegGeom g = seg_geom(r, s);
  uint32_t* rec = a.blocks + 2 * (r.blk_off + g.first + lane);
  const uint32_t info = lane < g.cnt ? rec[0] : 1u;
  const bool z = lane < g.cnt && (info & 255u) == smm_aec::kEncZero;
  const unsigned long long Z = __ballot(z);
  uint32_t bits = z ? 0u : info >> 8, fs = z ? kSkip : 0u;
  if (lane >= g.cnt) bits = 0u;
  if (z && (lane == 0u || ((Z >> (lane - 1u)) & 1ull) == 0ull)) {
    const unsigned long long rest = ~(Z >> lane);   // zero only for lane 0 of 64 zero blocks
    const uint32_t c = rest ? (uint32_t)__builtin_ctzll(rest) : kSeg;
    fs = smm_aec::zero_run_fs(c, lane + c == g.full);
    const bool ref = r.preprocess != 0u && g.b0 + lane == 0u;
    bits = (uint32_t)smm_aec::id_len(r.nbits) + 1u + (ref ? (uint32_t)r.nbits : 0u) + fs + 1u;
  }
  const uint32_t incl = wave_scan(bits);
  if (lane < g.cnt) rec[1] = (incl - bits) | (fs << 20);   // < 64 * 2086 < 2^20
  if (lane == kWave - 1) a.seg_bits[r.seg_off + s] = incl;
}

// ---- 3: rows.  A wave per row: the exclusive scan of its segments' bits, 64 at a step, and the row's bytes.
__global__ __launch_bounds__(kWave) void smm_grib_aec_rows_kernel(PackArgs a, int64_t b0) {
  const int64_t j = b0 + blockIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  const uint64_t bits = scan_parts<uint64_t>(
      r.n_segs, [&](uint32_t s) { return (uint64_t)a.seg_bits[r.seg_off + s]; },
      [&](uint32_t s, uint64_t before) { a.seg_at[r.seg_off + s] = before; });
  if (threadIdx.x == 0) a.row_out[2 * j + 1] = (bits + 7) / 8;
}

// ---- 4: layout.  One wave: rows back to back in row order, each at a 4-byte-aligned offset.
__global__ __launch_bounds__(kWave) void smm_grib_aec_layout_kernel(PackArgs a, int64_t n_j) {
  const uint64_t used = scan_parts<uint64_t>(
      n_j, [&](int64_t b) { return smm_grib::align4(a.row_out[2 * b + 1]); },
      [&](int64_t b, uint64_t before) { a.row_out[2 * b] = before; });
  if (threadIdx.x == 0) a.row_out[2 * n_j] = used;
}

// the segment's first bit in out, counted from out's first bit
__device__ __forceinline__ uint64_t seg_first_bit(const PackArgs& a, const PackRow& r, int64_t j, uint32_t s) {
  return 8 * a.row_out[2 * j] + a.seg_at[r.seg_off + s];
}

// ---- 5: edges.  The first and the last word of a segment's stream may hold bits of its neighbours in the row (a row
// begins and ends on a word of its own): they are zeroed here and ORed into by the emit kernel.  A segment has at least
// the bits of one ID.
__global__ __launch_bounds__(kPackThreads) void smm_grib_aec_edges_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const uint32_t s = at.part * kPackThreads + threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[at.j];
  if (r.nbits == 0 || s >= r.n_segs) return;
  const uint64_t first = seg_first_bit(a, r, at.j, s);
  zero_ends(a.out, a.out_words, first, first + a.seg_bits[r.seg_off + s]);
}

// ---- 6: emit.  A workgroup per segment, its bits in one window.
__global__ __launch_bounds__(kPackThreads) void smm_grib_aec_emit_kernel(PackArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t win[kWinWords];
  const RowPart where = row_part(b0, per_row);
  const int64_t j = where.j;
  const uint32_t s = where.part, tid = threadIdx.x;
  const PackRow* __restrict__ rows = a.rows;
  const PackRow r = rows[j];
  if (r.nbits == 0 || s >= r.n_segs) return;
  const SegGeom g = seg_geom(r, s);
  const uint64_t first_bit = seg_first_bit(a, r, j, s), w0 = first_bit >> 5;
  const uint32_t rel0 = (uint32_t)(first_bit & 31), seg_bits = a.seg_bits[r.seg_off + s];
  const uint32_t n_words = std::min((rel0 + seg_bits + 31u) / 32u, kWinWords);
  for (uint32_t w = tid; w < n_words; w += kPackThreads) win[w] = 0u;
  __syncthreads();
  const uint32_t J = (uint32_t)r.block, nbits = (uint32_t)r.nbits, idl = (uint32_t)smm_aec::id_len(r.nbits);
  const uint32_t xmax = smm_grib::sample_max(r.nbits), total = g.cnt * J;   // <= 4096
  const bool pp = r.preprocess != 0u;
  const RowBits q = row_bits(a, r);
  for (uint32_t base = 0; base < total; base += kPackThreads) {
    const bool valid = base + tid < total;                   // whole groups of J lanes, as in the cost kernel
    const uint32_t t = valid ? base + tid : tid % J, lb = t / J, p = t % J, blk = g.first + lb;
    const bool ref = pp && g.b0 + lb == 0u, coded = !(ref && p == 0u);
    const uint32_t nref = ref ? 1u : 0u;
    const uint32_t* rec = a.blocks + 2 * (r.blk_off + blk);
    const uint32_t option = rec[0] & 255u, place = rec[1], fs_run = place >> 20;
    const uint32_t at = rel0 + (place & 0xfffffu);
    const uint32_t d = smm_aec::symbol(q, blk * J + p, r.n_values, J * (uint32_t)r.rsi, pp, xmax);
    const bool split = option >= smm_aec::kEncSplit0 && option != smm_aec::kEncRaw, second = option == smm_aec::kEncSecondExt;
    const uint32_t k = split ? option - smm_aec::kEncSplit0 : 0u;
    // the FS code a lane writes: its symbol's (split), its pair's on the even lanes (second extension), none otherwise;
    // where it ends follows from the scan over the block's J lanes, taken by all lanes alike
    const uint32_t next = __shfl_down(d, 1, kWave);
    uint32_t len = 0;
    if (split && coded) len = (d >> k) + 1u;
    if (second && (p & 1u) == 0u) len = smm_aec::second_ext_value(coded ? d : 0u, next) + 1u;
    const uint32_t incl = group_scan(len, J);   // p == the lane's place among its J
    const uint32_t fs_total = __shfl(incl, (int)(J - 1u), (int)J);
    if (!valid) continue;
    const bool low = option == smm_aec::kEncZero || second;   // ID 0 and a selector bit
    const uint32_t hdr = at + idl + (low ? 1u : 0u) + nref * nbits;   // the first bit behind ID, selector and reference
    if (option == smm_aec::kEncRaw) {
      if (p == 0u) win_put(win, n_words, at, (1u << idl) - 1u, idl);
      win_put(win, n_words, at + idl + p * nbits, d, nbits);
      continue;
    }
    if (p == 0u && fs_run != kSkip) {
      if (split) win_put(win, n_words, at, k + 1u, idl);
      if (second) win_put(win, n_words, at + idl, 1u, 1u);
      if (ref) win_put(win, n_words, hdr - nbits, d, nbits);
      if (option == smm_aec::kEncZero) win_put(win, n_words, hdr + fs_run, 1u, 1u);
    }
    if (len != 0u) win_put(win, n_words, hdr + incl - 1u, 1u, 1u);
    if (split && coded && k != 0u) win_put(win, n_words, hdr + fs_total + (p - nref) * k, d & ((1u << k) - 1u), k);
  }
  __syncthreads();
  win_flush<kPackThreads>(a.out, a.out_words, win, n_words, w0, tid);
}

// the widest row of the call has max_samples samples in whole blocks and max_segs segments
int launch_aec_pack(const PackArgs& a, int64_t n_j, uint32_t max_samples, uint32_t max_segs, hipStream_t s) {
  const uint32_t chunks = (uint32_t)(((uint64_t)max_samples + kPackThreads - 1) / kPackThreads);
  const uint32_t scan_groups = (max_segs + kPackThreads / kWave - 1) / (kPackThreads / kWave);
  const uint32_t edge_groups = (max_segs + kPackThreads - 1) / kPackThreads;
  if (int rc = launch_flat(smm_grib_aec_cost_kernel, kPackThreads, n_j * chunks, s, a, chunks)) return rc;
  if (int rc = launch_flat(smm_grib_aec_scan_kernel, kPackThreads, n_j * scan_groups, s, a, scan_groups)) return rc;
  if (int rc = launch_flat(smm_grib_aec_rows_kernel, kWave, n_j, s, a)) return rc;
  hipLaunchKernelGGL(smm_grib_aec_layout_kernel, dim3(1), dim3(kWave), 0, s, a, n_j);
  SMM_HIP(hipGetLastError());
  if (int rc = launch_flat(smm_grib_aec_edges_kernel, kPackThreads, n_j * edge_groups, s, a, edge_groups)) return rc;
  return launch_flat(smm_grib_aec_emit_kernel, kPackThreads, n_j * max_segs, s, a, max_segs);
}

// What the entries with "wanted" records refuse about them: everything smm_grib_aec_unpack refuses, the place of the
// stream apart (byte_off and byte_len are results here).
int check_pack_records(const smm_grib_aec_t* recs, int64_t n_batch) {
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (!recs && n_batch > 0) return fail(SMM_ERR_INVALID, "null record pointer");
  std::string err;
  for (int64_t b = 0; b < n_batch; ++b) {
    smm_grib_aec_t one = recs[b];
    one.byte_off = one.byte_len = 0;
    if (!smm::check_grib_aec(&one, 1, 0, err)) {
      const size_t at = err.find(']');
      return fail(SMM_ERR_INVALID, "recs[" + std::to_string(b) + (at == std::string::npos ? "]: " + err : err.substr(at)));
    }
  }
  return SMM_OK;
}

uint64_t pack_bound(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off) {
  return sum_rows(recs, n_batch, byte_off,
                  [](const smm_grib_aec_t& c) { return smm_aec::pack_bound_bytes(c.n_values, c.nbits, c.block_size); });
}

int smm_grib_aec_pack_impl(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const smm_grib_aec_t* recs,
                           int64_t n_batch, void* out, int64_t out_bytes, smm_grib_aec_t* recs_out, uint64_t* used_bytes,
                           void* stream) {
  const size_t n = (size_t)n_batch;
  std::vector<PackRow> table(n);
  uint64_t blocks = 0, segs = 0;
  uint32_t max_samples = 0, max_segs = 0;
  for (size_t b = 0; b < n; ++b) {
    const smm_grib_aec_t& c = recs[b];
    PackRow& r = table[b];
    r = PackRow{rows_in[b].byte_off, blocks, segs, (uint32_t)c.n_values, 0u, 0u, 1u, c.nbits, c.block_size, c.rsi,
                (c.flags & SMM_GRIB_AEC_PREPROCESS) ? 1u : 0u};
    recs_out[b] = c;
    recs_out[b].byte_off = recs_out[b].byte_len = 0;
    if (c.nbits == 0) {
      r.block = r.rsi = 0;
      recs_out[b].block_size = 0;   // the mark of a row without a coded stream
      continue;
    }
    const uint32_t J = (uint32_t)c.block_size, rsi = (uint32_t)c.rsi;
    r.n_blocks = smm_aec::row_blocks(r.n_values, J);
    r.segs_per_rsi = (rsi + kSeg - 1) / kSeg;
    const uint32_t whole = r.n_blocks / rsi, rest = r.n_blocks % rsi;
    r.n_segs = whole * r.segs_per_rsi + (rest + kSeg - 1) / kSeg;
    blocks += r.n_blocks;
    segs += r.n_segs;
    max_samples = std::max(max_samples, r.n_blocks * J);
    max_segs = std::max(max_segs, r.n_segs);
  }
  *used_bytes = 0;
  if (n == 0) return SMM_OK;
  Arena arena;   // table, row results, segment offsets, block records, segment bits
  const size_t table_at = arena.add<PackRow>(n), rowout_at = arena.add<uint64_t>(2 * n + 1), segat_at = arena.add<uint64_t>(segs),
               blocks_at = arena.add<uint32_t>(2 * blocks), segbits_at = arena.add<uint32_t>(segs);
  std::vector<uint64_t> row_out(2 * n + 1, 0);
  if (int rc = run_transcode(
          device, stream, arena.bytes(), {Span{table_at, table.data(), n * sizeof(PackRow)}},
          [&](char* d, hipStream_t s) {
            PackArgs a{};
            a.x = (const uint32_t*)x;
            a.last_word = x_bytes > 0 ? smm_grib::align4((uint64_t)x_bytes) / 4 - 1 : 0;
            a.rows = Arena::at<PackRow>(d, table_at);
            a.row_out = Arena::at<uint64_t>(d, rowout_at);
            a.seg_at = Arena::at<uint64_t>(d, segat_at);
            a.blocks = Arena::at<uint32_t>(d, blocks_at);
            a.seg_bits = Arena::at<uint32_t>(d, segbits_at);
            a.out = (uint32_t*)out;
            a.out_words = (uint64_t)out_bytes / 4;
            return launch_aec_pack(a, n_batch, max_samples, max_segs, s);
          },
          Span{rowout_at, row_out.data(), (2 * n + 1) * sizeof(uint64_t)}, "places"))
    return rc;
  for (size_t b = 0; b < n; ++b) {
    recs_out[b].byte_off = row_out[2 * b];
    recs_out[b].byte_len = row_out[2 * b + 1];
  }
  *used_bytes = row_out[2 * n];
  return SMM_OK;
}

}  // namespace

extern "C" {

int smm_grib_aec_pack_bound(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes) {
  return offsets_entry(recs, n_batch, byte_off, total_bytes, check_pack_records, pack_bound);
}

int smm_grib_aec_pack(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in, const smm_grib_aec_t* recs,
                      int64_t n_batch, void* out, int64_t out_bytes, smm_grib_aec_t* recs_out, uint64_t* used_bytes,
                      void* stream) {
  return guarded([&] {
    if (int rc = check_pack_records(recs, n_batch)) return rc;
    if (int rc = check_pack_call(x, x_bytes, rows_in, recs, n_batch, out, out_bytes, recs_out, used_bytes, pack_bound)) return rc;
    return smm_grib_aec_pack_impl(device, x, x_bytes, rows_in, recs, n_batch, out, out_bytes, recs_out, used_bytes, stream);
  });
}

int smm_grib_aec_encode_host(const uint32_t* values, int64_t n_values, const smm_grib_aec_t* rec, void* out, int64_t out_cap,
                             uint64_t* byte_len, uint64_t* histogram) {
  return guarded([&] {
    if (!rec || !byte_len) return fail(SMM_ERR_INVALID, "null record or length pointer");
    if (int rc = check_pack_records(rec, 1)) return rc;
    if (n_values < 0 || (uint64_t)n_values != rec->n_values) return fail(SMM_ERR_INVALID, "n_values differs from rec.n_values");
    if (out_cap < 0) return fail(SMM_ERR_INVALID, "negative out_cap");
    *byte_len = 0;
    if (rec->nbits == 0 || n_values == 0) return (int)SMM_OK;
    if (!values) return fail(SMM_ERR_INVALID, "null values pointer");
    const uint64_t bound = smm_aec::pack_bound_bytes(rec->n_values, rec->nbits, rec->block_size);
    if ((uint64_t)out_cap < bound)
      return fail(SMM_ERR_INVALID, "out_cap " + std::to_string(out_cap) + " is below the bound of " + std::to_string(bound) + " bytes");
    if (!out) return fail(SMM_ERR_INVALID, "null output pointer");
    const uint32_t xmax = smm_grib::sample_max(rec->nbits);
    for (int64_t i = 0; i < n_values; ++i)
      if (values[i] > xmax) return fail(SMM_ERR_INVALID, "values[" + std::to_string(i) + "] does not fit into " + std::to_string(rec->nbits) + " bits");
    std::fill((uint8_t*)out, (uint8_t*)out + bound, (uint8_t)0);
    const smm_aec::Row row{0, 0, (uint32_t)rec->n_values, rec->nbits, rec->block_size, rec->rsi, (rec->flags & SMM_GRIB_AEC_PREPROCESS) != 0};
    const uint64_t len = smm_aec::encode_row([&](uint32_t i) { return values[i]; }, row, (uint8_t*)out, bound, histogram);
    if (len == UINT64_MAX) return fail(SMM_ERR_INTERNAL, "the stream passed its bound");
    *byte_len = len;
    return (int)SMM_OK;
  });
}

}  // extern "C"
