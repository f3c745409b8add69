// smm_grib_aec_unpack (gfx950): the CCSDS streams of GRIB-2 template 5.42 turned into simple-packed streams on the
// device, and the two host-only entries beside it (smm_grib_aec_layout, smm_grib_aec_decode_host).  The format and the
// decoder's two rules are the text of smm_grib_aec.hpp; the kernels read the stream through smm_grib_codec.hpp's
// load_word / bits_of and take the options apart with its zero_run_blocks / second_ext_pair / unmap.  What the kernels
// and the entries share with the other transcoders -- the cut launches, the scans, the store, the host shell and the
// entry checks -- is smm_grib_xcode.hpp.  Three kernels in stream order:
//   parse    one wave per row.  Block boundaries are only known by parsing, so a row is serial in blocks; a block is
//            done by all 64 lanes over a window of 128 stream words held in LDS
//   inverse  the preprocessor's inverse, one lane per reference sample interval, 64 intervals x 16 samples of the
//            scratch at a time through LDS (the global accesses are runs of 64 B, not one word per 16 KiB)
//   store    one thread per 32-bit word of a row's output stream, as smm_grib_pack's pack pass
// Plain vector stores, no atomics.
#include "smm_grib_xcode.hpp"

#include "smm_grib_aec.hpp"

namespace {

constexpr int kWinWords = 128;        // the parse kernel's window: 4096 bits
constexpr uint32_t kRefillAt = 60;    // words the cursor may be into the window at a block's start: the largest block
                                      // (5 + 1 + 32 + 64 * 32 bits) then ends 4037 bits in at most
constexpr int kTile = 16;             // samples of an interval per step of the inverse kernel
constexpr int kStoreThreads = 256;

struct AecRow {           // what a row of the call brings to the device; 56 B
  uint64_t byte_off, byte_len;   // the stream in x
  uint64_t scratch_off;          // the row's first sample in the scratch, in elements
  uint64_t out_off;              // the row's stream in out, in bytes: a multiple of 4
  uint32_t n_values;
  int32_t nbits, block, rsi;     // nbits == 0: the row has no stream, nothing is done
  uint32_t preprocess, pad;
};
struct AecArgs {
  const void* x;
  const AecRow* rows;
  uint32_t* scratch;
  uint32_t* out;
  int32_t* status;   // [n_j]
};

// ---- 1: parse.  Every value that steers the loop is the same in all lanes (the row's record, the cursor, words of the
// window every lane reads alike): the branches and barriers are wave-uniform.  A step consumes at least the ID's bits
// and J samples, so a row takes at most ceil(n_values / J) steps whatever its bytes hold.
__global__ __launch_bounds__(kWave) void smm_grib_aec_parse_kernel(AecArgs a, int64_t b0) {
  __shared__ uint32_t win[kWinWords];
  __shared__ uint32_t ones[kWave];
  const int64_t j = b0 + blockIdx.x;
  const uint32_t lane = threadIdx.x;
  const AecRow* __restrict__ rows = a.rows;
  const AecRow r = rows[j];
  if (r.nbits == 0 || r.n_values == 0) {
    if (lane == 0) a.status[j] = smm_aec::kOk;
    return;
  }
  if (r.byte_len == 0) {
    if (lane == 0) a.status[j] = smm_aec::kExhausted;
    return;
  }
  uint32_t* __restrict__ sc = a.scratch + r.scratch_off;
  const uint64_t end_byte = r.byte_off + r.byte_len, bit_end = 8 * end_byte, last_word = (end_byte - 1) >> 2;
  const uint32_t n = r.n_values, J = (uint32_t)r.block, rsi = (uint32_t)r.rsi, nbits = (uint32_t)r.nbits;
  const int idl = smm_aec::id_len(r.nbits);
  const uint32_t id_raw = (1u << idl) - 1u, block_bits = J * nbits;   // <= 2048
  uint64_t pos = 8 * r.byte_off, wbase = 0;
  bool have_win = false;
  uint32_t at = 0, b = 0;
  int status = smm_aec::kOk;

  // n (0..32) bits at stream bit p, from the window; the index is clamped to it
  auto wpeek = [&](uint64_t p, int nb) -> uint32_t {
    uint32_t i = (uint32_t)((p >> 5) - wbase);
    i = i < (uint32_t)(kWinWords - 1) ? i : (uint32_t)(kWinWords - 2);
    return smm_grib::bits_of(win[i], win[i + 1], (unsigned)(p & 31), nb);
  };

  while (at < n) {
    if (!have_win || (pos >> 5) - wbase >= kRefillAt) {
      __syncthreads();
      wbase = pos >> 5;
      win[lane] = smm_grib::load_word(a.x, wbase + lane, last_word, end_byte);
      win[lane + kWave] = smm_grib::load_word(a.x, wbase + kWave + lane, last_word, end_byte);
      have_win = true;
      __syncthreads();
    }
    const bool ref = r.preprocess != 0u && b == 0;
    const uint32_t nref = ref ? 1u : 0u;
    const uint32_t left = n - at;   // samples the row still takes: >= 1
    const uint32_t id = wpeek(pos, idl);
    uint64_t p = pos + (uint64_t)idl;
    uint32_t blocks = 1;
    if (id == id_raw) {
      if (lane < J && lane < left) sc[at + lane] = wpeek(p + (uint64_t)lane * nbits, (int)nbits);
      p += block_bits;
    } else {
      const bool low = id == 0;
      const uint32_t second = low ? wpeek(p, 1) : 0u;
      if (low) p += 1;
      const uint32_t refval = ref ? wpeek(p, (int)nbits) : 0u;
      if (ref) p += nbits;
      if (low && !second) {
        // a zero run: its FS value within 65 bits
        const uint32_t v0 = wpeek(p, 32), v1 = wpeek(p + 32, 32), v2 = wpeek(p + 64, 1);
        const uint32_t fs = v0 ? (uint32_t)__builtin_clz(v0) : v1 ? 32u + (uint32_t)__builtin_clz(v1) : v2 ? 64u : 65u;
        if (fs >= smm_aec::kMaxZeroFsBits) {
          status = p + smm_aec::kMaxZeroFsBits > bit_end ? smm_aec::kExhausted : smm_aec::kInvalid;
          break;
        }
        p += fs + 1;
        bool ros = false;
        blocks = smm_aec::zero_run_blocks(fs, b, rsi, &ros);
        if (blocks > rsi - b) {
          status = p > bit_end ? smm_aec::kExhausted : smm_aec::kInvalid;
          break;
        }
        const uint32_t want = blocks * J;   // <= 64 * 64
        const uint32_t fill = want < left ? want : left;
        for (uint32_t t = lane; t < fill; t += kWave) sc[at + t] = 0u;
      } else {
        // FS-coded samples: split-sample (k = ID - 1, J - nref codes) or second extension (J / 2 codes, no remainders)
        const uint32_t k = low ? 0u : id - 1u, nc = low ? J / 2 : J - nref;
        if (nc * k >= block_bits) {
          // no block has such a k -- but an ID or reference sample that the stream's end cuts is read from what lies behind
          status = p > bit_end ? smm_aec::kExhausted : smm_aec::kInvalid;
          break;
        }
        const uint32_t limit = block_bits - nc * k;   // rule 1: the FS codes end within this many bits
        // lane l looks at bits [w l, w l + w) of the FS part, w = ceil(limit / 64) <= 32: the bits the codes may take are
        // spread over the whole wave, so no lane holds many of the ones (with 64 bits a lane, the 32 codes of a smooth
        // block sat in lane 0, whose walk below the other lanes waited for); bits at or beyond the limit do not count
        const uint32_t w = (limit + 63u) / 64u, cb = w * lane;
        uint32_t chunk = 0;   // the lane's bits, left-aligned
        if (cb < limit) {
          const uint32_t take = limit - cb < w ? limit - cb : w;   // 1..32
          chunk = wpeek(p + cb, (int)take) << (32u - take);
        }
        const uint32_t cnt = (uint32_t)__builtin_popcount(chunk);
        const uint32_t incl = wave_scan(cnt);
        const uint32_t total = __shfl(incl, kWave - 1, kWave);
        const uint32_t have = total < nc ? total : nc;   // codes whose terminating one is there
        // the positions of the first nc ones, in order: lane l's start at rank incl - cnt
        uint32_t idx = incl - cnt;
        while (chunk != 0u && idx < nc) {
          const uint32_t z = (uint32_t)__builtin_clz(chunk);
          ones[idx++] = cb + z;
          chunk &= ~(0x80000000u >> z);
        }
        __syncthreads();
        uint32_t fs = 0;
        if (lane < have) fs = ones[lane] - (lane ? ones[lane - 1] + 1u : 0u);
        if (low) {
          // the first value above the largest decides, as in decode_row, which takes the codes in order: it is invalid
          // where its code ends inside the stream, whatever becomes of the codes behind it
          const unsigned long long over = __ballot(lane < have && fs > smm_aec::kMaxSecondExt);
          if (over != 0ull) {
            const uint32_t first = (uint32_t)__builtin_ctzll(over);
            status = p + ones[first] + 1u > bit_end ? smm_aec::kExhausted : smm_aec::kInvalid;
            break;
          }
        }
        if (total < nc) {   // the nc-th terminating one is not there
          status = p + limit > bit_end ? smm_aec::kExhausted : smm_aec::kInvalid;
          break;
        }
        const uint32_t fs_end = ones[nc - 1] + 1u;
        if (low) {
          if (lane < nc) {
            uint32_t pa, pb;
            smm_aec::second_ext_pair(fs, &pa, &pb);
            const uint32_t i0 = 2u * lane;
            if (i0 < left && !(ref && lane == 0)) sc[at + i0] = pa;
            if (i0 + 1 < left) sc[at + i0 + 1] = pb;
          }
        } else if (lane < nc) {
          const uint32_t rem = wpeek(p + fs_end + (uint64_t)lane * k, (int)k);
          if (nref + lane < left) sc[at + nref + lane] = (fs << k) + rem;
        }
        p += fs_end + nc * k;
        __syncthreads();   // `ones` is free for the next block
      }
      if (ref && lane == 0) sc[at] = refval;
    }
    if (p > bit_end) {
      status = smm_aec::kExhausted;
      break;
    }
    pos = p;
    const uint32_t adv = blocks * J;
    at = adv < left ? at + adv : n;
    b += blocks;
    if (b >= rsi) b = 0;
  }
  if (status != smm_aec::kOk)
    for (uint32_t t = at + lane; t < n; t += kWave) sc[t] = 0u;
  if (lane == 0) a.status[j] = status;
}

// ---- 2: inverse.  Workgroup (row, g) takes intervals [64 g, 64 g + 64) of the row, lane l the interval 64 g + l: its
// samples are a serial recurrence from its reference sample on.  A tile of 64 intervals x kTile samples is loaded with
// lanes running along the samples (16 consecutive words per interval), walked by the lanes along the intervals, and
// stored back the way it came.  A row without the preprocessor has nothing to invert.
__global__ __launch_bounds__(kWave) void smm_grib_aec_inverse_kernel(AecArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t tile[kWave][kTile + 1];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t g = at.part, lane = threadIdx.x;
  const AecRow* __restrict__ rows = a.rows;
  const AecRow r = rows[j];
  if (r.nbits == 0 || r.preprocess == 0u) return;
  const uint32_t n = r.n_values, span = (uint32_t)r.block * (uint32_t)r.rsi;   // samples of an interval: 8 .. 2^18
  const uint64_t first = (uint64_t)g * kWave * span;                           // the group's first sample
  if (first >= n) return;
  uint32_t* __restrict__ sc = a.scratch + r.scratch_off;
  const uint32_t xmax = smm_grib::sample_max(r.nbits);
  const uint64_t mine = first + (uint64_t)lane * span;   // the lane's interval starts here
  uint32_t xp = 0;
  for (uint32_t t0 = 0; t0 < span; t0 += kTile) {
#pragma unroll
    for (int q = 0; q < kTile; ++q) {
      const uint32_t e = (uint32_t)q * kWave + lane, rr = e / kTile, cc = e % kTile;
      const uint64_t s = first + (uint64_t)rr * span + t0 + cc;
      if (t0 + cc < span && s < n) tile[rr][cc] = sc[s];
    }
    __syncthreads();
    for (int c = 0; c < kTile; ++c) {
      const uint32_t t = t0 + (uint32_t)c;
      if (t < span && mine + t < n) {
        xp = t == 0 ? tile[lane][c] & xmax : smm_aec::unmap(xp, tile[lane][c], xmax);
        tile[lane][c] = xp;
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < kTile; ++q) {
      const uint32_t e = (uint32_t)q * kWave + lane, rr = e / kTile, cc = e % kTile;
      const uint64_t s = first + (uint64_t)rr * span + t0 + cc;
      if (t0 + cc < span && s < n) sc[s] = tile[rr][cc];
    }
    __syncthreads();
  }
}

// ---- 3: store.  One thread per 32-bit word of the row's stream (the grid covers the widest row; a narrower row's
// surplus threads leave): the samples that overlap the word, each cut to the row's width, put in place as
// smm_grib_codec.hpp's grib_word_part has it.  Words the samples do not reach are stored as zero.
__global__ __launch_bounds__(kStoreThreads) void smm_grib_aec_store_kernel(AecArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const AecRow* __restrict__ rows = a.rows;
  const AecRow r = rows[at.j];
  const uint32_t* __restrict__ sc = a.scratch + r.scratch_off;
  const uint32_t xmax = smm_grib::sample_max(r.nbits);
  store_row_word(a.out, r.out_off, at.part * kStoreThreads + threadIdx.x, r.nbits, r.n_values,
                 [&](uint64_t i) { return sc[i] & xmax; });
}

// the widest row of the call takes max_groups workgroups of the inverse kernel and max_words words of the store
int launch_aec(const AecArgs& a, int64_t n_j, uint32_t max_groups, uint32_t max_words, hipStream_t s) {
  const uint32_t blocks_per_row = (max_words + kStoreThreads - 1) / kStoreThreads;
  if (int rc = launch_flat(smm_grib_aec_parse_kernel, kWave, n_j, s, a)) return rc;
  if (int rc = launch_flat(smm_grib_aec_inverse_kernel, kWave, n_j * max_groups, s, a, max_groups)) return rc;
  return launch_flat(smm_grib_aec_store_kernel, kStoreThreads, n_j * blocks_per_row, s, a, blocks_per_row);
}

// everything the two entries with records refuse about them
int check_aec_records(const smm_grib_aec_t* recs, int64_t n_batch, int64_t x_bytes) {
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (x_bytes < 0) return fail(SMM_ERR_INVALID, "negative x_bytes");
  if (!recs && n_batch > 0) return fail(SMM_ERR_INVALID, "null record pointer");
  std::string err;
  if (!smm::check_grib_aec(recs, n_batch, x_bytes, err)) return fail(SMM_ERR_INVALID, err);
  return SMM_OK;
}

int smm_grib_aec_unpack_impl(int device, const void* x, const smm_grib_aec_t* recs, const smm_grib_row_t* rows_in,
                             int64_t n_batch, void* out, const uint64_t* offs, smm_grib_row_t* rows_out, void* stream) {
  const size_t n = (size_t)n_batch;
  std::vector<AecRow> table(n);
  uint64_t samples = 0;
  uint32_t max_words = 0, max_groups = 0;
  for (size_t b = 0; b < n; ++b) {
    const smm_grib_aec_t& c = recs[b];
    AecRow& r = table[b];
    r = AecRow{c.byte_off, c.byte_len, samples, offs[b], (uint32_t)c.n_values, c.nbits, c.block_size, c.rsi,
               (c.flags & SMM_GRIB_AEC_PREPROCESS) ? 1u : 0u, 0u};
    rows_out[b] = rows_in[b];
    if (c.nbits == 0) continue;
    rows_out[b].byte_off = offs[b];
    samples += c.n_values;
    max_words = std::max(max_words, (uint32_t)((offs[b + 1] - offs[b]) >> 2));
    if (r.preprocess) {
      const uint64_t span = (uint64_t)c.block_size * (uint64_t)c.rsi, per_group = span * kWave;
      max_groups = std::max(max_groups, (uint32_t)((c.n_values + per_group - 1) / per_group));
    }
  }
  if (samples == 0) return SMM_OK;
  Arena arena;
  const size_t table_at = arena.add<AecRow>(n), status_at = arena.add<int32_t>(n), scratch_at = arena.add<uint32_t>(samples);
  std::vector<int32_t> status(n, smm_aec::kOk);
  if (int rc = run_transcode(
          device, stream, arena.bytes(), {Span{table_at, table.data(), n * sizeof(AecRow)}},
          [&](char* d, hipStream_t s) {
            const AecArgs a{x, Arena::at<AecRow>(d, table_at), Arena::at<uint32_t>(d, scratch_at), (uint32_t*)out,
                            Arena::at<int32_t>(d, status_at)};
            return launch_aec(a, n_batch, max_groups, max_words, s);
          },
          Span{status_at, status.data(), n * sizeof(int32_t)}, "statuses"))
    return rc;
  for (size_t b = 0; b < n; ++b)
    if (status[b] != smm_aec::kOk)
      return fail(SMM_ERR_INVALID, "recs[" + std::to_string(b) + "]: the CCSDS stream " +
                                       (status[b] == smm_aec::kExhausted ? "ends before its values do" : "is invalid"));
  return SMM_OK;
}

}  // namespace

extern "C" {

int smm_grib_aec_layout(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes) {
  return offsets_entry(
      recs, n_batch, byte_off, total_bytes, [](const smm_grib_aec_t* r, int64_t n) { return check_aec_records(r, n, INT64_MAX); },
      smm::grib_aec_layout);
}

int smm_grib_aec_unpack(int device, const void* x, int64_t x_bytes, const smm_grib_aec_t* recs, const smm_grib_row_t* rows_in,
                        int64_t n_batch, void* out, int64_t out_bytes, smm_grib_row_t* rows_out, void* stream) {
  return guarded([&] {
    if (int rc = check_aec_records(recs, n_batch, x_bytes)) return rc;
    std::vector<uint64_t> offs;
    if (int rc = check_unpack_call(x, recs, rows_in, n_batch, out, out_bytes, rows_out, offs, smm::grib_aec_layout,
                                   [&](int64_t b) { return check_row_width(rows_in, recs, b); }))
      return rc;
    return smm_grib_aec_unpack_impl(device, x, recs, rows_in, n_batch, out, offs.data(), rows_out, stream);
  });
}

int smm_grib_aec_decode_host(const void* x_host, int64_t x_bytes, const smm_grib_aec_t* rec, uint32_t* values,
                             uint64_t* histogram, int* status) {
  return guarded([&] {
    if (!rec || !status) return fail(SMM_ERR_INVALID, "null record or status pointer");
    if (int rc = check_aec_records(rec, 1, x_bytes)) return rc;
    if (rec->n_values > 0 && !values) return fail(SMM_ERR_INVALID, "null values pointer");
    if (rec->nbits == 0) {
      for (uint64_t i = 0; i < rec->n_values; ++i) values[i] = 0;
      *status = smm_aec::kOk;
      return (int)SMM_OK;
    }
    if (!x_host && rec->byte_len > 0) return fail(SMM_ERR_INVALID, "null field pointer");
    const smm_aec::Row row{rec->byte_off, rec->byte_len, (uint32_t)rec->n_values, rec->nbits, rec->block_size, rec->rsi,
                           (rec->flags & SMM_GRIB_AEC_PREPROCESS) != 0};
    *status = smm_aec::decode_row(x_host, row, values, histogram);
    return (int)SMM_OK;
  });
}

}  // extern "C"
