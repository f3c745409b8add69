// CCSDS 121.0-B adaptive entropy coding as GRIB-2 data representation template 5.42 carries it (what libaec writes
// for ecCodes): the decoder and the encoder, each stated once.  Plain C++ that compiles for host and device -- the host
// decode (smm_grib_aec_decode_host), the kernels of smm_grib_aec_unpack (smm_grib_aec.hip) and
// tests/cpp/grib_aec_harness.cpp all read the stream through smm_grib_codec.hpp's load_word / bits_of and take the
// options apart with the small functions below; the host encode (smm_grib_aec_encode_host), the kernels of smm_grib_aec_pack
// (smm_grib_aec_pack.hip) and tests/cpp/grib_aec_encode_harness.cpp put them together with the ones behind decode_row.
//
// THE FORMAT, for unsigned samples of nbits (1..32) bits, blocks of J (8 / 16 / 32 / 64) samples, a reference sample
// interval of rsi (1..4096) blocks, no restricted code set, no RSI padding:
//   block      an ID of id_len(nbits) = 3 / 4 / 5 bits (nbits <= 8 / <= 16 / else), then by ID
//     0          one more bit: 0 = zero-block run, 1 = second extension
//     all ones   J raw samples of nbits bits
//     other      split-sample, k = ID - 1: the fundamental sequences (FS: zeros, then a one) of all coded samples
//                first, then their k-bit remainders; sample = (fs << k) + remainder
//   reference  with the preprocessor on the first block of every RSI carries an nbits reference sample and codes
//              J - 1 samples: the reference follows the ID (split), the ID and the selector bit (ID 0), or is the first
//              raw sample (uncompressed)
//   zero run   an FS value fs, n = fs + 1 blocks of zeros; n == 5 ("ROS") runs to the end of the 64-block segment
//              or of the RSI, whichever comes first; n > 5 means n - 1 blocks
//   2nd ext.   J / 2 FS values m <= 90, each a pair (a, b) with m = (a + b)(a + b + 1) / 2 + b; in a reference block
//              the a of the first pair is dropped
//   the encoder pads the last block to J samples: what lies beyond n_values is parsed and thrown away
//   postproc.  with the preprocessor on the coded samples are mapped prediction errors d of a unit-delay predictor,
//              inverted by unmap() below from the RSI's reference sample on: serial within an RSI, independent across
// TWO RULES OF THIS DECODER bound every loop and every read.  (1) The FS codes of one block take at most J * nbits
// bits less its remainders (an encoder picks the shortest option, and the uncompressed one costs J * nbits), those
// of a zero run at most 65: a longer code ends the row as invalid.  (2) No load goes past the 32-bit word that
// holds the stream's last byte; a read that needs a bit beyond the stream ends the row as exhausted.
//
// THE RULE OF THIS ENCODER (encode_row below; smm_grib_aec_encode_host runs it, the kernels of smm_grib_aec_pack in
// smm_grib_aec_pack.hip compute the same bits from the same small functions), for the same streams the decoder takes:
// unsigned samples of 1..32 bits, J in {8, 16, 32, 64}, rsi in 1..4096, preprocessor on or off; no signed samples, no
// restricted code set, no RSI padding.  Nothing in it is left to a search order or a heuristic:
//   symbols    preprocessor off: the samples.  On: sample i of an RSI is coded as d = map(x[i - 1], x[i]), the exact
//              inverse of unmap(); the RSI's first sample is its reference sample and is carried raw
//   padding    the last block is padded to J samples with samples whose symbol is 0: the last sample repeated with the
//              preprocessor on, zeros with it off
//   option     a block whose coded symbols are all 0 is a zero block (never dearer: a run of c blocks costs at most
//              ID + 1 + reference + c + 1 bits).  Every other block takes the option with the fewest bits, the ID, the
//              selector bit and the reference sample counted: second extension, split-sample k for EVERY k the ID width
//              allows (0 .. 2^id_len - 3; exhaustive, not a neighbour search), uncompressed.  Ties go to the first in the
//              order second extension, split in ascending k, uncompressed
//   2nd ext.   is a candidate only when every pair value is <= 90 (kMaxSecondExt)
//   rule 1     a split option is therefore chosen only when it is STRICTLY shorter than the uncompressed one:
//              ID + reference + FS codes + nc * k < ID + J * nbits, so the FS codes take fewer than J * nbits - nc * k
//              bits -- the decoder's rule 1 holds for every stream of this encoder (a second extension at most ties:
//              its FS codes take at most J * nbits - 1 bits)
//   zero runs  consecutive zero blocks join into a run that never crosses a 64-block segment of the RSI nor the RSI's
//              end.  A run of c blocks is coded fs = c - 1 for c <= 4 and fs = c for c >= 5, but a run of c >= 5 that
//              reaches the end of its segment or of its RSI is coded ROS (fs = 4).  The end of the data is no such end.
//              An all-zero reference block starts a run like any other and carries the reference sample
//   the end    the stream is padded with zero bits to a whole byte
// These are not libaec's bits (its k search and its padding are its own); it is a valid CCSDS 121.0-B stream that
// decode_row and libaec decode.  No block is coded longer than uncompressed, which bounds a row: pack_bound_bytes.
#pragma once

#include <cstdint>

#include "smm_grib_codec.hpp"

namespace smm_aec {

enum : int { kOk = SMM_GRIB_AEC_OK, kExhausted = SMM_GRIB_AEC_EXHAUSTED, kInvalid = SMM_GRIB_AEC_INVALID };
// the bins of the option histogram (SMM_GRIB_AEC_OPTIONS of them)
enum : int { kOptZero = 0, kOptZeroRos, kOptSecondExt, kOptSplit0, kOptSplitK, kOptUncompressed, kOptReference, kNumOptions };
static_assert(kNumOptions == SMM_GRIB_AEC_OPTIONS, "one bin per coding option");

constexpr uint32_t kRos = 5, kSegmentBlocks = 64, kMaxSecondExt = 90, kMaxZeroFsBits = 65;

SMM_GRIB_HD int id_len(int nbits) { return nbits > 16 ? 5 : nbits > 8 ? 4 : 3; }
// blocks of a zero run from its FS value, at block b of the RSI (b < rsi)
SMM_GRIB_HD uint32_t zero_run_blocks(uint32_t fs, uint32_t b, uint32_t rsi, bool* ros) {
  const uint32_t n = fs + 1;
  *ros = n == kRos;
  if (n == kRos) {
    const uint32_t to_rsi = rsi - b, to_seg = kSegmentBlocks - (b % kSegmentBlocks);
    return to_rsi < to_seg ? to_rsi : to_seg;
  }
  return n > kRos ? n - 1 : n;
}
// the pair of a second-extension value m <= kMaxSecondExt
SMM_GRIB_HD void second_ext_pair(uint32_t m, uint32_t* a, uint32_t* b) {
  uint32_t s = 0;
  while (s < 12 && (s + 1) * (s + 2) / 2 <= m) ++s;
  *b = m - s * (s + 1) / 2;
  *a = s - *b;
}
// the sample after x_prev from its mapped prediction error d: theta = min(x_prev, xmax - x_prev); d <= 2 * theta is
// the signed error folded (even: +d/2, odd: -(d+1)/2), a larger d is the distance from the nearer bound
SMM_GRIB_HD uint32_t unmap(uint32_t x_prev, uint32_t d, uint32_t xmax) {
  const bool low = x_prev < xmax - x_prev;
  const uint32_t theta = low ? x_prev : xmax - x_prev;
  const uint32_t half = (d >> 1) + (d & 1u);
  uint32_t x;
  if (half <= theta)
    x = (d & 1u) ? x_prev - half : x_prev + half;
  else
    x = low ? d : xmax - d;
  return x & xmax;
}

// ---- the scalar decode: one row, block after block
struct Row {
  uint64_t byte_off, byte_len;   // the stream in x
  uint32_t n_values;
  int nbits, block, rsi;
  bool preprocess;
};

struct Reader {
  const void* x;
  uint64_t pos, bit_end;       // absolute bit positions in x
  uint64_t last_word, end_byte;
  int status;

  SMM_GRIB_HD uint32_t peek(uint64_t p, int n) const {
    const uint64_t w = p >> 5;
    return smm_grib::bits_of(smm_grib::load_word(x, w, last_word, end_byte), smm_grib::load_word(x, w + 1, last_word, end_byte),
                             (unsigned)(p & 31), n);
  }
  // n (0..32) bits; 0 once the row has ended
  SMM_GRIB_HD uint32_t get(int n) {
    if (status != kOk) return 0;
    if (pos + (uint64_t)n > bit_end) return status = kExhausted, 0u;
    const uint32_t v = peek(pos, n);
    pos += (uint64_t)n;
    return v;
  }
  // an FS value whose code (value + 1 bits) fits into `limit` bits
  SMM_GRIB_HD uint32_t get_fs(uint32_t limit) {
    uint32_t v = 0;
    while (status == kOk) {
      if (v >= limit) return status = kInvalid, 0u;
      if (pos >= bit_end) return status = kExhausted, 0u;
      const uint64_t left = bit_end - pos;
      const uint32_t avail = left < 32 ? (uint32_t)left : 32u;
      const uint32_t chunk = peek(pos, 32);
      const uint32_t z = chunk ? (uint32_t)__builtin_clz(chunk) : 32u;
      if (z >= avail) {   // no one among the bits the stream still has here
        v += avail;
        pos += avail;
        continue;
      }
      v += z;
      pos += z + 1;
      if (v >= limit) return status = kInvalid, 0u;
      return v;
    }
    return 0;
  }
};

SMM_GRIB_HD Reader make_reader(const void* x, const Row& r) {
  Reader rd;
  rd.x = x;
  rd.pos = 8 * r.byte_off;
  rd.bit_end = 8 * (r.byte_off + r.byte_len);
  rd.end_byte = r.byte_off + r.byte_len;
  rd.last_word = r.byte_len ? (r.byte_off + r.byte_len - 1) >> 2 : r.byte_off >> 2;
  rd.status = r.byte_len ? kOk : kExhausted;
  return rd;
}

// Decodes row r of x into out[0, n_values); hist: kNumOptions counters that are added to, or null.  Returns the row's
// status; the samples from the block that ended the row on are zero.  Every step of the loop consumes at least the ID's
// bits and J samples, whatever the stream holds.
SMM_GRIB_HD int decode_row(const void* x, const Row& r, uint32_t* out, uint64_t* hist) {
  const uint32_t n = r.n_values, J = (uint32_t)r.block, rsi = (uint32_t)r.rsi;
  const int idl = id_len(r.nbits);
  const uint32_t id_raw = (1u << idl) - 1u, xmax = smm_grib::sample_max(r.nbits), block_bits = J * (uint32_t)r.nbits;
  Reader rd = make_reader(x, r);
  if (n == 0) return kOk;
  uint32_t at = 0, b = 0;
  auto put = [&](uint32_t j, uint32_t v) {
    if (j < n - at) out[at + j] = v;
  };
  while (at < n && rd.status == kOk) {
    const bool ref = r.preprocess && b == 0;
    const uint32_t nref = ref ? 1u : 0u;
    const uint32_t id = rd.get(idl);
    uint32_t blocks = 1;
    int option;
    if (id == 0) {
      const uint32_t second = rd.get(1);
      const uint32_t refval = ref ? rd.get(r.nbits) : 0u;
      if (second) {
        option = kOptSecondExt;
        uint32_t budget = block_bits;
        for (uint32_t i = nref; i < J && rd.status == kOk;) {
          const uint32_t m = rd.get_fs(budget);
          budget -= m + 1 <= budget ? m + 1 : budget;
          if (rd.status == kOk && m > kMaxSecondExt) rd.status = kInvalid;
          uint32_t pa = 0, pb = 0;
          if (rd.status == kOk) second_ext_pair(m, &pa, &pb);
          if ((i & 1u) == 0u) put(i++, pa);
          put(i++, pb);
        }
      } else {
        const uint32_t fs = rd.get_fs(kMaxZeroFsBits);
        bool ros = false;
        blocks = zero_run_blocks(fs, b, rsi, &ros);
        option = ros ? kOptZeroRos : kOptZero;
        if (rd.status == kOk && blocks > rsi - b) rd.status = kInvalid;
        if (rd.status != kOk) blocks = 1;
        const uint64_t want = (uint64_t)blocks * J;
        const uint32_t fill = want < (uint64_t)(n - at) ? (uint32_t)want : n - at;
        for (uint32_t j = 0; j < fill; ++j) out[at + j] = 0;
      }
      if (ref) put(0, refval);
    } else if (id == id_raw) {
      option = kOptUncompressed;
      for (uint32_t j = 0; j < J && rd.status == kOk; ++j) put(j, rd.get(r.nbits));
    } else {
      const int k = (int)id - 1;
      option = k ? kOptSplitK : kOptSplit0;
      if (ref) put(0, rd.get(r.nbits));
      const uint32_t nc = J - nref;
      if ((uint64_t)nc * (uint32_t)k >= block_bits && rd.status == kOk) rd.status = kInvalid;
      uint32_t budget = block_bits - nc * (uint32_t)k;
      for (uint32_t i = 0; i < nc && rd.status == kOk; ++i) {
        const uint32_t fs = rd.get_fs(budget);
        budget -= fs + 1 <= budget ? fs + 1 : budget;
        put(nref + i, fs << k);
      }
      for (uint32_t i = 0; i < nc && rd.status == kOk && k; ++i) {
        const uint32_t rem = rd.get(k);
        if (nref + i < n - at) out[at + nref + i] += rem;
      }
    }
    if (rd.status != kOk) break;
    if (hist) {
      ++hist[option];
      if (ref) ++hist[kOptReference];
    }
    const uint64_t adv = (uint64_t)blocks * J;
    at = adv < (uint64_t)(n - at) ? at + (uint32_t)adv : n;
    b += blocks;
    if (b >= rsi) b = 0;
  }
  for (uint32_t i = at; i < n && rd.status != kOk; ++i) out[i] = 0;
  const uint32_t span = J * rsi;   // <= 2^18
  uint32_t xp = 0;
  for (uint32_t i = 0; i < n; ++i) {
    if (!r.preprocess || i % span == 0)
      xp = out[i] & xmax;
    else
      xp = unmap(xp, out[i], xmax);
    out[i] = xp;
  }
  return rd.status;
}

// ---- the encoder: THE RULE OF THIS ENCODER in the head comment, as small functions that encode_row and the kernels of
// smm_grib_aec_pack share
enum : uint32_t { kEncZero = 0, kEncSecondExt = 1, kEncSplit0 = 2 /* + k */, kEncRaw = 255 };
constexpr uint32_t kNoSecondExt = 0xffffffffu;
constexpr uint32_t kFsCap = 4095;   // an FS value counted as at most this: above every uncompressed block (<= 2053 bits)

// the mapped prediction error of x after x_prev: unmap(x_prev, map(x_prev, x, xmax), xmax) == x, and map <= xmax
SMM_GRIB_HD uint32_t map(uint32_t x_prev, uint32_t x, uint32_t xmax) {
  const uint32_t up = xmax - x_prev;
  const uint32_t theta = x_prev < up ? x_prev : up;
  if (x >= x_prev) {
    const uint32_t delta = x - x_prev;
    return delta <= theta ? 2u * delta : theta + delta;
  }
  const uint32_t delta = x_prev - x;
  return delta <= theta ? 2u * delta - 1u : theta + delta;
}
SMM_GRIB_HD uint32_t row_blocks(uint32_t n_values, uint32_t J) { return (uint32_t)(((uint64_t)n_values + J - 1) / J); }
SMM_GRIB_HD uint32_t split_k_max(int idl) { return (1u << idl) - 3u; }
// Symbol i (i < row_blocks * J) of a row of n samples q(0..n): the padding of the last block, the raw reference sample
// at the start of every interval of `span` = J * rsi samples, the mapped error elsewhere.
template <class Q>
SMM_GRIB_HD uint32_t symbol(Q&& q, uint32_t i, uint32_t n, uint32_t span, bool preprocess, uint32_t xmax) {
  if (!preprocess) return i < n ? q(i) & xmax : 0u;
  const uint32_t at = i < n ? i : n - 1;
  if (i % span == 0) return q(at) & xmax;
  const uint32_t before = i - 1 < n ? i - 1 : n - 1;
  return map(q(before) & xmax, q(at) & xmax, xmax);
}
// the second-extension value of the pair (a, b), kNoSecondExt if it is above kMaxSecondExt
SMM_GRIB_HD uint32_t second_ext_value(uint32_t a, uint32_t b) {
  const uint64_t s = (uint64_t)a + b;
  if (s > 12) return kNoSecondExt;
  const uint32_t m = (uint32_t)(s * (s + 1) / 2) + b;
  return m <= kMaxSecondExt ? m : kNoSecondExt;
}
// bits of the FS code of symbol d under split k, as the option search counts them
SMM_GRIB_HD uint32_t fs_len(uint32_t d, uint32_t k) {
  const uint32_t fs = d >> k;
  return (fs < kFsCap ? fs : kFsCap) + 1u;
}
// The option of a block that is not a zero block and its bits.  second_ext_bits: the bits of its second-extension FS
// codes, kNoSecondExt if that is no candidate; fs_bits(k): the sum of fs_len(d, k) over its coded symbols -- called for
// every k in ascending order whatever the sums are (the kernels reduce it over lanes).
struct Choice {
  uint32_t option, bits;
};
template <class F>
SMM_GRIB_HD Choice choose_option(int nbits, uint32_t J, bool ref, uint32_t second_ext_bits, F&& fs_bits) {
  const uint32_t idl = (uint32_t)id_len(nbits), R = ref ? (uint32_t)nbits : 0u, nc = J - (ref ? 1u : 0u);
  Choice c{kEncRaw, idl + J * (uint32_t)nbits};
  if (second_ext_bits != kNoSecondExt && idl + 1u + R + second_ext_bits <= c.bits) c = Choice{kEncSecondExt, idl + 1u + R + second_ext_bits};
  const uint32_t kmax = split_k_max((int)idl);
  for (uint32_t k = 0; k <= kmax; ++k) {
    const uint32_t bits = idl + R + fs_bits(k) + nc * k;
    if (bits < c.bits) c = Choice{kEncSplit0 + k, bits};
  }
  return c;
}
// the FS value that codes a zero run of c (1..64) blocks; at_end: the run reaches the end of its segment or RSI
SMM_GRIB_HD uint32_t zero_run_fs(uint32_t c, bool at_end) { return c >= kRos && at_end ? kRos - 1u : c < kRos ? c - 1u : c; }
// blocks from block b of the RSI to the end of its segment or of the RSI
SMM_GRIB_HD uint32_t blocks_to_end(uint32_t b, uint32_t rsi) {
  const uint32_t to_rsi = rsi - b, to_seg = kSegmentBlocks - (b % kSegmentBlocks);
  return to_rsi < to_seg ? to_rsi : to_seg;
}
// The bound of a row's stream: every block uncompressed, in bytes, rounded up to 4.  No option is chosen unless it is at
// most that long, and a zero run of c blocks takes fewer bits than one uncompressed block.
SMM_GRIB_HD uint64_t pack_bound_bytes(uint64_t n_values, int nbits, int J) {
  if (nbits <= 0 || J <= 0) return 0;
  const uint64_t blocks = (n_values + (uint64_t)J - 1) / (uint64_t)J;
  return smm_grib::align4((blocks * (uint64_t)(id_len(nbits) + J * nbits) + 7) / 8);
}

// bits MSB first into bytes that are zero beforehand; a bit beyond cap_bits is dropped and remembered
struct Writer {
  uint8_t* out;
  uint64_t cap_bits, pos;
  bool ok;
  SMM_GRIB_HD void put(uint32_t v, int n) {
    for (int i = n - 1; i >= 0; --i, ++pos) {
      if (pos >= cap_bits) {
        ok = false;
        continue;
      }
      if ((v >> i) & 1u) out[pos >> 3] |= (uint8_t)(0x80u >> (pos & 7));
    }
  }
  SMM_GRIB_HD void put_fs(uint32_t fs) {
    pos += fs;
    put(1u, 1);
  }
};

// Encodes the r.n_values samples q(0), q(1), ... (r.byte_off and r.byte_len are not read) into out[0, cap_bytes), which
// holds zeros; hist: kNumOptions counters that are added to as decode_row counts them, or null.  Returns the stream's
// bytes, UINT64_MAX if they do not fit (cap_bytes below pack_bound_bytes).
template <class Q>
SMM_GRIB_HD uint64_t encode_row(Q&& q, const Row& r, uint8_t* out, uint64_t cap_bytes, uint64_t* hist) {
  const uint32_t n = r.n_values, J = (uint32_t)r.block, rsi = (uint32_t)r.rsi, span = J * rsi;
  const int idl = id_len(r.nbits);
  const uint32_t xmax = smm_grib::sample_max(r.nbits), nb = row_blocks(n, J);
  Writer w{out, 8 * cap_bytes, 0, true};
  uint32_t s[kSegmentBlocks];   // J <= 64 symbols
  auto load = [&](uint32_t blk, bool ref) {   // the block's symbols; are its coded ones all zero
    uint32_t any = 0;
    for (uint32_t p = 0; p < J; ++p) {
      s[p] = symbol(q, blk * J + p, n, span, r.preprocess, xmax);
      if (p > 0 || !ref) any |= s[p];
    }
    return any == 0u;
  };
  for (uint32_t blk = 0; blk < nb;) {
    const uint32_t b = blk % rsi;
    const bool ref = r.preprocess && b == 0;
    const uint32_t nref = ref ? 1u : 0u;
    const bool zero = load(blk, ref);
    const uint32_t refval = s[0];
    if (hist && ref) ++hist[kOptReference];
    if (zero) {
      const uint32_t to_end = blocks_to_end(b, rsi);
      uint32_t c = 1;
      while (c < to_end && blk + c < nb && load(blk + c, false)) ++c;
      const uint32_t fs = zero_run_fs(c, c == to_end);
      w.put(0u, idl + 1);
      if (ref) w.put(refval, r.nbits);
      w.put_fs(fs);
      if (hist) ++hist[fs == kRos - 1u ? kOptZeroRos : kOptZero];
      blk += c;
      continue;
    }
    uint32_t se = 0;
    for (uint32_t p = 0; p < J && se != kNoSecondExt; p += 2) {
      const uint32_t m = second_ext_value(p == 0 && ref ? 0u : s[p], s[p + 1]);
      se = m == kNoSecondExt ? kNoSecondExt : se + m + 1u;
    }
    const Choice ch = choose_option(r.nbits, J, ref, se, [&](uint32_t k) {
      uint32_t sum = 0;
      for (uint32_t p = nref; p < J; ++p) sum += fs_len(s[p], k);
      return sum;
    });
    if (ch.option == kEncRaw) {
      w.put((1u << idl) - 1u, idl);
      for (uint32_t p = 0; p < J; ++p) w.put(s[p], r.nbits);
      if (hist) ++hist[kOptUncompressed];
    } else if (ch.option == kEncSecondExt) {
      w.put(1u, idl + 1);
      if (ref) w.put(refval, r.nbits);
      for (uint32_t p = 0; p < J; p += 2) w.put_fs(second_ext_value(p == 0 && ref ? 0u : s[p], s[p + 1]));
      if (hist) ++hist[kOptSecondExt];
    } else {
      const uint32_t k = ch.option - kEncSplit0;
      w.put(k + 1u, idl);
      if (ref) w.put(refval, r.nbits);
      for (uint32_t p = nref; p < J; ++p) w.put_fs(s[p] >> k);
      for (uint32_t p = nref; p < J && k; ++p) w.put(s[p] & ((1u << k) - 1u), (int)k);
      if (hist) ++hist[k ? kOptSplitK : kOptSplit0];
    }
    ++blk;
  }
  return w.ok ? (w.pos + 7) / 8 : UINT64_MAX;
}

}  // namespace smm_aec
