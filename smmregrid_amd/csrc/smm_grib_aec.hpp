// CCSDS 121.0-B adaptive entropy coding as GRIB-2 data representation template 5.42 carries it (what libaec writes
// for ecCodes): the decoder, stated once.  Plain C++ that compiles for host and device -- the host decode
// (smm_grib_aec_decode_host), the kernels of smm_grib_aec_unpack (smm_grib_aec.hip) and tests/cpp/grib_aec_harness.cpp
// all read the stream through load_word / bits_of and take the options apart with the small functions below.
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
SMM_GRIB_HD uint32_t sample_max(int nbits) { return nbits >= 32 ? 0xffffffffu : (1u << nbits) - 1u; }

// Word i of x as the big-endian number it holds, i clamped to last_word.  The device loads the aligned word (the
// allocation covers x_bytes rounded up to 4); the host takes it byte by byte from any address and reads no byte at or
// beyond end_byte (they count as zero).
SMM_GRIB_HD uint32_t load_word(const void* x, uint64_t i, uint64_t last_word, uint64_t end_byte) {
  const uint64_t w = i < last_word ? i : last_word;
#if defined(__HIP_DEVICE_COMPILE__)
  (void)end_byte;
  return __builtin_bswap32(((const uint32_t*)x)[w]);
#else
  const uint8_t* p = (const uint8_t*)x;
  uint32_t v = 0;
  for (uint64_t k = 4 * w; k < 4 * w + 4; ++k) v = (v << 8) | (k < end_byte ? (uint32_t)p[k] : 0u);
  return v;
#endif
}
// the n (0..32) bits at bit `off` (0..31) of the 64 bits hi:lo
SMM_GRIB_HD uint32_t bits_of(uint32_t hi, uint32_t lo, unsigned off, int n) {
  const uint64_t both = ((uint64_t)hi << 32) | lo;
  const unsigned shift = (unsigned)(64 - (int)off - n) & 63u;
  return (uint32_t)(both >> shift) & (uint32_t)((1ull << n) - 1ull);
}

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
    return bits_of(load_word(x, w, last_word, end_byte), load_word(x, w + 1, last_word, end_byte), (unsigned)(p & 31), n);
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
  const uint32_t id_raw = (1u << idl) - 1u, xmax = sample_max(r.nbits), block_bits = J * (uint32_t)r.nbits;
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

}  // namespace smm_aec
