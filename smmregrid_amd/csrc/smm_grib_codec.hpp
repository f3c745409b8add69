// GRIB simple packing: the bit extraction and the decode of smm_apply_grib (rule: smm_grib_row_t in
// include/smmregrid_amd.h), as two small functions that the kernel (smm_grib.hip) and plain host code share -- this
// header needs no HIP: tests/cpp/grib_harness.cpp compiles it with g++ and checks the very code the kernel runs.
// Below them the bitmap arithmetic of smm_apply_grib_bm (tests/cpp/grib_bitmap_harness.cpp).
#pragma once

#include <cstdint>

#include "../../include/smmregrid_amd.h"

#if defined(__HIPCC__)
#define SMM_GRIB_HD __host__ __device__ __forceinline__
#else
#define SMM_GRIB_HD inline
#endif

namespace smm_grib {

// bytes a row of n values of nbits bits occupies; a byte count rounded up to whole 4-byte words
SMM_GRIB_HD uint64_t row_bytes(uint64_t n, int nbits) { return (n * (uint64_t)nbits + 7) / 8; }
SMM_GRIB_HD uint64_t align4(uint64_t bytes) { return (bytes + 3) & ~(uint64_t)3; }

// The unsigned big-endian integer of nbits (0..32) bits at bit position p of the byte stream that `words` holds, read
// as 32-bit words: word p / 32 and the one after it, both clamped to last_word (the last word of the buffer: nothing
// past the buffer's bytes rounded up to 4 is ever read; a value that ends inside the last word needs nothing from
// beyond it, and nbits == 0 needs nothing at all).  Both loads are unconditional.
// A row of fewer than 2^31 values of at most 32 bits spans fewer than 2^31 + 1 words: word indices are 32-bit.
SMM_GRIB_HD uint32_t grib_extract(const uint32_t* __restrict__ words, uint64_t p, int nbits, uint32_t last_word) {
  const uint32_t w = (uint32_t)(p >> 5);
  const uint32_t w0 = w < last_word ? w : last_word;
  const uint32_t w1 = w < last_word ? w + 1 : last_word;
  const uint64_t hi = __builtin_bswap32(words[w0]);   // the stream is big-endian: the first word is the upper one
  const uint64_t lo = __builtin_bswap32(words[w1]);
  const uint64_t both = (hi << 32) | lo;
  const unsigned shift = (unsigned)(64 - (int)(p & 31) - nbits) & 63u;
  const uint32_t mask = (uint32_t)((1ull << nbits) - 1ull);
  return (uint32_t)(both >> shift) & mask;
}

// ---- a byte range of x read as a bit stream that may begin and end at any byte: what the CCSDS and the complex-packed
// decoders (smm_grib_aec.hpp, smm_grib_cpx.hpp) read their streams through.
// the largest unsigned integer of nbits (0..32) bits
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

// q -> the float32 field value: float64 arithmetic, multiply and add kept apart, IEEE division (DIV = false leaves it
// out: the caller guarantees ddiv == 1.0, and t / 1.0 has the bits of t), one round-to-nearest-even conversion.
// The multiply and the add must not be contracted into an FMA: clang is told so inside the function (the pragma ends
// with its block and changes nothing for the including file); any other compiler needs -ffp-contract=off on its
// command line, as tests/test_grib_harness.py passes to g++.
template <bool DIV>
SMM_GRIB_HD float grib_decode(uint32_t q, double ref, double bscale, double ddiv) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  double t = (double)q * bscale;
  t = ref + t;
  if (DIV) t = t / ddiv;
  return (float)t;
}

// ---- bitmaps (smm_apply_grib_bm): the packed stream of a bitmapped row holds the present cells only, and cell c's
// value is packed value number rank(c) = set bitmap bits before c.  The rank table has one entry per 32 cells.
struct alignas(8) GribRankEntry {
  uint32_t bits;          // bitmap bits [32k, 32k + 32) in stream order: cell 32k is the top bit
  uint32_t rank_before;   // set bits among cells [0, 32k); n_src < 2^31
};
// 32-cell blocks of one segment of the table build: a (row, segment) workgroup counts, then scans, this many blocks
// (smm_grib.hip: 256 threads x 4 blocks) -- 32768 cells
constexpr int kGribSegBlocks = 1024;
SMM_GRIB_HD uint64_t bitmap_bytes(uint64_t n_src) { return (n_src + 7) / 8; }
inline uint64_t bitmap_blocks(uint64_t n_src) { return (n_src + 31) / 32; }
inline uint64_t bitmap_segments(uint64_t n_src) { return (bitmap_blocks(n_src) + kGribSegBlocks - 1) / kGribSegBlocks; }

// Block k (32 * k < n_src) of the bitmap whose first bit is bit bit0 of `words`: grib_extract's clamped two-word
// window with nbits = 32 -- the bitmap may start at any byte.  Bits of cells >= n_src (the last byte's pad, whatever
// follows the bitmap, the clamped second word) are cleared: they reach neither a rank nor a total.
SMM_GRIB_HD uint32_t bitmap_block(const uint32_t* __restrict__ words, uint32_t bit0, uint32_t k, uint32_t n_src,
                                  uint32_t last_word) {
  const uint32_t b = grib_extract(words, (uint64_t)bit0 + 32ull * k, 32, last_word);
  const uint32_t left = n_src - 32u * k;   // cells from 32k on: >= 1
  return left >= 32u ? b : b & ~(0xffffffffu >> left);
}
SMM_GRIB_HD uint32_t popcount32(uint32_t v) { return (uint32_t)__builtin_popcount(v); }
// is cell c present, by its block's entry
SMM_GRIB_HD bool bitmap_present(GribRankEntry e, uint32_t c) { return ((e.bits >> (31u - (c & 31u))) & 1u) != 0u; }
// Index of cell c's value in the packed stream: the block's rank plus the set bits above c's bit.  c % 32 == 0 has
// none above it: the shift is taken in two steps (by 1, then by 31 - c % 32 <= 31), never by 32.  A missing cell gets
// the index of the next present one: its loads are issued all the same, the caller replaces the value by NaN.
SMM_GRIB_HD uint32_t bitmap_index(GribRankEntry e, uint32_t c) {
  return e.rank_before + popcount32((e.bits >> 1) >> (31u - (c & 31u)));
}

// ---- the encode (smm_grib_pack / smm_apply_host_grib_pk; numpy: smmregrid_amd.GribEncode.encode).  THE RULE, for one
// batch row with a requested width nbits in 1..32 and ddiv = 10^D > 0, on float64 result values v:
//   t = v * ddiv                                  one rounding
//   present  iff  v is finite and |t| <= FLT_MAX; every other cell (NaN, +-inf, overflow) is missing
//   tmin, tmax = min, max of t over the present cells; n_values = their count
//   R = the largest float32 <= tmin: round to nearest, one float32 down if that lies above tmin
//   ref = (double)R + 0.0                         (a reference of -0 is stored as +0: min(-0, +0) has no order)
//   range = tmax - ref                            one rounding
//   range == 0 or n_values == 0: stored width 0, E = 0, no data bits; n_values == 0: ref = 0
//   else E = the smallest integer with range * 2^-E <= 2^nbits - 1 -- frexp(range) = (m, e): e - nbits when
//        m * 2^nbits <= 2^nbits - 1, else e - nbits + 1 -- raised to -1022 if below; bscale = 2^E; stored width nbits
//   q = rint(ldexp(t - ref, -E))                  the subtraction rounds once, the scaling is exact, ties to even
// 0 <= q <= 2^nbits - 1 follows: t <= tmax and rounding is monotonic, so t - ref <= range.  No multiply-add pair of it
// may be contracted (the pragma of grib_decode, -ffp-contract=off elsewhere).
constexpr double kGribFltMax = 3.4028234663852886e38;

// t of a cell and whether the cell is present
SMM_GRIB_HD bool grib_encode_t(double v, double ddiv, double* t) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  *t = v * ddiv;
  return __builtin_isfinite(v) && __builtin_fabs(*t) <= kGribFltMax;
}

struct GribPackRule {   // what the rule pass leaves per row on the device; 24 B
  double ref;
  int32_t E;
  int32_t width;       // the stored width: the requested one, or 0
  uint32_t n_values;   // present cells; n_dst < 2^31
  uint32_t pad;
};

// the rule of a row from its tmin / tmax / n_values
SMM_GRIB_HD GribPackRule grib_encode_rule(double tmin, double tmax, uint32_t n_values, int nbits) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  GribPackRule r{0.0, 0, 0, n_values, 0u};
  if (n_values == 0) return r;
  float R = (float)tmin;
  if ((double)R > tmin) {   // one float32 down, on the bits: 0 -> the negative subnormal next to it
    uint32_t u;
    __builtin_memcpy(&u, &R, 4);
    if ((u & 0x7fffffffu) == 0u)
      u = 0x80000001u;
    else if (u >> 31)
      u += 1u;
    else
      u -= 1u;
    __builtin_memcpy(&R, &u, 4);
  }
  r.ref = (double)R + 0.0;
  const double range = tmax - r.ref;
  if (range == 0.0) return r;
  int e = 0;
  const double m = __builtin_frexp(range, &e);
  const double top = __builtin_ldexp(1.0, nbits);   // 2^nbits
  int E = __builtin_ldexp(m, nbits) <= top - 1.0 ? e - nbits : e - nbits + 1;
  if (E < -1022) E = -1022;
  r.E = E;
  r.width = nbits;
  return r;
}

// q of a present cell's t
SMM_GRIB_HD uint32_t grib_encode_q(double t, double ref, int E) {
#if defined(__clang__)
#pragma clang fp contract(off)
#endif
  const double d = t - ref;
  return (uint32_t)__builtin_rint(__builtin_ldexp(d, -E));
}

// The output layout: row b owns a slot of align4(ceil(n_dst / 8)) bitmap bytes and align4(ceil(n_dst * nbits_b / 8))
// stream bytes, slots back to back in row order
SMM_GRIB_HD uint64_t pack_bitmap_bytes(uint64_t n_dst) { return align4(bitmap_bytes(n_dst)); }
SMM_GRIB_HD uint64_t pack_slot_bytes(uint64_t n_dst, int nbits) { return pack_bitmap_bytes(n_dst) + align4(row_bytes(n_dst, nbits)); }

// What value number i (at bit i * width of the row's stream) contributes to the stream's 32-bit word w, as the
// big-endian number the word holds: q shifted to its place, the bits that belong to the neighbouring words dropped.
// The value must overlap the word: 32 * w - width < i * width < 32 * w + 32.
SMM_GRIB_HD uint32_t grib_word_part(uint32_t q, uint64_t i, int width, uint64_t w) {
  const int shift = (int)((int64_t)(32 * w + 32) - (int64_t)(i * (uint64_t)width) - width);   // -31 .. 31
  return shift >= 0 ? (uint32_t)((uint64_t)q << shift) : q >> (-shift);
}
// the values [first, end) that overlap word w of a stream of n_values values of `width` (>= 1) bits; end <= first: none
SMM_GRIB_HD void grib_word_values(uint64_t w, int width, uint64_t n_values, uint64_t* first, uint64_t* end) {
  *first = (32 * w) / (uint64_t)width;
  const uint64_t e = (32 * w + 32 + (uint64_t)width - 1) / (uint64_t)width;
  *end = e < n_values ? e : n_values;
}
// Word w of a row's stream as the big-endian number it holds: what one thread of the pack kernel computes.  y: the row's
// n_dst result values; rule: the row's; tab: the row's rank table of n_blocks entries, read only when cells are missing.
// The values that overlap the word are found, their q recomputed from y, and put in place.  With every cell present
// value i is cell i; else the block of the first value is the last one whose rank_before <= i (binary search), the value
// is that block's (i - rank_before)-th set bit from the top, and the set bits are walked forward from there.  A word
// the stream does not reach, and every word of a width-0 row, is 0.
SMM_GRIB_HD uint32_t grib_pack_word(const double* __restrict__ y, double ddiv, const GribPackRule& rule, uint32_t n_dst,
                                    const GribRankEntry* __restrict__ tab, uint32_t n_blocks, uint32_t w) {
  uint32_t word = 0;
  if (rule.width <= 0) return word;
  uint64_t i = 0, end = 0;
  grib_word_values(w, rule.width, rule.n_values, &i, &end);
  if (i >= end) return word;
  if (rule.n_values == n_dst) {
    for (; i < end; ++i) {
      double t;
      (void)grib_encode_t(y[i], ddiv, &t);
      word |= grib_word_part(grib_encode_q(t, rule.ref, rule.E), i, rule.width, w);
    }
    return word;
  }
  uint32_t lo = 0, hi = n_blocks - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (tab[mid].rank_before <= (uint32_t)i)
      lo = mid;
    else
      hi = mid - 1;
  }
  uint32_t k = lo, bits = tab[lo].bits;
  for (uint32_t skip = (uint32_t)i - tab[lo].rank_before; skip > 0 && bits != 0u; --skip)
    bits &= ~(0x80000000u >> __builtin_clz(bits));
  for (; i < end; ++i) {
    while (bits == 0u && k + 1 < n_blocks) bits = tab[++k].bits;   // i < n_values: a set bit lies ahead
    if (bits == 0u) break;                                          // (a table that disagrees with n_values: stop)
    const uint32_t pos = (uint32_t)__builtin_clz(bits);
    bits &= ~(0x80000000u >> pos);
    double t;
    (void)grib_encode_t(y[32u * k + pos], ddiv, &t);
    word |= grib_word_part(grib_encode_q(t, rule.ref, rule.E), i, rule.width, w);
  }
  return word;
}

}  // namespace smm_grib

// smm_apply_grib_bm.  The device copy of a row's smm_grib_bitmap_t: n_values, which only the host's size checks
// read, gives its place to the row's rank table.
struct GribRowBitmap {
  uint64_t bitmap_off;   // byte offset of the bitmap in x; SMM_GRIB_NO_BITMAP: the row has none
  uint64_t table_off;    // first entry of the row's table in GribBitmapArgs::table (bitmapped rows only)
};
static_assert(sizeof(GribRowBitmap) == sizeof(smm_grib_bitmap_t), "one record per row, 16 B");
