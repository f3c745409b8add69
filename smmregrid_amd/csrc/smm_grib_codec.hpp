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
inline uint64_t row_bytes(uint64_t n, int nbits) { return (n * (uint64_t)nbits + 7) / 8; }
inline uint64_t align4(uint64_t bytes) { return (bytes + 3) & ~(uint64_t)3; }

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
inline uint64_t bitmap_bytes(uint64_t n_src) { return (n_src + 7) / 8; }
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

}  // namespace smm_grib

// smm_apply_grib_bm.  The device copy of a row's smm_grib_bitmap_t: n_values, which only the host's size checks
// read, gives its place to the row's rank table.
struct GribRowBitmap {
  uint64_t bitmap_off;   // byte offset of the bitmap in x; SMM_GRIB_NO_BITMAP: the row has none
  uint64_t table_off;    // first entry of the row's table in GribBitmapArgs::table (bitmapped rows only)
};
static_assert(sizeof(GribRowBitmap) == sizeof(smm_grib_bitmap_t), "one record per row, 16 B");
