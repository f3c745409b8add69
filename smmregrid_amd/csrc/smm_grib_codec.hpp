// GRIB simple packing: the bit extraction and the decode of smm_apply_grib (rule: smm_grib_row_t in
// include/smmregrid_amd.h), as two small functions that the kernel (smm_grib.hip) and plain host code share -- this
// header needs no HIP: tests/cpp/grib_harness.cpp compiles it with g++ and checks the very code the kernel runs.
#pragma once

#include <cstdint>

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

}  // namespace smm_grib
