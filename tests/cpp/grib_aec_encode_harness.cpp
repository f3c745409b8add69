// The CCSDS encoder of smm_grib_aec.hpp on the host under AddressSanitizer + UBSan: encode_row, then decode_row on what it
// wrote, on seeded random and adversarial integers over every width class, block size and a spread of reference sample
// intervals, with and without the preprocessor, from n_values = 0 on.  The stream is coded into a heap block of exactly
// the row's bound (pack_bound_bytes), so a bit past the bound is a sanitizer report; every stream must fit, decode ok and
// give the integers back, and the two histograms must agree.  tests/test_grib_ccsds_encode.py compiles and runs this.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_aec.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the integers of one case: `kind` picks the shape
static void fill(std::vector<uint32_t>& v, int kind, uint32_t xmax, uint32_t J) {
  uint32_t walk = (uint32_t)(rnd() & xmax);
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t x = 0;
    switch (kind) {
      case 0: x = (uint32_t)rnd() & xmax; break;                                         // full-range noise
      case 1: x = 0; break;                                                              // all zero
      case 2: x = xmax; break;                                                           // all ones
      case 3: x = (i & 1) ? xmax : 0u; break;                                            // the map's far branch
      case 4: walk = (walk + (uint32_t)(rnd() % 7) - 3u) & xmax; x = walk; break;        // a smooth walk
      case 5: x = (uint32_t)(rnd() % 5 == 0) & xmax; break;                              // 0 / 1: second extension
      case 6: x = (i % J == J / 2) ? xmax : (uint32_t)(rnd() & 3u) & xmax; break;        // one spike a block
      case 7: x = ((i / (3 * J)) & 1) ? 0u : (uint32_t)rnd() & xmax & 0xffu; break;      // zero runs between noise
      case 8: x = (uint32_t)(i * 2654435761u) & xmax & (xmax >> (i % 9)); break;         // mixed magnitudes
      default: x = (rnd() % 64 == 0) ? 13u & xmax : (uint32_t)(rnd() & 1u) & xmax; break;   // pairs around the limit of 90
    }
    v[i] = x;
  }
}

int main() {
  const int widths[] = {1, 2, 7, 8, 9, 12, 16, 17, 24, 31, 32};
  const int blocks[] = {8, 16, 32, 64};
  const int rsis[] = {1, 2, 5, 63, 64, 65, 128, 4096};
  long cases = 0;
  uint64_t enc_hist[smm_aec::kNumOptions] = {0}, dec_hist[smm_aec::kNumOptions] = {0};
  for (int nbits : widths)
    for (int J : blocks)
      for (int rsi : rsis)
        for (int pp = 0; pp < 2; ++pp)
          for (int kind = 0; kind < 10; ++kind) {
            const uint32_t span = (uint32_t)J * (uint32_t)rsi;
            const uint32_t sizes[] = {0u, 1u, (uint32_t)J - 1u, (uint32_t)J, (uint32_t)J + 1u, (uint32_t)(rnd() % 700),
                                      span > 3000u ? 777u : span - 1u, span > 3000u ? 1030u : span + 1u};
            const uint32_t n = sizes[(cases + kind) % 8];
            const uint32_t xmax = smm_grib::sample_max(nbits);
            std::vector<uint32_t> v(n), back(n + 1);
            fill(v, kind, xmax, (uint32_t)J);
            const uint64_t bound = smm_aec::pack_bound_bytes(n, nbits, J);
            uint8_t* out = new uint8_t[bound + (bound == 0)];
            memset(out, 0, bound);
            const smm_aec::Row row{0, 0, n, nbits, J, rsi, pp != 0};
            const uint32_t* src = v.data();
            const uint64_t len = smm_aec::encode_row([src](uint32_t i) { return src[i]; }, row, out, bound, enc_hist);
            ++cases;
            if (len == UINT64_MAX || len > bound) {
              fprintf(stderr, "case %ld (w %d J %d rsi %d pp %d kind %d n %u): %llu bytes pass the bound of %llu\n", cases, nbits, J,
                      rsi, pp, kind, n, (unsigned long long)len, (unsigned long long)bound);
              return 1;
            }
            // decode from a block of exactly the stream's bytes
            uint8_t* exact = new uint8_t[len + (len == 0)];
            memcpy(exact, out, len);
            smm_aec::Row r = row;
            r.byte_len = len;
            back[n] = 0xFEEDFACEu;
            const int st = smm_aec::decode_row(exact, r, back.data(), dec_hist);
            const bool same = n == 0 || memcmp(back.data(), v.data(), 4 * (size_t)n) == 0;
            delete[] exact;
            delete[] out;
            if (st != smm_aec::kOk || !same || back[n] != 0xFEEDFACEu) {
              fprintf(stderr, "case %ld (w %d J %d rsi %d pp %d kind %d n %u): status %d, integers %s\n", cases, nbits, J, rsi, pp,
                      kind, n, st, same ? "equal" : "differ");
              return 1;
            }
          }
  for (int o = 0; o < smm_aec::kNumOptions; ++o) {
    if (enc_hist[o] != dec_hist[o] || enc_hist[o] == 0) {
      fprintf(stderr, "option %d: the encoder counts %llu, the decoder %llu\n", o, (unsigned long long)enc_hist[o],
              (unsigned long long)dec_hist[o]);
      return 1;
    }
  }
  printf("%ld cases, options", cases);
  for (int o = 0; o < smm_aec::kNumOptions; ++o) printf(" %llu", (unsigned long long)enc_hist[o]);
  printf("\n");
  return 0;
}
