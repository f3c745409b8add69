// The complex-packing encoder of smm_grib_cpx.hpp on the host under AddressSanitizer + UBSan: encode_row, then decode_row
// on what it wrote, on seeded random and adversarial integers over every width class, order and group length, from
// n_values = 1 on (a row of no values has no stream), the rows that overflow a descriptor or a difference among them.  The
// stream is coded into a heap block of exactly the row's bound (pack_bound_bytes), so a bit past the bound is a
// sanitizer report, and decoded from a block of exactly its bytes; every stream must fit, decode ok and give the
// integers back, and the effective order must be the wanted one wherever the width is at most 29 bits.
// tests/test_grib_complex_encode.py compiles and runs this.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_cpx.hpp"

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the integers of one case: `kind` picks the shape
static void fill(std::vector<uint32_t>& v, int kind, uint32_t xmax, uint32_t L) {
  uint32_t walk = (uint32_t)(rnd() & xmax);
  for (size_t i = 0; i < v.size(); ++i) {
    uint32_t x = 0;
    switch (kind) {
      case 0: x = (uint32_t)rnd() & xmax; break;                                         // full-range noise
      case 1: x = 0; break;                                                              // all zero
      case 2: x = xmax; break;                                                           // all ones
      case 3: x = (i & 1) ? xmax : 0u; break;                                            // the widest differences
      case 4: walk = (walk + (uint32_t)(rnd() % 7) - 3u) & xmax; x = walk; break;        // a smooth walk
      case 5: x = (uint32_t)((i * i / 7 + i * 3) & xmax); break;                         // constant second differences
      case 6: x = (i % L == L / 2) ? xmax : (uint32_t)(rnd() & 3u) & xmax; break;        // one spike a group
      case 7: x = ((i / (3 * L)) & 1) ? 5u & xmax : (uint32_t)rnd() & xmax & 0xffu; break;   // groups of width 0 between noise
      case 8: x = (i == 0) ? xmax : (uint32_t)(rnd() & 1u) & xmax; break;                // h_1 at its largest
      default: x = (i == 1) ? xmax : (xmax >> 1); break;                                 // h_2 at its largest
    }
    v[i] = x;
  }
}

int main() {
  const int widths[] = {1, 2, 7, 8, 9, 12, 16, 17, 24, 29, 30, 31, 32};
  const uint32_t lengths[] = {8, 16, 32, 64};
  long cases = 0, fallbacks = 0;
  for (int nbits : widths)
    for (uint32_t L : lengths)
      for (int order = 0; order < 3; ++order)
        for (int kind = 0; kind < 10; ++kind) {
          const uint32_t sizes[] = {1u, 2u, 3u, L - 1u, L, L + 1u, (uint32_t)(rnd() % 700) + 1u, 1030u};
          const uint32_t n = sizes[(cases + kind) % 8];
          const uint32_t xmax = smm_grib::sample_max(nbits);
          std::vector<uint32_t> v(n), back(n + 1);
          fill(v, kind, xmax, L);
          const uint64_t bound = smm_cpx::pack_bound_bytes(n, nbits, order, L);
          uint8_t* out = new uint8_t[bound + (bound == 0)];
          memset(out, 0, bound);
          const smm_cpx::Want want{n, nbits, order, L};
          smm_cpx::Row row{};
          const uint32_t* src = v.data();
          const uint64_t len = smm_cpx::encode_row([src](uint32_t i) { return src[i]; }, want, out, bound, &row);
          ++cases;
          if (len == UINT64_MAX || len > bound || len != row.byte_len) {
            fprintf(stderr, "case %ld (w %d L %u order %d kind %d n %u): %llu bytes pass the bound of %llu\n", cases, nbits, L, order,
                    kind, n, (unsigned long long)len, (unsigned long long)bound);
            return 1;
          }
          const int expect = n > (uint32_t)order ? order : 0;
          if (row.order != expect) {
            ++fallbacks;
            if (nbits <= 29 || row.order != 0) {
              fprintf(stderr, "case %ld (w %d L %u order %d kind %d n %u): coded at order %d\n", cases, nbits, L, order, kind, n,
                      row.order);
              return 1;
            }
          }
          // decode from a block of exactly the stream's bytes
          uint8_t* exact = new uint8_t[len + (len == 0)];
          memcpy(exact, out, len);
          back[n] = 0xFEEDFACEu;
          const int st = smm_cpx::decode_row(exact, row, back.data());
          const bool same = memcmp(back.data(), v.data(), 4 * (size_t)n) == 0;
          delete[] exact;
          delete[] out;
          if (st != smm_cpx::kOk || !same || back[n] != 0xFEEDFACEu) {
            fprintf(stderr, "case %ld (w %d L %u order %d kind %d n %u): status %d, integers %s\n", cases, nbits, L, order, kind, n,
                    st, same ? "equal" : "differ");
            return 1;
          }
        }
  if (fallbacks == 0) {
    fprintf(stderr, "no row fell back to order 0: the overflow rows are missing\n");
    return 1;
  }
  printf("%ld cases, fallbacks %ld\n", cases, fallbacks);
  return 0;
}
