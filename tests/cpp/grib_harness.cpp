// Stand-alone check of the GRIB code that needs no device, built with -fsanitize=address,undefined by
// tests/test_grib_harness.py: grib_extract / grib_decode of smm_grib_codec.hpp -- the very functions the kernel of
// smm_apply_grib runs -- and check_grib_rules / check_grib_ranges / plan_grib_chunks of smm_grib_plan.cpp.
// Prints "<NAME>BAD <count> ..." lines; a count of 0 is a pass.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <random>
#include <string>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "../../smmregrid_amd/csrc/smm_grib_codec.hpp"
#include "../../smmregrid_amd/csrc/smm_internal.h"

namespace {

// bit i of the big-endian stream
inline unsigned bit_at(const uint8_t* b, uint64_t i) { return (b[i >> 3] >> (7 - (i & 7))) & 1u; }

// every width x every byte offset 0..3 x value counts whose last value ends on the buffer's last byte.  The heap block
// holds exactly align4(x_bytes) bytes: a load past it is an AddressSanitizer report.
int extract_bad(long* checked) {
  std::mt19937_64 rng(20261018);
  int bad = 0;
  for (int nbits = 0; nbits <= 32; ++nbits)
    for (int off = 0; off < 4; ++off)
      for (int count : {1, 2, 3, 5, 8, 31, 64, 97}) {
        uint64_t data_bytes = smm_grib::row_bytes((uint64_t)count, nbits);
        if (nbits > 0)   // whole bytes: pick counts so that the stream ends on a byte boundary, i.e. on the last byte
          while (((uint64_t)count * nbits) % 8) ++count, data_bytes = smm_grib::row_bytes((uint64_t)count, nbits);
        const uint64_t x_bytes = (uint64_t)off + data_bytes;
        const uint64_t alloc = smm_grib::align4(x_bytes);
        uint8_t* buf = (uint8_t*)std::malloc(alloc ? alloc : 1);
        if (!buf) return -1;
        for (uint64_t i = 0; i < alloc; ++i) buf[i] = (uint8_t)rng();
        const uint32_t last_word = alloc ? (uint32_t)(alloc / 4 - 1) : 0;
        // the kernel's addressing: words from byte_off & ~3, first bit 8 * (byte_off & 3)
        const uint32_t* words = (const uint32_t*)buf;
        for (int i = 0; i < count; ++i) {
          uint32_t want = 0;
          for (int k = 0; k < nbits; ++k) want = (want << 1) | bit_at(buf, 8ull * off + (uint64_t)i * nbits + k);
          if (alloc == 0) continue;   // no bytes at all: the entries substitute their row table for x
          const uint32_t got = smm_grib::grib_extract(words, 8ull * off + (uint64_t)i * nbits, nbits, last_word);
          bad += got != want;
          ++*checked;
        }
        // a 0-bit row that starts at the very end of the buffer: the clamp keeps the loads inside
        if (alloc) bad += smm_grib::grib_extract(words, 8ull * x_bytes, 0, last_word) != 0;
        std::free(buf);
      }
  return bad;
}

template <bool DIV>
float decode_statement(uint32_t q, double ref, double bscale, double ddiv) {
  volatile double x = (double)q;          // the numpy statement, one rounded operation per line
  volatile double m = x * bscale;
  volatile double s = ref + m;
  volatile double t = DIV ? s / ddiv : s;
  return (float)t;
}

int decode_bad(long* checked, int* subnormals, int* infs, int* ties) {
  int bad = 0;
  const uint32_t qs[] = {0u, 1u, 2u, 0x7fu, 0xfffu, 0xffffu, 0x1ffffu, 0xffffffu, 0x1000001u, 0x1000003u, 0x1fffffdu,
                         0x7fffffffu, 0xffffff7fu, 0xffffff80u, 0xffffffffu, 0x9e3779b9u};
  const int Es[] = {-140, -30, -12, -1, 0, 3, 60, 127};
  const double refs[] = {0.0, -273.15, 101325.0, -1.0e-3, 16777216.0, 3.0e38};
  const int Ds[] = {0, 2, -1};
  for (uint32_t q : qs)
    for (int E : Es)
      for (double ref : refs)
        for (int D : Ds) {
          const double bscale = std::ldexp(1.0, E), ddiv = std::pow(10.0, D);
          const float want = decode_statement<true>(q, ref, bscale, ddiv);
          const float got = smm_grib::grib_decode<true>(q, ref, bscale, ddiv);
          bad += std::memcmp(&want, &got, 4) != 0;
          if (ddiv == 1.0) {   // DIV = false: the same bits
            const float g2 = smm_grib::grib_decode<false>(q, ref, bscale, ddiv);
            bad += std::memcmp(&want, &g2, 4) != 0;
          }
          *subnormals += (want != 0.0f && std::fabs(want) < std::numeric_limits<float>::min());
          *infs += std::isinf(want);
          *ties += (E == 0 && ref == 0.0 && D == 0 && q > (1u << 24) && (q & 1u));
          ++*checked;
        }
  return bad;
}

smm_grib_row_t row(uint64_t off, int nbits) { return smm_grib_row_t{off, 0.0, 1.0, 1.0, nbits, 0}; }

int checks_bad() {
  int bad = 0;
  std::string err;
  std::vector<smm_grib_row_t> r = {row(0, 16), row(3, 12), row(40, 0)};
  bad += !smm::check_grib_rules(r.data(), 3, err);
  // 10 values: 20 B at 16 bits from 0, 15 B at 12 bits from 3, nothing at 0 bits from 40 = x_bytes
  bad += !smm::check_grib_ranges(r.data(), nullptr, 3, 10, 40, err);
  bad += smm::check_grib_ranges(r.data(), nullptr, 3, 10, 39, err);            // the 0-bit row starts past the end
  r[1].byte_off = 26;                                                  // 26 + 15 = 41 > 40
  bad += smm::check_grib_ranges(r.data(), nullptr, 3, 10, 40, err) || err.find("rows[1]") == std::string::npos;
  r[1].byte_off = 25;                                                  // ends exactly at x_bytes
  bad += !smm::check_grib_ranges(r.data(), nullptr, 3, 10, 40, err);
  r[1].byte_off = ~0ull - 3;                                           // no wrap-around
  bad += smm::check_grib_ranges(r.data(), nullptr, 3, 10, 40, err);
  r[1] = row(0, 33);
  bad += smm::check_grib_rules(r.data(), 3, err) || err.find("nbits") == std::string::npos;
  r[1] = row(0, 8);
  r[1].bscale = 6.0;
  bad += smm::check_grib_rules(r.data(), 3, err) || err.find("bscale") == std::string::npos;
  r[1].bscale = std::ldexp(1.0, -1074);                                // a power of two, but subnormal
  bad += smm::check_grib_rules(r.data(), 3, err);
  r[1].bscale = 1.0;
  r[1].ddiv = 0.0;
  bad += smm::check_grib_rules(r.data(), 3, err) || err.find("ddiv") == std::string::npos;
  r[1].ddiv = 1.0;
  r[1].ref = std::nan("");
  bad += smm::check_grib_rules(r.data(), 3, err) || err.find("ref") == std::string::npos;
  r[1].ref = 0.0;
  r[1].reserved = 7;
  bad += smm::check_grib_rules(r.data(), 3, err) || err.find("reserved") == std::string::npos;
  return bad;
}

// consecutive, covering, x_bytes as defined, and under the bound wherever a chunk has more than one row
int plan_ok(const smm::GribChunkPlan& p, const std::vector<smm_grib_row_t>& rows, int64_t S, int64_t D, int64_t requested) {
  int bad = 0;
  int64_t next = 0;
  size_t max_x = 0;
  int64_t max_rows = 0;
  for (const smm::GribChunk& c : p.chunks) {
    bad += c.r0 != next || c.nr < 1;
    size_t x = 0;
    for (int64_t b = c.r0; b < c.r0 + c.nr; ++b)
      x += 40 + (size_t)smm_grib::align4(smm_grib::row_bytes((uint64_t)S, rows[(size_t)b].nbits));
    bad += x != c.x_bytes;
    if (requested > 0) bad += c.nr != std::min<int64_t>(requested, (int64_t)rows.size() - c.r0);
    else if (c.nr > 1) bad += x + (size_t)c.nr * D * 8 > p.target;
    max_x = std::max(max_x, x);
    max_rows = std::max(max_rows, c.nr);
    next += c.nr;
  }
  bad += next != (int64_t)rows.size() || max_x != p.max_x || max_rows != p.max_rows;
  return bad;
}

int plan_bad(int* multi_row_chunks, int* single_over_target) {
  int bad = 0;
  const size_t MiB = (size_t)1 << 20;
  // config-4 geometry: 6.6 M source cells at 16 bits, 786432 target cells, 128 rows: 13 MB + 6 MB per row
  std::vector<smm_grib_row_t> rows(128, row(0, 16));
  smm::GribChunkPlan p = smm::plan_grib_chunks(rows.data(), nullptr, 128, 1, 6599680, 786432, 0, (size_t)200 << 30);
  bad += plan_ok(p, rows, 6599680, 786432, 0);
  bad += p.target > 256 * MiB || p.target < 32 * MiB || p.chunks.size() < 8;
  *multi_row_chunks += p.max_rows > 1;
  // mixed widths with 0-bit rows: a chunk is sized by bytes, so the thin rows gather in long chunks
  for (size_t b = 0; b < rows.size(); ++b) rows[b].nbits = (b % 4 == 0) ? 0 : (b % 4 == 1 ? 12 : (b % 4 == 2 ? 24 : 7));
  p = smm::plan_grib_chunks(rows.data(), nullptr, 128, 1, 6599680, 1000, 0, 0);
  bad += plan_ok(p, rows, 6599680, 1000, 0);
  std::vector<smm_grib_row_t> thin(1000, row(0, 0));
  p = smm::plan_grib_chunks(thin.data(), nullptr, 1000, 1, 6599680, 10, 0, 0);
  bad += plan_ok(p, thin, 6599680, 10, 0) || p.chunks.size() != 1 || p.chunks[0].x_bytes != 40000;
  // a single row larger than the target still gets a chunk of one; free memory bounds the target
  std::vector<smm_grib_row_t> fat(3, row(0, 32));
  p = smm::plan_grib_chunks(fat.data(), nullptr, 3, 1, 100000000, 5, 0, 64 * MiB);      // 400 MB per row, target 8 MiB
  bad += plan_ok(p, fat, 100000000, 5, 0) || p.chunks.size() != 3 || p.target != 8 * MiB;
  *single_over_target += p.chunks[0].x_bytes > p.target;
  // chunk_rows overrides the plan
  p = smm::plan_grib_chunks(rows.data(), nullptr, 128, 1, 6599680, 786432, 5, 0);
  bad += plan_ok(p, rows, 6599680, 786432, 5) || p.chunks.size() != 26 || p.chunks.back().nr != 3;
  p = smm::plan_grib_chunks(rows.data(), nullptr, 7, 1, 100, 50, 1000, 0);
  bad += plan_ok(p, std::vector<smm_grib_row_t>(rows.begin(), rows.begin() + 7), 100, 50, 1000) || p.chunks.size() != 1;
  p = smm::plan_grib_chunks(rows.data(), nullptr, 0, 1, 100, 50, 0, 0);
  bad += !p.chunks.empty();
  // a seeded sweep
  std::mt19937_64 rng(7);
  for (int it = 0; it < 300; ++it) {
    const int64_t n = 1 + (int64_t)(rng() % 200), S = 1 + (int64_t)(rng() % 3000000), D = 1 + (int64_t)(rng() % 500000);
    std::vector<smm_grib_row_t> rr((size_t)n);
    for (auto& q : rr) q = row(0, (int)(rng() % 33));
    const int64_t req = (it % 3 == 0) ? 1 + (int64_t)(rng() % 9) : 0;
    const size_t free_b = (it % 5 == 0) ? (size_t)(rng() % (8ull << 30)) : 0;
    p = smm::plan_grib_chunks(rr.data(), nullptr, n, 1, S, D, req, free_b);
    bad += plan_ok(p, rr, S, D, req);
    *multi_row_chunks += p.max_rows > 1;
  }
  return bad;
}

}  // namespace

int main() {
  long n_extract = 0, n_decode = 0;
  int sub = 0, infs = 0, ties = 0, multi = 0, over = 0;
  const int eb = extract_bad(&n_extract);
  std::printf("EXTRACTBAD %d %ld\n", eb, n_extract);
  const int db = decode_bad(&n_decode, &sub, &infs, &ties);
  std::printf("DECODEBAD %d %ld %d %d %d\n", db, n_decode, sub, infs, ties);
  std::printf("CHECKBAD %d\n", checks_bad());
  const int pb = plan_bad(&multi, &over);
  std::printf("PLANBAD %d %d %d\n", pb, multi, over);
  return 0;
}
