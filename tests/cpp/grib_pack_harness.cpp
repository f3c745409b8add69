// The GRIB encode of smm_grib_pack on the host, from the very functions the kernels run (smm_grib_codec.hpp compiled with
// plain g++ -ffp-contract=off): grib_encode_t / grib_encode_rule / grib_pack_word, the bitmap words and the rank table
// (bitmap_block on the bytes just written, as the build kernels read them), and the layout, the refusals and the scratch
// arithmetic of smm_grib_plan.cpp.  tests/test_grib_pack_harness.py writes a case file, runs this program -- built with
// AddressSanitizer and UBSan -- and compares every byte and record with smmregrid_amd.GribEncode.encode.
//
//   in : int64 n_rows, n_dst, ldy; n_rows x smm_grib_encode_t; n_rows x ldy float64
//   out: uint64 total; n_rows x smm_grib_row_t; n_rows x smm_grib_bitmap_t; total bytes
// Every heap block has exactly the size the layout gives: a store or load outside it is a sanitizer report.
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "../../smmregrid_amd/csrc/smm_grib_codec.hpp"
#include "../../smmregrid_amd/csrc/smm_internal.h"

namespace {

int fail(const char* what) {
  fprintf(stderr, "grib_pack_harness: %s\n", what);
  return 2;
}

// the refusals and the scratch pieces (no input needed); returns the number of wrong answers
int self_checks() {
  int bad = 0;
  std::string err;
  smm_grib_encode_t e{1.0, 16, 0};
  bad += !smm::check_grib_encode(&e, 1, 100, err);
  bad += !smm::check_grib_encode(&e, 1, ((int64_t)1 << 31) - 1, err);
  bad += smm::check_grib_encode(&e, 1, (int64_t)1 << 31, err);
  bad += smm::check_grib_encode(&e, 1, -1, err);
  for (int nbits : {0, -1, 33}) {
    smm_grib_encode_t x = e;
    x.nbits = nbits;
    bad += smm::check_grib_encode(&x, 1, 100, err);
  }
  for (double d : {0.0, -1.0, (double)INFINITY, (double)NAN}) {
    smm_grib_encode_t x = e;
    x.ddiv = d;
    bad += smm::check_grib_encode(&x, 1, 100, err);
  }
  smm_grib_encode_t r = e;
  r.reserved = 1;
  bad += smm::check_grib_encode(&r, 1, 100, err);
  for (int nbits = 1; nbits <= 32; ++nbits) {
    smm_grib_encode_t x = e;
    x.nbits = nbits;
    bad += !smm::check_grib_encode(&x, 1, 100, err);
  }
  // the scratch pieces are disjoint, 8-byte aligned and in order
  for (int64_t n_dst : {1, 33, 32768, 32769, 100000})
    for (int64_t rows : {1, 3, 128}) {
      const smm::GribPackScratch s = smm::grib_pack_scratch(n_dst, rows);
      const size_t segs = (size_t)rows * smm_grib::bitmap_segments(n_dst), blocks = (size_t)rows * smm_grib::bitmap_blocks(n_dst);
      bad += s.part_max < s.part_min + segs * 8 || s.part_cnt < s.part_max + segs * 8 || s.rules < s.part_cnt + segs * 4 ||
             s.table < s.rules + (size_t)rows * sizeof(smm_grib::GribPackRule) || s.totals < s.table + blocks * 8 ||
             s.bytes < s.totals + segs * 4;
      bad += (s.part_max | s.rules | s.table | s.bytes) % 8 != 0 || s.part_cnt % 4 != 0 || s.totals % 4 != 0;
    }
  return bad;
}

}  // namespace

int main(int argc, char** argv) {
  if (argc != 3) return fail("usage: grib_pack_harness <cases in> <packed out>");
  const int bad = self_checks();
  if (bad) return fail(("self checks: " + std::to_string(bad) + " wrong").c_str());

  FILE* in = fopen(argv[1], "rb");
  if (!in) return fail("cannot open the case file");
  int64_t hdr[3];
  if (fread(hdr, 8, 3, in) != 3) return fail("short header");
  const int64_t n_rows = hdr[0], n_dst = hdr[1], ldy = hdr[2];
  std::vector<smm_grib_encode_t> enc((size_t)n_rows);
  std::vector<double> y((size_t)(n_rows * ldy));
  if (fread(enc.data(), sizeof(smm_grib_encode_t), enc.size(), in) != enc.size()) return fail("short encode table");
  if (fread(y.data(), 8, y.size(), in) != y.size()) return fail("short values");
  fclose(in);

  std::string err;
  if (!smm::check_grib_encode(enc.data(), n_rows, n_dst, err)) return fail(err.c_str());
  std::vector<uint64_t> offs((size_t)n_rows);
  const uint64_t total = smm::grib_out_layout(n_dst, enc.data(), n_rows, offs.data());
  std::vector<uint32_t> out((size_t)(total / 4), 0xa5a5a5a5u);   // exactly the layout; every word must be overwritten
  std::vector<uint8_t> written((size_t)(total / 4), 0);
  std::vector<smm_grib_row_t> rows((size_t)n_rows);
  std::vector<smm_grib_bitmap_t> bms((size_t)n_rows);
  const uint32_t n_blocks = (uint32_t)smm_grib::bitmap_blocks((uint64_t)n_dst);
  const uint32_t last_word = (uint32_t)(total / 4 - 1);

  for (int64_t b = 0; b < n_rows; ++b) {
    // a row of exactly n_dst values: the pad of ldy is out of reach
    const std::vector<double> v(y.begin() + b * ldy, y.begin() + b * ldy + n_dst);
    const double ddiv = enc[(size_t)b].ddiv;
    uint32_t* bm_words = out.data() + offs[(size_t)b] / 4;
    // 1: range + bitmap, 64 cells (one ballot) at a time
    double mn = INFINITY, mx = -INFINITY;
    uint32_t cnt = 0;
    for (uint32_t base = 0; base < (uint32_t)n_dst; base += 64) {
      uint64_t bal = 0;
      for (uint32_t l = 0; l < 64 && base + l < (uint32_t)n_dst; ++l) {
        double t;
        if (smm_grib::grib_encode_t(v[base + l], ddiv, &t)) {
          mn = t < mn ? t : mn;
          mx = t > mx ? t : mx;
          ++cnt;
          bal |= 1ull << l;
        }
      }
      auto rev = [](uint32_t x) {
        uint32_t r = 0;
        for (int i = 0; i < 32; ++i) r |= ((x >> i) & 1u) << (31 - i);
        return r;
      };
      const uint32_t k = base >> 5;
      if (k < n_blocks) bm_words[k] = __builtin_bswap32(rev((uint32_t)bal)), written[offs[(size_t)b] / 4 + k] = 1;
      if (k + 1 < n_blocks) bm_words[k + 1] = __builtin_bswap32(rev((uint32_t)(bal >> 32))), written[offs[(size_t)b] / 4 + k + 1] = 1;
    }
    // 2: the rule and the records
    const smm_grib::GribPackRule rule = smm_grib::grib_encode_rule(mn, mx, cnt, enc[(size_t)b].nbits);
    const uint64_t stream_off = offs[(size_t)b] + smm_grib::pack_bitmap_bytes((uint64_t)n_dst);
    rows[(size_t)b] = smm_grib_row_t{stream_off, rule.ref, std::ldexp(1.0, rule.E), ddiv, rule.width, 0};
    bms[(size_t)b] = smm_grib_bitmap_t{cnt == (uint32_t)n_dst ? SMM_GRIB_NO_BITMAP : offs[(size_t)b], cnt};
    // the rank table, from the bitmap bytes as the build kernels read them
    std::vector<smm_grib::GribRankEntry> tab(n_blocks);
    uint32_t rank = 0;
    for (uint32_t k = 0; k < n_blocks; ++k) {
      const uint32_t bits = smm_grib::bitmap_block(out.data() + offs[(size_t)b] / 4, 0, k, (uint32_t)n_dst,
                                                   last_word - (uint32_t)(offs[(size_t)b] / 4));
      tab[k] = smm_grib::GribRankEntry{bits, rank};
      rank += smm_grib::popcount32(bits);
    }
    if (rank != cnt) return fail("the rank table disagrees with the count");
    // 3: pack, word by word
    const uint32_t n_words = (uint32_t)(smm_grib::align4(smm_grib::row_bytes((uint64_t)n_dst, enc[(size_t)b].nbits)) / 4);
    for (uint32_t w = 0; w < n_words; ++w) {
      out[stream_off / 4 + w] =
          __builtin_bswap32(smm_grib::grib_pack_word(v.data(), ddiv, rule, (uint32_t)n_dst, tab.data(), n_blocks, w));
      written[stream_off / 4 + w] = 1;
    }
  }
  for (size_t i = 0; i < written.size(); ++i)
    if (!written[i]) return fail("a word of the layout was not written");

  FILE* o = fopen(argv[2], "wb");
  if (!o) return fail("cannot open the output file");
  fwrite(&total, 8, 1, o);
  fwrite(rows.data(), sizeof(smm_grib_row_t), rows.size(), o);
  fwrite(bms.data(), sizeof(smm_grib_bitmap_t), bms.size(), o);
  fwrite(out.data(), 4, out.size(), o);
  fclose(o);
  printf("OK %lld rows of %lld cells, %llu bytes\n", (long long)n_rows, (long long)n_dst, (unsigned long long)total);
  return 0;
}
