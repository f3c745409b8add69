// Stand-alone check of the bitmap code of smm_apply_grib_bm that needs no device, built with
// -fsanitize=address,undefined by tests/test_grib_bitmap_harness.py: bitmap_block / bitmap_present / bitmap_index of
// smm_grib_codec.hpp -- the very functions the table build and the gather run -- against a bit-by-bit loop, and
// check_grib_ranges / plan_grib_chunks of smm_grib_plan.cpp with bitmap records.  Prints "<NAME>BAD <count> ..." lines; 0 is a pass.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <random>
#include <string>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "../../smmregrid_amd/csrc/smm_grib_codec.hpp"
#include "../../smmregrid_amd/csrc/smm_internal.h"

namespace {

using smm_grib::GribRankEntry;

inline unsigned bit_at(const uint8_t* b, uint64_t i) { return (b[i >> 3] >> (7 - (i & 7))) & 1u; }

// The rank table of the bitmap at byte `off` of buf, as the build kernels fill it: the block function, a running sum.
std::vector<GribRankEntry> build_table(const uint8_t* buf, uint64_t alloc, uint64_t off, uint32_t n_src) {
  const uint32_t* words = (const uint32_t*)buf + (off >> 2);   // the kernels' addressing: words from off & ~3
  const uint32_t last_word = (uint32_t)(alloc / 4 - 1 - (off >> 2));
  std::vector<GribRankEntry> t;
  uint32_t rank = 0;
  for (uint32_t k = 0; k < smm_grib::bitmap_blocks(n_src); ++k) {
    const uint32_t bits = smm_grib::bitmap_block(words, 8u * (uint32_t)(off & 3), k, n_src, last_word);
    t.push_back(GribRankEntry{bits, rank});
    rank += smm_grib::popcount32(bits);
  }
  return t;
}

// pattern: 0 random at a random density, 1 all missing, 2 all present, 3 whole blocks all zero / all one in turn,
// 4 only the first and the last cell
int codec_bad(long* checked, long* pad_cases) {
  std::mt19937_64 rng(20261019);
  int bad = 0;
  for (uint32_t n_src : {1u, 31u, 32u, 33u, 63u, 64u, 65u, 96u, 300u, 777u})
    for (uint64_t off = 0; off < 8; ++off)   // byte residues 0..3, with and without a word in front
      for (int pattern = 0; pattern < 5; ++pattern) {
        const uint64_t x_bytes = off + smm_grib::bitmap_bytes(n_src);
        const uint64_t alloc = smm_grib::align4(x_bytes);   // the heap block holds exactly this: a load past it is a report
        uint8_t* buf = (uint8_t*)std::malloc(alloc);
        if (!buf) return -1;
        for (uint64_t i = 0; i < alloc; ++i) buf[i] = (uint8_t)rng();
        const double density = (double)(rng() % 1000) / 999.0;
        std::vector<uint8_t> want(n_src);
        for (uint32_t c = 0; c < n_src; ++c) {
          unsigned b = 0;
          if (pattern == 0) b = (double)(rng() % 1000) / 1000.0 < density;
          if (pattern == 2) b = 1;
          if (pattern == 3) b = (c / 32) % 2;
          if (pattern == 4) b = c == 0 || c == n_src - 1;
          want[c] = (uint8_t)b;
          uint8_t& byte = buf[off + (c >> 3)];
          byte = (uint8_t)((byte & ~(0x80u >> (c & 7))) | (b ? (0x80u >> (c & 7)) : 0u));
        }
        // two fillings of everything that is not the bitmap's first n_src bits -- the last byte's pad, the block's
        // tail, the bytes in front: all ones and all zeros must give the same table
        std::vector<GribRankEntry> tables[2];
        for (int fill = 0; fill < 2; ++fill) {
          for (uint64_t i = 8 * off + n_src; i < 8 * alloc; ++i) {
            uint8_t& byte = buf[i >> 3];
            byte = (uint8_t)(fill ? byte | (0x80u >> (i & 7)) : byte & ~(0x80u >> (i & 7)));
          }
          std::memset(buf, fill ? 0xff : 0x00, (size_t)off);
          tables[fill] = build_table(buf, alloc, off, n_src);
        }
        *pad_cases += (8 * alloc > 8 * off + n_src);
        bad += tables[0].size() != tables[1].size() ||
               std::memcmp(tables[0].data(), tables[1].data(), tables[0].size() * sizeof(GribRankEntry)) != 0;
        const std::vector<GribRankEntry>& t = tables[0];
        bad += t.size() != smm_grib::bitmap_blocks(n_src);
        uint32_t rank = 0;
        for (uint32_t c = 0; c < n_src; ++c) {
          const GribRankEntry e = t[c >> 5];
          bad += bit_at(buf + off, c) != want[c];                        // the harness's own bitmap writer
          bad += smm_grib::bitmap_present(e, c) != (want[c] != 0);
          bad += smm_grib::bitmap_index(e, c) != rank;                   // set bits before c, by the loop
          if ((c & 31) == 0) bad += e.rank_before != rank;
          rank += want[c];
          ++*checked;
        }
        // bits of cells >= n_src in the last block are cleared
        if (n_src % 32) bad += (t.back().bits & (0xffffffffu >> (n_src % 32))) != 0;
        std::free(buf);
      }
  return bad;
}

smm_grib_row_t row(uint64_t off, int nbits) { return smm_grib_row_t{off, 0.0, 1.0, 1.0, nbits, 0}; }
smm_grib_bitmap_t bm(uint64_t off, uint64_t n) { return smm_grib_bitmap_t{off, n}; }
const uint64_t NO = SMM_GRIB_NO_BITMAP;

int checks_bad() {
  int bad = 0;
  std::string err;
  // 20 cells: a bitmap takes 3 bytes.  Row 0: 12 values of 16 bits = 24 B at 0, bitmap at 24..27; row 1 without a
  // bitmap: 20 values of 12 bits = 30 B at 27; row 2: no value at all, data "at" the end, bitmap shared with row 0
  std::vector<smm_grib_row_t> r = {row(0, 16), row(27, 12), row(57, 16)};
  std::vector<smm_grib_bitmap_t> m = {bm(24, 12), bm(NO, 20), bm(24, 0)};
  bad += !smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err);
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 56, err);                 // row 1 ends at 57
  m[0].n_values = 21;                                                                    // more values than cells
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err) || err.find("n_values") == std::string::npos ||
         err.find("rows[0]") == std::string::npos;
  m[0].n_values = 12;
  m[1].n_values = 21;                                                                    // ... in a row without a bitmap too
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err) || err.find("rows[1]") == std::string::npos;
  m[1].n_values = 20;
  m[2].bitmap_off = 55;                                                                  // 55 + 3 = 58 > 57
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err) || err.find("bitmap") == std::string::npos ||
         err.find("leave the buffer") == std::string::npos;
  m[2].bitmap_off = 54;                                                                  // ends exactly at x_bytes
  bad += !smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err);
  m[2].bitmap_off = ~0ull - 1;                                                           // no wrap-around
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err);
  m[2].bitmap_off = 24;
  m[0].n_values = 13;                                                                    // 26 B of data: still inside
  bad += !smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err);
  r[0].byte_off = 32;                                                                    // 32 + 26 = 58: the n_values-based range
  bad += smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err) || err.find("rows[0]") == std::string::npos ||
         err.find("leave the buffer") == std::string::npos;
  m[0].n_values = 12;                                                                    // 32 + 24 = 56: inside again, where
  bad += !smm::check_grib_ranges(r.data(), m.data(), 3, 20, 57, err);                // 20 values (40 B) would not be
  bad += smm::check_grib_ranges(r.data(), nullptr, 1, 20, 57, err);
  return bad;
}

int plan_ok(const smm::GribChunkPlan& p, const std::vector<smm_grib_row_t>& rows, const std::vector<smm_grib_bitmap_t>& bms,
            int64_t S, int64_t D, int64_t requested) {
  int bad = 0;
  int64_t next = 0, max_rows = 0;
  size_t max_x = 0, max_rank = 0;
  const size_t blocks = (size_t)((S + 31) / 32), segs = (blocks + smm_grib::kGribSegBlocks - 1) / smm_grib::kGribSegBlocks;
  for (const smm::GribChunk& c : p.chunks) {
    bad += c.r0 != next || c.nr < 1;
    size_t x = 0, rank = 0;
    for (int64_t b = c.r0; b < c.r0 + c.nr; ++b) {
      const bool has = bms[(size_t)b].bitmap_off != NO;
      const uint64_t n = has ? bms[(size_t)b].n_values : (uint64_t)S;
      x += 40 + 16 + (size_t)(((n * (uint64_t)rows[(size_t)b].nbits + 7) / 8 + 3) / 4 * 4);
      if (has) x += (size_t)((((uint64_t)S + 7) / 8 + 3) / 4 * 4), rank += blocks * 8 + segs * 4;
    }
    bad += x != c.x_bytes || rank != c.rank_bytes;
    if (requested > 0) bad += c.nr != std::min<int64_t>(requested, (int64_t)rows.size() - c.r0);
    else if (c.nr > 1) bad += x + rank + (size_t)c.nr * D * 8 > p.target;
    max_x = std::max(max_x, x);
    max_rank = std::max(max_rank, rank);
    max_rows = std::max(max_rows, c.nr);
    next += c.nr;
  }
  bad += next != (int64_t)rows.size() || max_x != p.max_x || max_rows != p.max_rows || max_rank != p.max_rank;
  return bad;
}

int plan_bad(int* multi_row_plans, int* single_over_target, int* rank_counted) {
  int bad = 0;
  const size_t MiB = (size_t)1 << 20;
  // config-4 geometry, 30 % missing: 128 rows of 6.6 M cells at 16 bits, every one with a bitmap
  const int64_t S = 6599680, D = 786432;
  std::vector<smm_grib_row_t> rows(128, row(0, 16));
  std::vector<smm_grib_bitmap_t> bms(128, bm(0, (uint64_t)(0.7 * S)));
  smm::GribChunkPlan p = smm::plan_grib_chunks(rows.data(), bms.data(), 128, 1, S, D, 0, (size_t)200 << 30);
  bad += plan_ok(p, rows, bms, S, D, 0) || p.target > 256 * MiB || p.target < 32 * MiB || p.chunks.size() < 8;
  *multi_row_plans += p.max_rows > 1;
  // the table bytes count: the same rows without bitmaps (and so with all their values) make another plan
  std::vector<smm_grib_bitmap_t> none(128, bm(NO, (uint64_t)S));
  smm::GribChunkPlan q = smm::plan_grib_chunks(rows.data(), none.data(), 128, 1, S, D, 0, (size_t)200 << 30);
  bad += plan_ok(q, rows, none, S, D, 0) || q.max_rank != 0;
  *rank_counted += p.max_rank > 0 && p.chunks[0].rank_bytes == (size_t)p.chunks[0].nr * (206240 * 8 + 202 * 4);
  // without bitmaps the plan is that of the call without records, with 16 B more per row
  smm::GribChunkPlan o = smm::plan_grib_chunks(rows.data(), nullptr, 128, 1, S, D, 0, (size_t)200 << 30);
  bad += o.chunks.size() != q.chunks.size() || q.chunks[0].x_bytes != o.chunks[0].x_bytes + 16 * (size_t)o.chunks[0].nr;
  // mixed: every other row bitmapped, widths mixed, 0-bit rows
  for (size_t b = 0; b < rows.size(); ++b) {
    rows[b].nbits = (b % 4 == 0) ? 0 : (b % 4 == 1 ? 12 : (b % 4 == 2 ? 24 : 7));
    if (b % 2) bms[b] = bm(NO, (uint64_t)S);
  }
  p = smm::plan_grib_chunks(rows.data(), bms.data(), 128, 1, S, 1000, 0, 0);
  bad += plan_ok(p, rows, bms, S, 1000, 0);
  // a fat row gets a chunk of one; free memory bounds the target
  std::vector<smm_grib_row_t> fat(3, row(0, 32));
  std::vector<smm_grib_bitmap_t> fatbm(3, bm(0, 90000000));
  p = smm::plan_grib_chunks(fat.data(), fatbm.data(), 3, 1, 100000000, 5, 0, 64 * MiB);
  bad += plan_ok(p, fat, fatbm, 100000000, 5, 0) || p.chunks.size() != 3 || p.target != 8 * MiB;
  *single_over_target += p.chunks[0].x_bytes > p.target;
  // chunk_rows overrides
  p = smm::plan_grib_chunks(rows.data(), bms.data(), 128, 1, S, D, 5, 0);
  bad += plan_ok(p, rows, bms, S, D, 5) || p.chunks.size() != 26 || p.chunks.back().nr != 3 || p.target != 0;
  p = smm::plan_grib_chunks(rows.data(), bms.data(), 0, 1, S, D, 0, 0);
  bad += !p.chunks.empty();
  // a seeded sweep
  std::mt19937_64 rng(11);
  for (int it = 0; it < 300; ++it) {
    const int64_t n = 1 + (int64_t)(rng() % 200), s = 1 + (int64_t)(rng() % 3000000), d = 1 + (int64_t)(rng() % 500000);
    std::vector<smm_grib_row_t> rr((size_t)n);
    std::vector<smm_grib_bitmap_t> bb((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
      rr[(size_t)i] = row(0, (int)(rng() % 33));
      bb[(size_t)i] = (rng() % 3) ? bm(rng() % 1000, rng() % (uint64_t)(s + 1)) : bm(NO, (uint64_t)s);
    }
    const int64_t req = (it % 3 == 0) ? 1 + (int64_t)(rng() % 9) : 0;
    const size_t free_b = (it % 5 == 0) ? (size_t)(rng() % (8ull << 30)) : 0;
    p = smm::plan_grib_chunks(rr.data(), bb.data(), n, 1, s, d, req, free_b);
    bad += plan_ok(p, rr, bb, s, d, req);
    *multi_row_plans += p.max_rows > 1;
  }
  return bad;
}

}  // namespace

int main() {
  long checked = 0, pads = 0;
  int multi = 0, over = 0, rank_counted = 0;
  const int cb = codec_bad(&checked, &pads);
  std::printf("CODECBAD %d %ld %ld\n", cb, checked, pads);
  std::printf("CHECKBAD %d\n", checks_bad());
  const int pb = plan_bad(&multi, &over, &rank_counted);
  std::printf("PLANBAD %d %d %d %d\n", pb, multi, over, rank_counted);
  std::printf("SEGBLOCKS %d\n", smm_grib::kGribSegBlocks);
  return 0;
}
