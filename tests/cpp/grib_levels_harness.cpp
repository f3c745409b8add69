// Stand-alone program for tests/test_grib_levels_harness.py: the chunk plan of the GRIB host entries in units
// (smm::plan_grib_chunks, smm_grib_plan.cpp) over random row widths, bitmaps and units, and the staging layout of every
// chunk it plans (smm::layout_grib_chunk), built with AddressSanitizer + UBSan.  A chunk is a run of whole outer indices;
// every property is recomputed here from the rows.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <utility>
#include <vector>

#include <sanitizer/asan_interface.h>

#include "../../include/smmregrid_amd.h"
#include "../../smmregrid_amd/csrc/smm_grib_codec.hpp"
#include "../../smmregrid_amd/csrc/smm_internal.h"

namespace {

constexpr uint64_t NO = SMM_GRIB_NO_BITMAP;

smm_grib_row_t row(uint64_t off, int nbits) { return smm_grib_row_t{off, 0.0, 1.0, 1.0, nbits, 0}; }
smm_grib_bitmap_t bm(uint64_t off, uint64_t n_values) { return smm_grib_bitmap_t{off, n_values}; }

struct Counts {
  int multi_unit = 0, single_over_target = 0, short_last = 0, no_bitmaps = 0;
  int layout_bad = 0, layouts_bm = 0, layouts_plain = 0, layouts_unit1 = 0;
};

// A buffer of exactly n bytes for every chunk in turn.  A fresh allocation per chunk costs AddressSanitizer a pass over
// the shadow of all its bytes (chunks reach 256 MiB and more, thousands of them); here one block is kept, grown when a
// chunk needs more, and poisoned behind byte n by hand: moving the boundary costs only the bytes it moves over.
struct ExactBuffer {
  char* base = nullptr;
  size_t cap = 0, open = 0;   // [0, open) is addressable, [open, cap) poisoned
  char* exactly(size_t n) {
    if (n > cap) {
      std::free(base);
      base = (char*)std::malloc(n);
      cap = open = n;
      return base;
    }
    const size_t from = std::min(n, open) & ~(size_t)7, to = std::min(cap, (std::max(n, open) + 7) & ~(size_t)7);
    ASAN_POISON_MEMORY_REGION(base + from, to - from);
    ASAN_UNPOISON_MEMORY_REGION(base + from, n - from);   // a last granule of n % 8 bytes stays closed behind them
    open = n;
    return base;
  }
  ~ExactBuffer() { std::free(base); }
} g_buffer;

// The layout of chunk c in a buffer of exactly c.x_bytes bytes (a write past it is a sanitizer error): the cursor ends at
// x_bytes, every piece starts on a multiple of 4, no data or bitmap range overlaps another or the tables, and the rank
// tables are numbered in row order and add up to rank_bytes.  bms empty: the call without bitmap records.
int layout_bad(const smm::GribChunk& c, const std::vector<smm_grib_row_t>& rows, const std::vector<smm_grib_bitmap_t>& bms,
               int64_t S) {
  int bad = 0;
  const uint64_t blocks = ((uint64_t)S + 31) / 32, segs = (blocks + smm_grib::kGribSegBlocks - 1) / smm_grib::kGribSegBlocks;
  char* hx = g_buffer.exactly(c.x_bytes);
  const smm::GribChunkLayout lay = smm::layout_grib_chunk(hx, c, rows.data(), bms.empty() ? nullptr : bms.data(), S);
  const smm_grib_row_t* table = (const smm_grib_row_t*)hx;
  const GribRowBitmap* rec = (const GribRowBitmap*)(hx + (size_t)c.nr * sizeof(smm_grib_row_t));
  const uint64_t tables_end = (uint64_t)c.nr * (40 + (bms.empty() ? 0 : 16));
  bad += lay.end != c.x_bytes;
  std::vector<std::pair<uint64_t, uint64_t>> ranges;   // (start, bytes) of every data and bitmap piece
  uint64_t n_tables = 0;
  for (int64_t r = 0; r < c.nr; ++r) {
    const smm_grib_row_t& in = rows[(size_t)(c.r0 + r)];
    const bool has = !bms.empty() && bms[(size_t)(c.r0 + r)].bitmap_off != NO;
    const uint64_t nv = has ? bms[(size_t)(c.r0 + r)].n_values : (uint64_t)S;
    bad += table[r].nbits != in.nbits || table[r].ref != in.ref || table[r].bscale != in.bscale || table[r].ddiv != in.ddiv;
    bad += table[r].byte_off % 4 != 0;
    ranges.push_back({table[r].byte_off, (nv * (uint64_t)in.nbits + 7) / 8});
    if (bms.empty()) continue;
    if (has) {
      bad += rec[r].bitmap_off % 4 != 0 || rec[r].table_off != n_tables * blocks;
      ranges.push_back({rec[r].bitmap_off, ((uint64_t)S + 7) / 8});
      ++n_tables;
    } else {
      bad += rec[r].bitmap_off != NO || rec[r].table_off != 0;
    }
  }
  bad += lay.n_tables != n_tables || n_tables * (blocks * 8 + segs * 4) != c.rank_bytes;
  std::sort(ranges.begin(), ranges.end());
  uint64_t floor = tables_end;
  for (const auto& g : ranges) {
    bad += g.first < floor;
    floor = std::max(floor, g.first + g.second);
  }
  bad += floor > c.x_bytes;
  return bad;
}

// bms empty: the call without bitmap records
int plan_ok(const smm::GribChunkPlan& p, const std::vector<smm_grib_row_t>& rows, const std::vector<smm_grib_bitmap_t>& bms,
            int64_t n_outer, int64_t unit, int64_t S, int64_t D, int64_t requested, Counts* n) {
  int bad = 0;
  int64_t next = 0, max_rows = 0;
  size_t max_x = 0, max_rank = 0;
  const size_t blocks = (size_t)((S + 31) / 32), segs = (blocks + smm_grib::kGribSegBlocks - 1) / smm_grib::kGribSegBlocks;
  for (const smm::GribChunk& c : p.chunks) {
    bad += c.r0 != next || c.nr < unit || c.nr % unit != 0 || c.r0 % unit != 0;   // in order, whole units, >= 1
    n->layout_bad += layout_bad(c, rows, bms, S);
    (bms.empty() ? n->layouts_plain : n->layouts_bm) += 1;
    n->layouts_unit1 += unit == 1;
    size_t x = 0, rank = 0;
    for (int64_t b = c.r0; b < c.r0 + c.nr; ++b) {
      const bool has = !bms.empty() && bms[(size_t)b].bitmap_off != NO;
      const uint64_t nv = has ? bms[(size_t)b].n_values : (uint64_t)S;
      x += 40 + (bms.empty() ? 0 : 16) + (size_t)(((nv * (uint64_t)rows[(size_t)b].nbits + 7) / 8 + 3) / 4 * 4);
      if (has) x += (size_t)((((uint64_t)S + 7) / 8 + 3) / 4 * 4), rank += blocks * 8 + segs * 4;
    }
    bad += x != c.x_bytes || rank != c.rank_bytes;
    const int64_t units = c.nr / unit;
    if (requested > 0) {
      bad += units != std::min<int64_t>(requested, n_outer - c.r0 / unit);
      n->short_last += units < requested;
    } else if (units > 1) {
      bad += x + rank + (size_t)c.nr * (size_t)D * 8 > p.target;
    } else {
      n->single_over_target += x + rank + (size_t)c.nr * (size_t)D * 8 > p.target;
    }
    n->multi_unit += units > 1;
    max_x = std::max(max_x, x);
    max_rank = std::max(max_rank, rank);
    max_rows = std::max(max_rows, c.nr);
    next += c.nr;
  }
  bad += next != n_outer * unit || max_x != p.max_x || max_rows != p.max_rows || max_rank != p.max_rank;
  bad += requested > 0 ? p.target != 0 : p.target == 0;
  return bad;
}

int plan_bad(Counts* n) {
  int bad = 0;
  const size_t MiB = (size_t)1 << 20;
  // 16 ocean levels x 32 steps of r1440x721 -> r360x180, 16 bits, 70 % of the cells present: the bench shape
  {
    const int64_t S = 1440 * 721, D = 360 * 180, unit = 16, n_outer = 32;
    std::vector<smm_grib_row_t> rows((size_t)(unit * n_outer), row(0, 16));
    std::vector<smm_grib_bitmap_t> bms(rows.size(), bm(0, (uint64_t)(0.7 * S)));
    smm::GribChunkPlan p = smm::plan_grib_chunks(rows.data(), bms.data(), n_outer, unit, S, D, 0, (size_t)200 << 30);
    bad += plan_ok(p, rows, bms, n_outer, unit, S, D, 0, n) || p.target > 256 * MiB || p.target < 32 * MiB || p.chunks.size() < 8;
    // the same without records: 16 B less per row, no rank bytes
    smm::GribChunkPlan q = smm::plan_grib_chunks(rows.data(), nullptr, n_outer, unit, S, D, 0, (size_t)200 << 30);
    bad += plan_ok(q, rows, {}, n_outer, unit, S, D, 0, n) || q.max_rank != 0;
    n->no_bitmaps += q.max_rank == 0 && !q.chunks.empty();
    // chunk_outer is honoured, the last chunk is short
    p = smm::plan_grib_chunks(rows.data(), bms.data(), n_outer, unit, S, D, 5, 0);
    bad += plan_ok(p, rows, bms, n_outer, unit, S, D, 5, n) || p.chunks.size() != 7 || p.chunks.back().nr != 2 * unit;
    // no outer index, no unit: no chunks
    bad += !smm::plan_grib_chunks(rows.data(), bms.data(), 0, unit, S, D, 0, 0).chunks.empty();
    bad += !smm::plan_grib_chunks(rows.data(), bms.data(), n_outer, 0, S, D, 0, 0).chunks.empty();
    bad += !smm::plan_grib_chunks(rows.data(), bms.data(), 0, 0, S, D, 3, 0).chunks.empty();
  }
  // a unit that alone exceeds the bound still gets a chunk; free memory bounds the target
  {
    const int64_t S = 100000000, unit = 2, n_outer = 3;
    std::vector<smm_grib_row_t> fat((size_t)(unit * n_outer), row(0, 32));
    std::vector<smm_grib_bitmap_t> fatbm(fat.size(), bm(0, 90000000));
    smm::GribChunkPlan p = smm::plan_grib_chunks(fat.data(), fatbm.data(), n_outer, unit, S, 5, 0, 64 * MiB);
    bad += plan_ok(p, fat, fatbm, n_outer, unit, S, 5, 0, n) || p.chunks.size() != 3 || p.target != 8 * MiB ||
           p.chunks[0].x_bytes <= p.target;
  }
  // a seeded sweep over widths, bitmaps, units, requests and free memory
  std::mt19937_64 rng(17);
  for (int it = 0; it < 400; ++it) {
    const int64_t n_outer = 1 + (int64_t)(rng() % 40), unit = 1 + (int64_t)(rng() % 24);
    const int64_t s = 1 + (int64_t)(rng() % 3000000), d = 1 + (int64_t)(rng() % 300000);
    const int64_t n_rows = n_outer * unit;
    std::vector<smm_grib_row_t> rr((size_t)n_rows);
    std::vector<smm_grib_bitmap_t> bb((size_t)n_rows);
    for (int64_t i = 0; i < n_rows; ++i) {
      rr[(size_t)i] = row(0, (int)(rng() % 33));
      bb[(size_t)i] = (rng() % 3) ? bm(rng() % 1000, rng() % (uint64_t)(s + 1)) : bm(NO, (uint64_t)s);
    }
    if (it % 7 == 0) bb.clear();
    const int64_t req = (it % 3 == 0) ? 1 + (int64_t)(rng() % 9) : 0;
    const size_t free_b = (it % 5 == 0) ? (size_t)(rng() % (8ull << 30)) : 0;
    const smm::GribChunkPlan p =
        smm::plan_grib_chunks(rr.data(), bb.empty() ? nullptr : bb.data(), n_outer, unit, s, d, req, free_b);
    bad += plan_ok(p, rr, bb, n_outer, unit, s, d, req, n);
  }
  return bad;
}

}  // namespace

int main() {
  Counts n;
  const int pb = plan_bad(&n);
  std::printf("PLANBAD %d %d %d %d %d\n", pb, n.multi_unit, n.single_over_target, n.short_last, n.no_bitmaps);
  std::printf("LAYOUTBAD %d %d %d %d\n", n.layout_bad, n.layouts_bm, n.layouts_plain, n.layouts_unit1);
  return 0;
}
