// Host side of the GRIB entries that needs no device: the refusals of a row table and the chunk plan of
// smm_apply_host_grib, the same with bitmaps for the _bm entries, and the unit plan of smm_group_apply_host_grib
// (declared in smm_internal.h).  Plain C++: tests/cpp/grib_harness.cpp, grib_bitmap_harness.cpp and
// grib_levels_harness.cpp link this file.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <string>

#include "../../include/smmregrid_amd.h"
#include "smm_grib_codec.hpp"
#include "smm_internal.h"

namespace smm {

bool check_grib_rules(const smm_grib_row_t* rows, int64_t n_batch, std::string& err) {
  for (int64_t b = 0; b < n_batch; ++b) {
    const smm_grib_row_t& r = rows[b];
    const std::string at = "rows[" + std::to_string(b) + "]";
    if (r.nbits < 0 || r.nbits > 32) return err = at + ".nbits must be within 0..32", false;
    if (r.reserved != 0) return err = at + ".reserved must be 0", false;
    int e = 0;
    if (!std::isnormal(r.bscale) || r.bscale <= 0.0 || std::frexp(r.bscale, &e) != 0.5)
      return err = at + ".bscale must be a power of two in the normal range (2^E)", false;
    if (!std::isfinite(r.ddiv) || !(r.ddiv > 0.0)) return err = at + ".ddiv must be finite and > 0 (10^D)", false;
    if (!std::isfinite(r.ref)) return err = at + ".ref must be finite", false;
  }
  return true;
}

bool check_grib_ranges(const smm_grib_row_t* rows, int64_t n_batch, int64_t n_src, int64_t x_bytes, std::string& err) {
  for (int64_t b = 0; b < n_batch; ++b) {
    const uint64_t need = smm_grib::row_bytes((uint64_t)n_src, rows[b].nbits);   // n_src < 2^31, nbits <= 32: no overflow
    if (rows[b].byte_off > (uint64_t)x_bytes || need > (uint64_t)x_bytes - rows[b].byte_off)
      return err = "rows[" + std::to_string(b) + "]: bytes [" + std::to_string(rows[b].byte_off) + ", " +
                   std::to_string(rows[b].byte_off) + " + " + std::to_string(need) + ") leave the buffer of " +
                   std::to_string(x_bytes) + " bytes", false;
  }
  return true;
}

GribChunkPlan plan_grib_chunks(const smm_grib_row_t* rows, int64_t n_batch, int64_t n_src, int64_t D,
                               int64_t requested_rows, size_t free_bytes) {
  constexpr size_t kTarget = (size_t)256 << 20, kMinChunk = (size_t)32 << 20;
  constexpr int64_t kMinChunks = 8;
  GribChunkPlan plan;
  auto row_cost_x = [&](int64_t b) {
    return sizeof(smm_grib_row_t) + (size_t)smm_grib::align4(smm_grib::row_bytes((uint64_t)n_src, rows[b].nbits));
  };
  const size_t y_row = (size_t)std::max<int64_t>(D, 0) * 8;
  if (requested_rows <= 0) {
    size_t total = 0;
    for (int64_t b = 0; b < n_batch; ++b) total += row_cost_x(b) + y_row;
    plan.target = std::min(kTarget, std::max(kMinChunk, total / (size_t)kMinChunks));
    if (free_bytes > 0) plan.target = std::min(plan.target, std::max<size_t>(free_bytes / 8, 1));
  }
  for (int64_t b = 0; b < n_batch;) {
    GribChunk c{b, 0, 0};
    size_t bytes = 0;
    while (b < n_batch) {
      const size_t x = row_cost_x(b);
      if (requested_rows > 0 ? c.nr >= requested_rows : (c.nr > 0 && bytes + x + y_row > plan.target)) break;
      bytes += x + y_row;
      c.x_bytes += x;
      ++c.nr;
      ++b;
    }
    plan.max_x = std::max(plan.max_x, c.x_bytes);
    plan.max_rows = std::max(plan.max_rows, c.nr);
    plan.chunks.push_back(c);
  }
  return plan;
}

bool check_grib_bitmaps(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_batch, int64_t n_src,
                        int64_t x_bytes, std::string& err) {
  auto outside = [&](uint64_t off, uint64_t need) { return off > (uint64_t)x_bytes || need > (uint64_t)x_bytes - off; };
  for (int64_t b = 0; b < n_batch; ++b) {
    const smm_grib_bitmap_t& m = bitmaps[b];
    const std::string at = "rows[" + std::to_string(b) + "]";
    if (m.n_values > (uint64_t)n_src)
      return err = at + ": n_values " + std::to_string(m.n_values) + " exceeds the grid's " + std::to_string(n_src) + " cells",
             false;
    const bool has = m.bitmap_off != SMM_GRIB_NO_BITMAP;
    if (has && outside(m.bitmap_off, smm_grib::bitmap_bytes((uint64_t)n_src)))
      return err = at + ": bitmap bytes [" + std::to_string(m.bitmap_off) + ", " + std::to_string(m.bitmap_off) + " + " +
                   std::to_string(smm_grib::bitmap_bytes((uint64_t)n_src)) + ") leave the buffer of " +
                   std::to_string(x_bytes) + " bytes", false;
    const uint64_t need = smm_grib::row_bytes(has ? m.n_values : (uint64_t)n_src, rows[b].nbits);
    if (outside(rows[b].byte_off, need))
      return err = at + ": bytes [" + std::to_string(rows[b].byte_off) + ", " + std::to_string(rows[b].byte_off) + " + " +
                   std::to_string(need) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes", false;
  }
  return true;
}

size_t grib_bm_row_staged(const smm_grib_row_t& row, const smm_grib_bitmap_t& bm, int64_t n_src) {
  const bool has = bm.bitmap_off != SMM_GRIB_NO_BITMAP;
  return sizeof(smm_grib_row_t) + sizeof(smm_grib_bitmap_t) +
         (size_t)smm_grib::align4(smm_grib::row_bytes(has ? bm.n_values : (uint64_t)n_src, row.nbits)) +
         (has ? (size_t)smm_grib::align4(smm_grib::bitmap_bytes((uint64_t)n_src)) : 0);
}

size_t grib_bm_row_rank(const smm_grib_bitmap_t& bm, int64_t n_src) {
  if (bm.bitmap_off == SMM_GRIB_NO_BITMAP) return 0;
  return (size_t)smm_grib::bitmap_blocks((uint64_t)n_src) * sizeof(smm_grib::GribRankEntry) +
         (size_t)smm_grib::bitmap_segments((uint64_t)n_src) * sizeof(uint32_t);
}

GribChunkPlan plan_grib_chunks_bm(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_batch,
                                  int64_t n_src, int64_t D, int64_t requested_rows, size_t free_bytes) {
  constexpr size_t kTarget = (size_t)256 << 20, kMinChunk = (size_t)32 << 20;   // plan_grib_chunks' bounds
  constexpr int64_t kMinChunks = 8;
  GribChunkPlan plan;
  const size_t y_row = (size_t)std::max<int64_t>(D, 0) * 8;
  if (requested_rows <= 0) {
    size_t total = 0;
    for (int64_t b = 0; b < n_batch; ++b)
      total += grib_bm_row_staged(rows[b], bitmaps[b], n_src) + grib_bm_row_rank(bitmaps[b], n_src) + y_row;
    plan.target = std::min(kTarget, std::max(kMinChunk, total / (size_t)kMinChunks));
    if (free_bytes > 0) plan.target = std::min(plan.target, std::max<size_t>(free_bytes / 8, 1));
  }
  for (int64_t b = 0; b < n_batch;) {
    GribChunk c{b, 0, 0};
    size_t bytes = 0;
    while (b < n_batch) {
      const size_t x = grib_bm_row_staged(rows[b], bitmaps[b], n_src), r = grib_bm_row_rank(bitmaps[b], n_src);
      if (requested_rows > 0 ? c.nr >= requested_rows : (c.nr > 0 && bytes + x + r + y_row > plan.target)) break;
      bytes += x + r + y_row;
      c.x_bytes += x;
      c.rank_bytes += r;
      ++c.nr;
      ++b;
    }
    plan.max_x = std::max(plan.max_x, c.x_bytes);
    plan.max_rank = std::max(plan.max_rank, c.rank_bytes);
    plan.max_rows = std::max(plan.max_rows, c.nr);
    plan.chunks.push_back(c);
  }
  return plan;
}

GribChunkPlan plan_grib_chunks_units(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_outer,
                                     int64_t unit, int64_t n_src, int64_t D, int64_t requested_units, size_t free_bytes) {
  constexpr size_t kTarget = (size_t)256 << 20, kMinChunk = (size_t)32 << 20;   // plan_grib_chunks' bounds
  constexpr int64_t kMinChunks = 8;
  GribChunkPlan plan;
  if (n_outer <= 0 || unit <= 0) return plan;
  const size_t y_row = (size_t)std::max<int64_t>(D, 0) * 8;
  // staged and rank bytes of outer index o: its `unit` consecutive records
  auto unit_cost = [&](int64_t o, size_t& x, size_t& r) {
    x = r = 0;
    for (int64_t b = o * unit; b < (o + 1) * unit; ++b) {
      if (bitmaps) {
        x += grib_bm_row_staged(rows[b], bitmaps[b], n_src);
        r += grib_bm_row_rank(bitmaps[b], n_src);
      } else {
        x += sizeof(smm_grib_row_t) + (size_t)smm_grib::align4(smm_grib::row_bytes((uint64_t)n_src, rows[b].nbits));
      }
    }
  };
  if (requested_units <= 0) {
    size_t total = 0, x = 0, r = 0;
    for (int64_t o = 0; o < n_outer; ++o) {
      unit_cost(o, x, r);
      total += x + r + (size_t)unit * y_row;
    }
    plan.target = std::min(kTarget, std::max(kMinChunk, total / (size_t)kMinChunks));
    if (free_bytes > 0) plan.target = std::min(plan.target, std::max<size_t>(free_bytes / 8, 1));
  }
  for (int64_t o = 0; o < n_outer;) {
    GribChunk c{o * unit, 0, 0};
    size_t bytes = 0;
    int64_t units = 0;
    while (o < n_outer) {
      size_t x = 0, r = 0;
      unit_cost(o, x, r);
      const size_t all = x + r + (size_t)unit * y_row;
      if (requested_units > 0 ? units >= requested_units : (units > 0 && bytes + all > plan.target)) break;
      bytes += all;
      c.x_bytes += x;
      c.rank_bytes += r;
      c.nr += unit;
      ++units;
      ++o;
    }
    plan.max_x = std::max(plan.max_x, c.x_bytes);
    plan.max_rank = std::max(plan.max_rank, c.rank_bytes);
    plan.max_rows = std::max(plan.max_rows, c.nr);
    plan.chunks.push_back(c);
  }
  return plan;
}

}  // namespace smm
