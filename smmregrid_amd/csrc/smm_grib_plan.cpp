// Host side of the GRIB entries that needs no device: the refusals of a row table and of its bitmap records, the chunk
// plan of the host entries and the layout of a staged chunk (declared in smm_internal.h).  Plain C++:
// tests/cpp/grib_harness.cpp, grib_bitmap_harness.cpp, grib_levels_harness.cpp, grib_pack_harness.cpp and
// grib_levels_pack_harness.cpp link this file.
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

bool check_grib_ranges(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_batch, int64_t n_src,
                       int64_t x_bytes, std::string& err) {
  auto outside = [&](uint64_t off, uint64_t need) { return off > (uint64_t)x_bytes || need > (uint64_t)x_bytes - off; };
  for (int64_t b = 0; b < n_batch; ++b) {
    const std::string at = "rows[" + std::to_string(b) + "]";
    if (bitmaps && bitmaps[b].n_values > (uint64_t)n_src)
      return err = at + ": n_values " + std::to_string(bitmaps[b].n_values) + " exceeds the grid's " + std::to_string(n_src) +
                   " cells", false;
    const GribRowCost c = grib_row_cost(rows[b], bitmaps ? &bitmaps[b] : nullptr, n_src);   // n_src < 2^31, nbits <= 32: no overflow
    if (c.has_bitmap && outside(bitmaps[b].bitmap_off, c.bitmap_bytes))
      return err = at + ": bitmap bytes [" + std::to_string(bitmaps[b].bitmap_off) + ", " + std::to_string(bitmaps[b].bitmap_off) +
                   " + " + std::to_string(c.bitmap_bytes) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes", false;
    if (outside(rows[b].byte_off, c.data_bytes))
      return err = at + ": bytes [" + std::to_string(rows[b].byte_off) + ", " + std::to_string(rows[b].byte_off) + " + " +
                   std::to_string(c.data_bytes) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes", false;
  }
  return true;
}

GribRowCost grib_row_cost(const smm_grib_row_t& row, const smm_grib_bitmap_t* bm, int64_t n_src) {
  GribRowCost c;
  c.has_bitmap = bm && bm->bitmap_off != SMM_GRIB_NO_BITMAP;
  c.records = sizeof(smm_grib_row_t) + (bm ? sizeof(GribRowBitmap) : 0);
  c.data_bytes = (size_t)smm_grib::row_bytes(c.has_bitmap ? bm->n_values : (uint64_t)n_src, row.nbits);
  c.staged_data = (size_t)smm_grib::align4(c.data_bytes);
  if (c.has_bitmap) {
    c.bitmap_bytes = (size_t)smm_grib::bitmap_bytes((uint64_t)n_src);
    c.staged_bitmap = (size_t)smm_grib::align4(c.bitmap_bytes);
    c.rank = (size_t)smm_grib::bitmap_blocks((uint64_t)n_src) * sizeof(smm_grib::GribRankEntry) +
             (size_t)smm_grib::bitmap_segments((uint64_t)n_src) * sizeof(uint32_t);
  }
  return c;
}

GribChunkPlan plan_grib_chunks(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_outer, int64_t unit,
                               int64_t n_src, int64_t D, int64_t requested_units, size_t free_bytes,
                               const size_t* out_row_bytes) {
  constexpr size_t kTarget = (size_t)256 << 20, kMinChunk = (size_t)32 << 20;
  constexpr int64_t kMinChunks = 8;
  GribChunkPlan plan;
  if (n_outer <= 0 || unit <= 0) return plan;
  const size_t y_row = (size_t)std::max<int64_t>(D, 0) * 8;
  // staged and rank bytes of outer index o: its `unit` consecutive records
  // ... and, for a packed result, what its rows add on the device (out_row_bytes)
  auto unit_cost = [&](int64_t o, size_t& x, size_t& r, size_t& e) {
    x = r = e = 0;
    for (int64_t b = o * unit; b < (o + 1) * unit; ++b) {
      const GribRowCost c = grib_row_cost(rows[b], bitmaps ? &bitmaps[b] : nullptr, n_src);
      x += c.staged();
      r += c.rank;
      if (out_row_bytes) e += out_row_bytes[b];
    }
  };
  if (requested_units <= 0) {
    size_t total = 0, x = 0, r = 0, e = 0;
    for (int64_t o = 0; o < n_outer; ++o) {
      unit_cost(o, x, r, e);
      total += x + r + e + (size_t)unit * y_row;
    }
    plan.target = std::min(kTarget, std::max(kMinChunk, total / (size_t)kMinChunks));
    if (free_bytes > 0) plan.target = std::min(plan.target, std::max<size_t>(free_bytes / 8, 1));
  }
  for (int64_t o = 0; o < n_outer;) {
    GribChunk c{o * unit, 0, 0};
    size_t bytes = 0;
    int64_t units = 0;
    while (o < n_outer) {
      size_t x = 0, r = 0, e = 0;
      unit_cost(o, x, r, e);
      const size_t all = x + r + e + (size_t)unit * y_row;
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

GribChunkLayout layout_grib_chunk(char* hx, const GribChunk& ch, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                                  int64_t n_src) {
  smm_grib_row_t* table = (smm_grib_row_t*)hx;
  GribRowBitmap* bm = (GribRowBitmap*)(hx + (size_t)ch.nr * sizeof(smm_grib_row_t));
  const uint64_t n_blocks = smm_grib::bitmap_blocks((uint64_t)n_src);
  GribChunkLayout out;
  for (int64_t r = 0; r < ch.nr; ++r)   // the records come first ...
    out.end += grib_row_cost(rows[ch.r0 + r], bitmaps ? &bitmaps[ch.r0 + r] : nullptr, n_src).records;
  for (int64_t r = 0; r < ch.nr; ++r) {   // ... then each row's data and, behind it, its bitmap
    const GribRowCost c = grib_row_cost(rows[ch.r0 + r], bitmaps ? &bitmaps[ch.r0 + r] : nullptr, n_src);
    table[r] = rows[ch.r0 + r];
    table[r].byte_off = out.end;
    out.end += c.staged_data;
    if (!bitmaps) continue;
    bm[r] = GribRowBitmap{c.has_bitmap ? (uint64_t)out.end : SMM_GRIB_NO_BITMAP, c.has_bitmap ? out.n_tables * n_blocks : 0};
    out.end += c.staged_bitmap;
    out.n_tables += c.has_bitmap;
  }
  return out;
}

bool check_grib_encode(const smm_grib_encode_t* enc, int64_t n_batch, int64_t n_dst, std::string& err) {
  if (n_dst < 0 || n_dst >= ((int64_t)1 << 31)) return err = "n_dst must be within [0, 2^31)", false;
  for (int64_t b = 0; b < n_batch; ++b) {
    const std::string at = "enc[" + std::to_string(b) + "]";
    if (enc[b].nbits < 1 || enc[b].nbits > 32) return err = at + ".nbits must be within 1..32", false;
    if (!std::isfinite(enc[b].ddiv) || !(enc[b].ddiv > 0.0)) return err = at + ".ddiv must be finite and > 0 (10^D)", false;
    if (enc[b].reserved != 0) return err = at + ".reserved must be 0", false;
  }
  return true;
}

uint64_t grib_out_layout(int64_t n_dst, const smm_grib_encode_t* enc, int64_t n_batch, uint64_t* byte_off) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (byte_off) byte_off[b] = at;
    at += smm_grib::pack_slot_bytes((uint64_t)n_dst, enc[b].nbits);
  }
  return at;
}

bool check_grib_aec(const smm_grib_aec_t* recs, int64_t n_batch, int64_t x_bytes, std::string& err) {
  constexpr uint32_t kKnown = SMM_GRIB_AEC_SIGNED | SMM_GRIB_AEC_3BYTE | SMM_GRIB_AEC_MSB | SMM_GRIB_AEC_PREPROCESS |
                              SMM_GRIB_AEC_RESTRICTED | SMM_GRIB_AEC_PAD_RSI;
  for (int64_t b = 0; b < n_batch; ++b) {
    const smm_grib_aec_t& r = recs[b];
    const std::string at = "recs[" + std::to_string(b) + "]";
    if (r.nbits < 0 || r.nbits > 32) return err = at + ".nbits must be within 0..32", false;
    if (r.reserved != 0) return err = at + ".reserved must be 0", false;
    if (r.n_values >= ((uint64_t)1 << 31)) return err = at + ".n_values must be below 2^31", false;
    if (r.nbits == 0) continue;   // a constant field has no stream
    if (r.block_size != 8 && r.block_size != 16 && r.block_size != 32 && r.block_size != 64)
      return err = at + ".block_size must be 8, 16, 32 or 64", false;
    if (r.rsi < 1 || r.rsi > 4096) return err = at + ".rsi must be within 1..4096", false;
    if (r.flags & SMM_GRIB_AEC_SIGNED) return err = at + ".flags: AEC_DATA_SIGNED (signed samples) is not decoded", false;
    if (r.flags & SMM_GRIB_AEC_RESTRICTED) return err = at + ".flags: AEC_RESTRICTED (the restricted code set) is not decoded", false;
    if (r.flags & SMM_GRIB_AEC_PAD_RSI) return err = at + ".flags: AEC_PAD_RSI (byte-padded intervals) is not decoded", false;
    if (r.flags & ~kKnown) return err = at + ".flags has bits outside ccsdsFlags", false;
    if (r.byte_off > (uint64_t)x_bytes || r.byte_len > (uint64_t)x_bytes - r.byte_off)
      return err = at + ": bytes [" + std::to_string(r.byte_off) + ", " + std::to_string(r.byte_off) + " + " +
                   std::to_string(r.byte_len) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes", false;
  }
  return true;
}

uint64_t grib_aec_layout(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (byte_off) byte_off[b] = at;
    at += smm_grib::align4(smm_grib::row_bytes(recs[b].n_values, recs[b].nbits));
  }
  return at;
}

bool check_grib_cpx(const smm_grib_cpx_t* recs, int64_t n_batch, int64_t x_bytes, std::string& err) {
  for (int64_t b = 0; b < n_batch; ++b) {
    const smm_grib_cpx_t& r = recs[b];
    const std::string at = "recs[" + std::to_string(b) + "]";
    if (r.order == SMM_GRIB_CPX_SIMPLE) continue;   // simple-packed already: the row's own record says it all
    if (r.order < 0 || r.order > 2) return err = at + ".order (of spatial differencing) must be 0, 1 or 2", false;
    if (r.order > 0 && (r.n_oct < 1 || r.n_oct > 4))
      return err = at + ".n_oct (octets per extra descriptor) must be within 1..4", false;
    if (r.nbits < 0 || r.nbits > 32) return err = at + ".nbits must be within 0..32", false;
    if (r.width_bits < 0 || r.width_bits > 32) return err = at + ".width_bits must be within 0..32", false;
    if (r.length_bits < 0 || r.length_bits > 32) return err = at + ".length_bits must be within 0..32", false;
    if (r.width_ref > 255) return err = at + ".width_ref is one octet: 0..255", false;
    if (r.length_inc > 255) return err = at + ".length_inc is one octet: 0..255", false;
    if (r.reserved != 0) return err = at + ".reserved must be 0", false;
    if (r.n_values >= ((uint64_t)1 << 31)) return err = at + ".n_values must be below 2^31", false;
    if (r.n_values > 0 && r.n_groups == 0) return err = at + ".n_groups is 0 for " + std::to_string(r.n_values) + " values", false;
    if (r.n_values > 0 && r.n_values <= (uint64_t)r.order)
      return err = at + ".n_values must exceed the order of spatial differencing", false;
    if (r.byte_off > (uint64_t)x_bytes || r.byte_len > (uint64_t)x_bytes - r.byte_off)
      return err = at + ": bytes [" + std::to_string(r.byte_off) + ", " + std::to_string(r.byte_off) + " + " +
                   std::to_string(r.byte_len) + ") leave the buffer of " + std::to_string(x_bytes) + " bytes", false;
  }
  return true;
}

uint64_t grib_cpx_layout(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    if (byte_off) byte_off[b] = at;
    if (recs[b].order != SMM_GRIB_CPX_SIMPLE) at += recs[b].n_values * 4;
  }
  return at;
}

bool check_grib_cpx_mvm(const uint8_t* mvm, int64_t n_batch, std::string& err) {
  for (int64_t b = 0; mvm && b < n_batch; ++b)
    if (mvm[b] > 2)
      return err = "mvm[" + std::to_string(b) + "] (missing value management) must be 0, 1 or 2, not " + std::to_string((int)mvm[b]), false;
  return true;
}

uint64_t grib_cpx_layout_mv(const smm_grib_cpx_t* recs, const uint8_t* mvm, int64_t n_batch, uint64_t* byte_off,
                            uint64_t* bitmap_off) {
  uint64_t at = 0;
  for (int64_t b = 0; b < n_batch; ++b) {
    const bool coded = recs[b].order != SMM_GRIB_CPX_SIMPLE;
    if (byte_off) byte_off[b] = at;
    if (coded) at += recs[b].n_values * 4;
    const bool bitmapped = coded && mvm && mvm[b] != 0;
    if (bitmap_off) bitmap_off[b] = bitmapped ? at : SMM_GRIB_NO_BITMAP;
    if (bitmapped) at += ((recs[b].n_values + 7) / 8 + 3) / 4 * 4;
  }
  return at;
}

GribPackScratch grib_pack_scratch(int64_t n_dst, int64_t n_rows) {
  const size_t n = (size_t)std::max<int64_t>(n_rows, 0);
  const size_t segs = n * (size_t)smm_grib::bitmap_segments((uint64_t)n_dst);
  const size_t blocks = n * (size_t)smm_grib::bitmap_blocks((uint64_t)n_dst);
  auto align8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
  GribPackScratch s;
  s.part_min = 0;
  s.part_max = s.part_min + segs * 8;
  s.part_cnt = s.part_max + segs * 8;
  s.rules = align8(s.part_cnt + segs * 4);
  s.table = s.rules + n * sizeof(smm_grib::GribPackRule);
  s.totals = s.table + blocks * sizeof(smm_grib::GribRankEntry);
  s.bytes = align8(s.totals + segs * 4);
  return s;
}

}  // namespace smm

