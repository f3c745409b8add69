// The chunk plan of smm_group_apply_host_grib_pk on the host (smm_grib_plan.cpp compiled with plain g++): plan_grib_chunks
// with units of n_lev * n_inner > 1 records and the per-record out_row_bytes of a packed result -- slot, records, pack
// tables and one row's scratch, as the entries build them.  tests/test_grib_levels_pack_harness.py builds this program with
// AddressSanitizer and UBSan and runs it; it reads no input.  Checked for every plan:
//   - the chunks are whole outer indices and tile [0, n_outer) in order, none empty;
//   - chunk_outer 1 and 2 are honoured, 0 sizes by bytes: a tight free_bytes gives single-outer chunks, never none;
//   - a chunk of more than one outer index keeps staged + rank + Y + packed bytes inside the plan's target, and the
//     target inside an eighth of free_bytes;
//   - a chunk's slot offsets relative to its first row are smm_grib_out_layout of its own rows (mixed widths 1, 7, 12, 16,
//     17, 24, 32), and its scratch is within what the rows were budgeted;
//   - layout_grib_chunk fills a heap block of exactly the chunk's staged bytes plus its pack tables.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/smmregrid_amd.h"
#include "../../smmregrid_amd/csrc/smm_grib_codec.hpp"
#include "../../smmregrid_amd/csrc/smm_internal.h"

namespace {

int n_bad = 0;
#define CHECK(cond, ...)                                    \
  do {                                                      \
    if (!(cond)) {                                          \
      fprintf(stderr, "grib_levels_pack_harness: %s: ", #cond); \
      fprintf(stderr, __VA_ARGS__);                         \
      fprintf(stderr, "\n");                                \
      ++n_bad;                                              \
    }                                                       \
  } while (0)

size_t align8(size_t v) { return (v + 7) & ~(size_t)7; }

struct Call {
  int64_t n_outer, n_lev, n_inner, S, D;
  std::vector<smm_grib_row_t> rows;
  std::vector<smm_grib_bitmap_t> bitmaps;
  std::vector<smm_grib_encode_t> enc;
  std::vector<uint64_t> offs;      // n_rows + 1, the last the total
  std::vector<size_t> out_row;
  int64_t unit() const { return n_lev * n_inner; }
  int64_t n_rows() const { return n_outer * unit(); }
};

// rows of mixed input widths, some with a bitmap (present cells only in the stream), one level without any value; the
// output widths cycle with a period that is no divisor of the unit
Call make_call(int64_t n_outer, int64_t n_lev, int64_t n_inner, int64_t S, int64_t D) {
  static const int widths_in[] = {0, 1, 12, 16, 25, 32};
  static const int widths_out[] = {1, 7, 12, 16, 17, 24, 32};
  Call c{n_outer, n_lev, n_inner, S, D, {}, {}, {}, {}, {}};
  uint64_t at = 0, lcg = 12345;
  for (int64_t b = 0; b < c.n_rows(); ++b) {
    lcg = lcg * 6364136223846793005ull + 1442695040888963407ull;
    const int64_t l = (b / n_inner) % n_lev;
    smm_grib_row_t r{at, -3.5, 0.25, b % 3 ? 1.0 : 100.0, widths_in[b % 6], 0};
    smm_grib_bitmap_t bm{SMM_GRIB_NO_BITMAP, (uint64_t)S};
    if (l == n_lev - 1) {   // an empty level
      bm = smm_grib_bitmap_t{at, 0};
    } else if (b % 4 != 1) {
      bm = smm_grib_bitmap_t{at, (uint64_t)(lcg >> 33) % (uint64_t)(S + 1)};
    }
    if (bm.bitmap_off != SMM_GRIB_NO_BITMAP) {
      at += smm_grib::bitmap_bytes((uint64_t)S);
      r.byte_off = at;
    }
    at += smm_grib::row_bytes(bm.n_values, r.nbits);
    c.rows.push_back(r);
    c.bitmaps.push_back(bm);
    c.enc.push_back(smm_grib_encode_t{b % 2 ? 10.0 : 1.0, widths_out[b % 7], 0});
  }
  std::string err;
  CHECK(smm::check_grib_rules(c.rows.data(), c.n_rows(), err), "%s", err.c_str());
  CHECK(smm::check_grib_ranges(c.rows.data(), c.bitmaps.data(), c.n_rows(), S, (int64_t)at, err), "%s", err.c_str());
  CHECK(smm::check_grib_encode(c.enc.data(), c.n_rows(), D, err), "%s", err.c_str());
  c.offs.assign((size_t)c.n_rows() + 1, 0);
  c.offs.back() = smm::grib_out_layout(D, c.enc.data(), c.n_rows(), c.offs.data());
  const size_t scratch = smm::grib_pack_scratch(D, 1).bytes;
  for (int64_t b = 0; b < c.n_rows(); ++b)
    c.out_row.push_back((size_t)(c.offs[(size_t)b + 1] - c.offs[(size_t)b]) + smm::kGribOutRecordBytes + smm::kGribPackTableBytes +
                        scratch);
  return c;
}

// all bytes of outer index o that the plan counts
size_t unit_bytes(const Call& c, int64_t o) {
  size_t all = (size_t)c.unit() * (size_t)c.D * 8;
  for (int64_t b = o * c.unit(); b < (o + 1) * c.unit(); ++b) {
    const smm::GribRowCost k = smm::grib_row_cost(c.rows[(size_t)b], &c.bitmaps[(size_t)b], c.S);
    all += k.staged() + k.rank + c.out_row[(size_t)b];
  }
  return all;
}

// returns the number of chunks
size_t check_plan(const Call& c, int64_t chunk_outer, size_t free_bytes, const char* what) {
  const smm::GribChunkPlan plan = smm::plan_grib_chunks(c.rows.data(), c.bitmaps.data(), c.n_outer, c.unit(), c.S, c.D, chunk_outer,
                                                        free_bytes, c.out_row.data());
  const int64_t unit = c.unit();
  CHECK(!plan.chunks.empty(), "%s", what);
  int64_t next = 0, max_rows = 0;
  size_t max_x = 0, max_rank = 0;
  if (chunk_outer <= 0 && free_bytes > 0) CHECK(plan.target <= std::max<size_t>(free_bytes / 8, 1), "%s: target %zu", what, plan.target);
  if (chunk_outer <= 0) CHECK(plan.target > 0, "%s", what);
  for (const smm::GribChunk& ch : plan.chunks) {
    CHECK(ch.r0 == next, "%s: chunk at %lld, expected %lld", what, (long long)ch.r0, (long long)next);
    CHECK(ch.nr > 0 && ch.nr % unit == 0 && ch.r0 % unit == 0, "%s: %lld rows from %lld", what, (long long)ch.nr, (long long)ch.r0);
    if (ch.nr <= 0) return 0;
    const int64_t o0 = ch.r0 / unit, no = ch.nr / unit;
    CHECK(o0 + no <= c.n_outer, "%s: a chunk leaves the call", what);
    if (o0 + no > c.n_outer) return 0;
    if (chunk_outer > 0) CHECK(no == std::min(chunk_outer, c.n_outer - o0), "%s: %lld outer indices", what, (long long)no);
    size_t x = 0, rank = 0, all = 0;
    for (int64_t b = ch.r0; b < ch.r0 + ch.nr; ++b) {
      const smm::GribRowCost k = smm::grib_row_cost(c.rows[(size_t)b], &c.bitmaps[(size_t)b], c.S);
      x += k.staged();
      rank += k.rank;
    }
    for (int64_t o = o0; o < o0 + no; ++o) all += unit_bytes(c, o);
    CHECK(ch.x_bytes == x && ch.rank_bytes == rank, "%s: staged %zu / %zu, rank %zu / %zu", what, ch.x_bytes, x, ch.rank_bytes, rank);
    if (chunk_outer <= 0 && no > 1) CHECK(all <= plan.target, "%s: %zu bytes in a chunk of %lld against %zu", what, all, (long long)no, plan.target);
    // and one more outer index would not have fitted
    if (chunk_outer <= 0 && o0 + no < c.n_outer) CHECK(all + unit_bytes(c, o0 + no) > plan.target, "%s: a chunk stopped early", what);
    // the chunk's slots, relative to its first row: the layout of its own rows
    std::vector<uint64_t> local((size_t)ch.nr);
    const uint64_t slots = smm::grib_out_layout(c.D, c.enc.data() + ch.r0, ch.nr, local.data());
    CHECK(slots == c.offs[(size_t)(ch.r0 + ch.nr)] - c.offs[(size_t)ch.r0], "%s: slot bytes", what);
    for (int64_t r = 0; r < ch.nr; ++r) {
      CHECK(local[(size_t)r] == c.offs[(size_t)(ch.r0 + r)] - c.offs[(size_t)ch.r0], "%s: slot %lld", what, (long long)r);
      CHECK(local[(size_t)r] % 4 == 0, "%s: slot %lld is not word aligned", what, (long long)r);
    }
    // what the chunk's packed result takes on the device stays within what its rows were budgeted
    size_t budget = 0;
    for (int64_t b = ch.r0; b < ch.r0 + ch.nr; ++b) budget += c.out_row[(size_t)b];
    const size_t packed = (size_t)slots + (size_t)ch.nr * (smm::kGribOutRecordBytes + smm::kGribPackTableBytes) +
                          smm::grib_pack_scratch(c.D, ch.nr).bytes;
    CHECK(packed <= budget, "%s: packed %zu against %zu budgeted", what, packed, budget);
    // the staging block: the chunk's X, then 8-byte aligned its pack tables -- exactly this many bytes on the heap
    std::vector<char> hx(align8(ch.x_bytes) + (size_t)ch.nr * smm::kGribPackTableBytes, (char)0x5a);
    const smm::GribChunkLayout lay = smm::layout_grib_chunk(hx.data(), ch, c.rows.data(), c.bitmaps.data(), c.S);
    CHECK(lay.end == ch.x_bytes, "%s: layout ends at %zu of %zu", what, lay.end, ch.x_bytes);
    memset(hx.data() + align8(ch.x_bytes), 0, (size_t)ch.nr * smm::kGribPackTableBytes);
    next += ch.nr;
    max_rows = std::max(max_rows, ch.nr);
    max_x = std::max(max_x, ch.x_bytes);
    max_rank = std::max(max_rank, ch.rank_bytes);
  }
  CHECK(next == c.n_rows(), "%s: the chunks cover %lld of %lld rows", what, (long long)next, (long long)c.n_rows());
  CHECK(plan.max_rows == max_rows && plan.max_x == max_x && plan.max_rank == max_rank, "%s: the plan's maxima", what);
  return plan.chunks.size();
}

}  // namespace

int main() {
  // 7 outer indices of 3 levels x 2 inner rows: units of 6 records, output widths of period 7
  const Call c = make_call(7, 3, 2, 1000, 300);
  CHECK(check_plan(c, 1, 0, "chunk_outer 1") == 7, "chunk_outer 1");
  CHECK(check_plan(c, 2, 0, "chunk_outer 2") == 4, "chunk_outer 2");
  CHECK(check_plan(c, 7, 0, "chunk_outer 7") == 1, "chunk_outer 7");
  CHECK(check_plan(c, 100, 0, "chunk_outer 100") == 1, "chunk_outer 100");
  CHECK(check_plan(c, 0, 0, "chunk_outer 0, free unknown") == 1, "a small call is one chunk");
  CHECK(check_plan(c, 0, (size_t)64 << 30, "chunk_outer 0, 64 GiB free") == 1, "a small call is one chunk");
  // tight: nothing but one outer index fits
  CHECK(check_plan(c, 0, 1, "free_bytes 1") == 7, "single-outer chunks");
  CHECK(check_plan(c, 0, 8 * 1000, "free_bytes 8000") == 7, "single-outer chunks");
  size_t most = 0;
  for (int64_t o = 0; o < c.n_outer; ++o) most = std::max(most, unit_bytes(c, o));
  CHECK(check_plan(c, 0, 8 * (most - 1), "one byte short of the largest unit") >= 4, "mostly single-outer chunks");
  // room for two or three outer indices
  const size_t two = check_plan(c, 0, 8 * (2 * most), "room for two"), three = check_plan(c, 0, 8 * (3 * most + 1), "room for three");
  CHECK(two >= 3 && two <= 4, "%zu chunks with room for two", two);
  CHECK(three >= 2 && three <= 3, "%zu chunks with room for three", three);
  // the packed result counts: the same call without out_row_bytes fits more per chunk
  const smm::GribChunkPlan bare = smm::plan_grib_chunks(c.rows.data(), c.bitmaps.data(), c.n_outer, c.unit(), c.S, c.D, 0, 8 * (2 * most));
  CHECK(bare.chunks.size() <= two, "out_row_bytes is not counted");
  // other shapes: one level, one inner row, one outer index, a grid of one cell, an empty call
  for (const Call& k : {make_call(5, 1, 2, 33, 1), make_call(4, 8, 1, 2592, 288), make_call(1, 2, 3, 64, 65), make_call(3, 2, 2, 1, 31)}) {
    for (int64_t chunk_outer : {1, 2, 0})
      for (size_t free_bytes : {(size_t)0, (size_t)1, (size_t)1 << 20}) check_plan(k, chunk_outer, free_bytes, "other shapes");
  }
  CHECK(smm::plan_grib_chunks(c.rows.data(), c.bitmaps.data(), 0, c.unit(), c.S, c.D, 0, 0, c.out_row.data()).chunks.empty(), "empty call");
  if (n_bad) {
    fprintf(stderr, "grib_levels_pack_harness: %d checks failed\n", n_bad);
    return 2;
  }
  printf("OK\n");
  return 0;
}
