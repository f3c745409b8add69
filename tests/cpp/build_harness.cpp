// Host-only harness around smm_build.cpp (COO -> CSR -> SELL-64 -> LDS tile plans), compiled
// with g++ -fsanitize=address,undefined by tests/test_build_sanitized.py.
// argv[1]: host threads of the builders (0 / absent = automatic)
// stdin : n_src n_dst nnz, then nnz lines "src1 dst1 w"
// stdout: the canonical CSR and invariants of the SELL / tile-plan structures.
#include <cinttypes>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_internal.h"

int main(int argc, char** argv) {
  if (argc > 1) smm::set_host_threads(atoi(argv[1]));
  long long n_src, n_dst, nnz;
  if (scanf("%lld %lld %lld", &n_src, &n_dst, &nnz) != 3) return 2;
  std::vector<int32_t> src((size_t)nnz), dst((size_t)nnz);
  std::vector<double> w((size_t)nnz);
  for (long long k = 0; k < nnz; ++k)
    if (scanf("%d %d %lf", &src[(size_t)k], &dst[(size_t)k], &w[(size_t)k]) != 3) return 2;
  smm::HostCsr csr;
  std::string err;
  if (!smm::build_csr(n_src, n_dst, nnz, src.data(), dst.data(), w.data(), csr, err)) {
    printf("ERROR %s\n", err.c_str());
    return 0;
  }
  smm::HostSell sell;
  smm::build_sell(csr, sell);
  printf("CSR %lld %lld %lld %lld\n", (long long)csr.nnz, (long long)csr.n_used_src,
         (long long)csr.max_row_nnz, (long long)sell.n_slots);
  for (int64_t d = 0; d <= csr.n_dst; ++d) printf("%lld ", (long long)csr.rowptr[(size_t)d]);
  printf("\n");
  for (int64_t p = 0; p < csr.nnz; ++p) printf("%d ", csr.col[(size_t)p]);
  printf("\n");
  for (int64_t p = 0; p < csr.nnz; ++p) printf("%.17g ", csr.val[(size_t)p]);
  printf("\n");
  // SELL invariants: every link sits at slice_off + k*64 + lane, padding repeats the last column
  long long bad = 0;
  for (int64_t d = 0; d < csr.n_dst; ++d) {
    const int64_t s = d >> 6, r = d & 63;
    const int64_t base = sell.slice_off[(size_t)s] + r;
    const int64_t nslots = (sell.slice_off[(size_t)s + 1] - sell.slice_off[(size_t)s]) / 64;
    const int32_t len = sell.rowlen[(size_t)d];
    if (len != csr.rowptr[(size_t)d + 1] - csr.rowptr[(size_t)d] || len > nslots) ++bad;
    for (int64_t k = 0; k < nslots; ++k) {
      const int32_t c = sell.col[(size_t)(base + k * 64)];
      const double v = sell.val[(size_t)(base + k * 64)];
      if (k < len) {
        if (c != csr.col[(size_t)(csr.rowptr[(size_t)d] + k)] || v != csr.val[(size_t)(csr.rowptr[(size_t)d] + k)]) ++bad;
      } else {
        if (v != 0.0 || c < 0 || (n_src > 0 && c >= n_src)) ++bad;
      }
    }
  }
  // both tile-plan shapes: every link's LDS index must resolve to its source column
  for (int rows : {256, 64, 16}) {
    const int spb = rows / 64;   // 0 for the sub-slice shape
    smm::HostTilePlan plan;
    const int64_t budget = rows == 256 ? 512 : 128;
    smm::build_tile_plan(csr, sell, rows, 16, budget, plan);
    auto check_plan = [&](int64_t limit) {
      long long pbad = 0;
      if (!plan.valid) return pbad;
      const int64_t rows_per_block = rows;
      int64_t direct_links = 0;
      for (int64_t b = 0; b < plan.n_blocks; ++b) {
        const int64_t nch = plan.blk_chunk_off[(size_t)b + 1] - plan.blk_chunk_off[(size_t)b];
        if (nch < 0 || nch > limit || nch > plan.max_block_chunks) ++pbad;
        if (plan.blk_direct[(size_t)b]) {
          if (nch != 0) ++pbad;
          const int64_t d0 = b * rows_per_block, d1 = std::min(csr.n_dst, d0 + rows_per_block);
          direct_links += csr.rowptr[(size_t)d1] - csr.rowptr[(size_t)d0];
        }
      }
      if (direct_links != plan.direct_links || plan.total_chunks != (int64_t)plan.chunk_src.size()) ++pbad;
      for (int64_t d = 0; d < csr.n_dst; ++d) {
        const int64_t b = d / rows_per_block, s = d >> 6, r = d & 63;
        if (plan.blk_direct[(size_t)b]) continue;  // gathered from X directly, no LDS indices
        const int64_t c0 = plan.blk_chunk_off[(size_t)b];
        const int64_t base = sell.slice_off[(size_t)s] + r;
        for (int32_t k = 0; k < sell.rowlen[(size_t)d]; ++k) {
          const int32_t li = plan.lcol[(size_t)(base + (int64_t)k * 64)];
          const int64_t ch = li / 16, e = li % 16;
          if (c0 + ch >= plan.blk_chunk_off[(size_t)b + 1]) { ++pbad; continue; }
          const int64_t col = (int64_t)plan.chunk_src[(size_t)(c0 + ch)] * 16 + e;
          if (col != csr.col[(size_t)(csr.rowptr[(size_t)d] + k)]) ++pbad;
        }
      }
      return pbad;
    };
    long long pbad = check_plan(budget);
    printf("PLAN %d %d %lld %lld %lld %lld %lld\n", spb, (int)plan.valid, (long long)plan.max_block_chunks,
           (long long)plan.total_chunks, (long long)plan.distinct_chunks, (long long)plan.direct_links, pbad);
    // tightened budget: demoted blocks are direct, every remaining LDS index still resolves
    const int64_t chosen = smm::tighten_tile_plan(csr, plan, budget);
    long long tbad = check_plan(chosen);
    if (plan.valid && plan.direct_links * 100 > csr.nnz && chosen != budget) ++tbad;
    printf("TIGHT %d %lld %lld %lld %lld\n", spb, (long long)chosen, (long long)plan.max_block_chunks,
           (long long)plan.direct_links, tbad);
  }
  // adopt_csr: the canonical CSR round-trips unchanged; each corruption of it is rejected
  {
    long long abad = 0;
    smm::HostCsr back;
    std::string e2;
    if (!smm::adopt_csr(n_src, n_dst, csr.rowptr.data(), csr.col.data(), csr.val.data(), back, e2)) ++abad;
    if (back.rowptr != csr.rowptr || back.col != csr.col || back.val != csr.val || back.nnz != csr.nnz ||
        back.n_used_src != csr.n_used_src || back.max_row_nnz != csr.max_row_nnz)
      ++abad;
    smm::HostCsr tmp;
    if (csr.nnz > 0) {
      std::vector<int32_t> c2(csr.col);
      c2[0] = (int32_t)n_src;                                   // column out of range
      if (smm::adopt_csr(n_src, n_dst, csr.rowptr.data(), c2.data(), csr.val.data(), tmp, e2)) ++abad;
      std::vector<int64_t> r2(csr.rowptr);
      r2[0] = 1;                                                // rowptr must start at 0
      if (smm::adopt_csr(n_src, n_dst, r2.data(), csr.col.data(), csr.val.data(), tmp, e2)) ++abad;
    }
    for (int64_t d = 0; d < csr.n_dst; ++d) {
      if (csr.rowptr[(size_t)d + 1] - csr.rowptr[(size_t)d] >= 2) {
        std::vector<int32_t> c2(csr.col);
        std::swap(c2[(size_t)csr.rowptr[(size_t)d]], c2[(size_t)csr.rowptr[(size_t)d] + 1]);  // unsorted row
        if (smm::adopt_csr(n_src, n_dst, csr.rowptr.data(), c2.data(), csr.val.data(), tmp, e2)) ++abad;
        c2 = csr.col;
        c2[(size_t)csr.rowptr[(size_t)d] + 1] = c2[(size_t)csr.rowptr[(size_t)d]];            // repeated column
        if (smm::adopt_csr(n_src, n_dst, csr.rowptr.data(), c2.data(), csr.val.data(), tmp, e2)) ++abad;
        std::vector<int64_t> r2(csr.rowptr);
        r2[(size_t)d + 1] = r2[(size_t)d] - 1;                                                  // decreasing rowptr
        if (smm::adopt_csr(n_src, n_dst, r2.data(), csr.col.data(), csr.val.data(), tmp, e2)) ++abad;
        break;
      }
    }
    printf("ADOPTBAD %lld\n", abad);
  }
  // chunk sizing of the host pipelines (smm_apply_host / smm_group_apply_host): Y counts too
  {
    long long cbad = 0;
    const size_t GiB = (size_t)1 << 30, MiB = (size_t)1 << 20;
    // config 2: 3600 rows, S = 1 038 240 f64 rows on 128-B lines, D = 64 800, U = 259 200
    smm::HostChunk c = smm::host_chunk_units(3600, 8305920, 518400, 2073600, 32, 128, 0, 200 * GiB);
    if (!c.pack || c.units % 128 != 0 || c.units < 128 || (size_t)c.units * (2073600 + 518400) > 512 * MiB) ++cbad;
    // U << D: 64 used source cells feeding a 12.6-M-cell target (a regional subset onto HEALPix): the
    // chunk is bound by its Y bytes, not by the packed X
    c = smm::host_chunk_units(4096, 40000 * 8, (size_t)12582912 * 8, 64 * 8, 32, 128, 0, 200 * GiB);
    if (c.units < 1 || (size_t)c.units * ((size_t)12582912 * 8 + 64 * 8) > GiB) ++cbad;
    if (c.pack && c.units < 32) ++cbad;
    // the same with little free memory: four buffers stay within a quarter of it
    c = smm::host_chunk_units(4096, 40000 * 8, (size_t)12582912 * 8, 64 * 8, 32, 128, 0, 4 * GiB);
    if (c.units < 1 || 4 * (size_t)c.units * ((c.pack ? 64 * 8 : 40000 * 8) + (size_t)12582912 * 8) > 4 * GiB + 4 * ((size_t)12582912 * 8)) ++cbad;
    if (c.pack && c.units < 32) ++cbad;
    // short batches never pack; a requested chunk size is kept
    c = smm::host_chunk_units(16, 8000, 800, 2000, 32, 128, 0, 0);
    if (c.pack || c.units != 16) ++cbad;
    c = smm::host_chunk_units(1000, 8000, 800, 2000, 32, 128, 100, 0);
    if (!c.pack || c.units != 100) ++cbad;
    c = smm::host_chunk_units(1000, 8000, 800, 2000, 32, 128, 7, 0);
    if (c.pack || c.units != 7) ++cbad;
    c = smm::host_chunk_units(1000, 8000, 800, 0, 32, 128, 0, 0);
    if (c.pack || c.units != 1000) ++cbad;
    // a level group whose 32 batch entries of all levels exceed 1 GiB of staging keeps whole rows
    c = smm::host_chunk_units(120, (size_t)75 * 11778304, (size_t)75 * 518400, (size_t)39000000 * 8, 32, 1, 0, 200 * GiB);
    if (c.pack || c.units < 1) ++cbad;
    printf("CHUNKBAD %lld\n", cbad);
  }
  // chunk plan of smm_group_apply_host (smm::plan_group_chunks): outer blocks with every level, or level-major
  {
    long long gbad = 0;
    struct Args {
      int64_t n_outer, n_lev, n_inner, S, D;
      size_t xsz, ysz;
      std::vector<int64_t> used;
      bool allowed;
      int64_t requested;
      size_t free_bytes;
      int64_t budget_kb;
    };
    // What holds for every plan.  The chunks tile (outer x level) exactly once in pipeline order (outer blocks ascending,
    // the level ranges of a block ascending), none is empty, x_bytes is the packed size of the chunk's levels, the maxima
    // are the maxima of the list.  pack is false exactly when the chunks are whole rows: every level, blocks of one
    // size, no packed bytes.  A level-major plan (packed, and not host_chunk_units' packed outer blocks) has blocks of
    // bo >= min(32 batch entries, n_outer) outer indices; a chunk of several levels keeps X + Y within the staging
    // target (256 MiB, or budget_kb) and takes every level that fits; a chunk of one level keeps X within four targets.
    // With free_bytes known, the four device buffers (2 x max_x, 2 x max_y) stay within a quarter of it once they
    // exceed the 2 GiB that host_chunk_units' clamp tolerates -- in blocks of the outer axis unless one index is left.
    long long n_level_major = 0, n_multi = 0, n_y_ended = 0, n_whole = 0, n_mem_bound = 0;
    auto plan_of = [&](const Args& a) {
      const size_t GiB = (size_t)1 << 30;
      const smm::GroupChunkPlan p = smm::plan_group_chunks(a.n_outer, a.n_lev, a.n_inner, a.S, a.D, a.xsz, a.ysz, a.used.data(),
                                                           a.allowed, a.requested, a.free_bytes, a.budget_kb);
      std::vector<int> seen((size_t)(a.n_outer * a.n_lev), 0);
      size_t max_x = 0, max_y = 0, max_rows = 0;
      if (p.x_row != (a.S * a.xsz + 127) / 128 * 128) ++gbad;
      if (p.chunks.empty()) ++gbad;
      int64_t next_o = 0, next_l = 0, block_no = 0;
      for (const smm::GroupChunk& c : p.chunks) {
        if (c.no < 1 || c.nl < 1 || c.o0 < 0 || c.l0 < 0 || c.o0 + c.no > a.n_outer || c.l0 + c.nl > a.n_lev) {
          ++gbad;
          continue;
        }
        // pipeline order: the next level range of the same block, or the first one of the next block
        if (c.l0 != next_l || c.o0 != next_o || (c.l0 > 0 && c.no != block_no)) ++gbad;
        block_no = c.no;
        next_l = c.l0 + c.nl;
        if (next_l == a.n_lev) next_l = 0, next_o = c.o0 + c.no;
        size_t xb = 0;
        for (int64_t l = c.l0; l < c.l0 + c.nl; ++l) {
          xb += (size_t)a.used[(size_t)l] * c.no * a.n_inner * a.xsz;
          for (int64_t o = c.o0; o < c.o0 + c.no; ++o) ++seen[(size_t)(o * a.n_lev + l)];
        }
        if (c.x_bytes != (p.pack ? xb : 0)) ++gbad;
        max_x = std::max(max_x, p.pack ? xb : (size_t)c.no * a.n_lev * a.n_inner * p.x_row);
        max_y = std::max(max_y, (size_t)c.no * a.n_inner * c.nl * a.D * a.ysz);
        max_rows = std::max(max_rows, (size_t)(c.no * a.n_lev * a.n_inner));
      }
      if (next_l != 0 || next_o != a.n_outer) ++gbad;
      for (int v : seen) gbad += v != 1;
      if (p.max_x != max_x || p.max_y != max_y || p.max_rows != max_rows) ++gbad;
      if (p.chunks.empty()) return p;
      // packing: only when the call allows it and at most four fifths of the selected cells are used
      int64_t used_total = 0;
      for (int64_t u : a.used) used_total += u;
      const bool may_pack = a.allowed && used_total > 0 && used_total * 5 <= a.n_lev * a.S * 4;
      if (p.pack && !may_pack) ++gbad;
      if (p.pack && a.requested > 0 && a.budget_kb > 0) ++gbad;
      const int64_t min_outer = (32 + a.n_inner - 1) / a.n_inner, bo = p.chunks[0].no;
      const smm::HostChunk hc = smm::host_chunk_units(a.n_outer, (size_t)a.n_lev * a.n_inner * p.x_row,
                                                      (size_t)a.n_lev * a.n_inner * a.D * a.ysz,
                                                      may_pack ? (size_t)used_total * a.n_inner * a.xsz : 0, min_outer, 1,
                                                      a.requested, a.free_bytes);
      const bool level_major = p.pack && !(hc.pack && a.budget_kb <= 0);
      const size_t all = 2 * (max_x + max_y);
      if (!level_major) {   // blocks of the outer axis, every level: whole rows or packed
        for (const smm::GroupChunk& c : p.chunks)
          if (c.l0 != 0 || c.nl != a.n_lev || (c.no != bo && c.o0 + c.no != a.n_outer) || c.no > bo) ++gbad;
        if (a.requested > 0 && bo != std::min(a.requested, a.n_outer)) ++gbad;
        if (a.requested <= 0 && a.free_bytes > 0 && all > 2 * GiB && max_x + max_y > a.free_bytes / 4 && bo > 1) ++gbad;
        n_whole += !p.pack;
        return p;
      }
      ++n_level_major;
      const size_t target = a.budget_kb > 0 ? (size_t)a.budget_kb << 10 : 256 * ((size_t)1 << 20);
      if (a.requested > 0 || bo < std::min(min_outer, a.n_outer)) ++gbad;
      if (a.free_bytes > 0 && all > 2 * GiB && all > a.free_bytes / 4) ++gbad;
      n_mem_bound += a.free_bytes > 0 && all > 2 * GiB;
      for (const smm::GroupChunk& c : p.chunks) {
        if ((c.no != bo && c.o0 + c.no != a.n_outer) || c.no > bo) ++gbad;
        const size_t y_level = (size_t)c.no * a.n_inner * a.D * a.ysz;
        if (c.nl == 1 && c.x_bytes > 4 * target) ++gbad;
        if (c.nl > 1 && c.x_bytes + (size_t)c.nl * y_level > target) ++gbad;
        n_multi += c.nl > 1;
        if (c.l0 + c.nl < a.n_lev) {   // the next level was refused: it did not fit
          const size_t x1 = c.x_bytes + (size_t)a.used[(size_t)(c.l0 + c.nl)] * c.no * a.n_inner * a.xsz;
          const size_t y1 = (size_t)(c.nl + 1) * y_level, all1 = 2 * (std::max(x1, max_x) + std::max(y1, max_y));
          const bool no_memory = a.free_bytes > 0 && all1 > 2 * GiB && all1 > a.free_bytes / 4;
          if (x1 + y1 <= target && !no_memory) ++gbad;
          n_y_ended += x1 <= target && x1 + y1 > target;   // the Y bound, not the X bound, ended the chunk
        }
      }
      return p;
    };
    struct C { int64_t o0, no, l0, nl; size_t x_bytes; };
    auto expect = [&](const Args& a, bool pack, const std::vector<C>& want) {
      const smm::GroupChunkPlan p = plan_of(a);
      bool ok = p.pack == pack && p.chunks.size() == want.size();
      for (size_t i = 0; ok && i < want.size(); ++i) {
        const smm::GroupChunk& c = p.chunks[i];
        ok = c.o0 == want[i].o0 && c.no == want[i].no && c.l0 == want[i].l0 && c.nl == want[i].nl && c.x_bytes == want[i].x_bytes;
      }
      if (!ok) ++gbad;
    };
    const size_t MiB = (size_t)1 << 20, GiB = (size_t)1 << 30;
    // Outer-block packing.  S = 10^6 f64 (rows of 8 000 000 B, a multiple of 128), D = 1000, U = 350 000 of 3 * 10^6 cells
    // (<= 4/5).  host_chunk_units: packed unit 350 000 * 8 + 3 * 1000 * 8 = 2 824 000 B; 256 MiB / that = 95 units, cut
    // to the cap max(32, 32 MiB / unit = 11, ceil(100 / 8) = 13) = 32: blocks of 32, 32, 32 and a short 4, all levels each,
    // x_bytes = 350 000 * no * 8
    const Args big{100, 3, 1, 1000000, 1000, 8, 8, {200000, 100000, 50000}, true, 0, 0, 0};
    expect(big, true, {{0, 32, 0, 3, 89600000}, {32, 32, 0, 3, 89600000}, {64, 32, 0, 3, 89600000}, {96, 4, 0, 3, 11200000}});
    // packing ruled out by the flags: whole rows, unit 3 * 8 000 000 + 24 000 B, 256 MiB / that = 11 (< the 13 of
    // eight chunks per call): nine blocks of 11 and a last of 1
    std::vector<C> rows11;
    for (int64_t o = 0; o < 100; o += 11) rows11.push_back({o, std::min<int64_t>(11, 100 - o), 0, 3, 0});
    Args a = big;
    a.allowed = false;
    expect(a, false, rows11);
    // more than four fifths of the cells used (2.5 M * 5 > 3 M * 4): whole rows, the same blocks
    a = big;
    a.used = {900000, 800000, 800000};
    expect(a, false, rows11);
    // a requested chunk_outer is kept and level-major never entered, whatever the budget: 7 (< 32 entries) does not
    // pack; 40 packs, but not when the tuning knob asks for level-major chunks
    a = big;
    a.requested = 7;
    a.budget_kb = 64;
    std::vector<C> rows7;
    for (int64_t o = 0; o < 100; o += 7) rows7.push_back({o, std::min<int64_t>(7, 100 - o), 0, 3, 0});
    expect(a, false, rows7);
    a.requested = 40;
    expect(a, false, {{0, 40, 0, 3, 0}, {40, 40, 0, 3, 0}, {80, 20, 0, 3, 0}});
    a.budget_kb = 0;
    expect(a, true, {{0, 40, 0, 3, 112000000}, {40, 40, 0, 3, 112000000}, {80, 20, 0, 3, 56000000}});
    // Level-major, budget 64 KiB: target 65 536 B, cap 262 144 B.  40 outer indices, f64: a level of 100 used cells is
    // 100 * 40 * 8 = 32 000 B of X, one of 10 is 3 200 B, and every level brings 40 * 50 * 8 = 16 000 B of Y;
    // bo = 262 144 / 800 = 327 -> 40.  Two wide levels are 64 000 + 32 000 = 96 000 B: {1}, {1}; the third with a thin
    // one 35 200 + 32 000 = 67 200: {1}; the two thin ones 6 400 + 32 000 = 38 400: {2}.  (X alone took 64 000 | 38 400:
    // {2}, {3} before Y counted.)
    const Args thin{40, 5, 1, 1000, 50, 8, 8, {100, 100, 100, 10, 10}, true, 0, 0, 64};
    expect(thin, true, {{0, 40, 0, 1, 32000}, {0, 40, 1, 1, 32000}, {0, 40, 2, 1, 32000}, {0, 40, 3, 2, 6400}});
    // with D = 1 the Y of a level is 320 B and X decides, the plan from before Y counted: 64 000 + 640 = 64 640 fits, a
    // third wide level (96 000) does not: {2}; then 38 400 + 960 = 39 360: {3}
    a = thin;
    a.D = 1;
    expect(a, true, {{0, 40, 0, 2, 64000}, {0, 40, 2, 3, 38400}});
    // the same for a packed field and result (2-byte cells) under 16 KiB: levels of 8 000 and 800 B of X, 4 000 B of Y
    // each: 16 000 + 8 000 > 16 384: {1}, {1}; 8 800 + 8 000 = 16 800: {1}; 1 600 + 8 000 = 9 600: {2}
    a = thin;
    a.xsz = a.ysz = 2;
    a.budget_kb = 16;
    expect(a, true, {{0, 40, 0, 1, 8000}, {0, 40, 1, 1, 8000}, {0, 40, 2, 1, 8000}, {0, 40, 3, 2, 1600}});
    // a level beyond the target on its own (500 * 40 * 8 = 160 000 B > 65 536) is still taken, alone
    const Args wide{40, 3, 1, 1000, 50, 8, 8, {100, 500, 100}, true, 0, 0, 64};
    expect(wide, true, {{0, 40, 0, 1, 32000}, {0, 40, 1, 1, 160000}, {0, 40, 2, 1, 32000}});
    // bo cut by the cap: the widest level is 4 000 B per outer index, 262 144 / 4 000 = 65: blocks of 65 and 35.
    // 65: 260 000 | 52 000 | 52 000 (two would be 104 000 of X); 35: 140 000 | 28 000 | 28 000 (two are 56 000 of X and
    // 2 * 35 * 400 = 28 000 of Y: 84 000; one chunk of 56 000 before Y counted)
    const Args capped{100, 3, 1, 1000, 50, 8, 8, {500, 100, 100}, true, 0, 0, 64};
    expect(capped, true, {{0, 65, 0, 1, 260000}, {0, 65, 1, 1, 52000}, {0, 65, 2, 1, 52000}, {65, 35, 0, 1, 140000},
                          {65, 35, 1, 1, 28000}, {65, 35, 2, 1, 28000}});
    // bo cut by the free memory: free / 8 / (4 000 + 50 * 8) = 40 with 1 408 000 B free: blocks of 40, 40, 20.
    // 40: 160 000 | 32 000 | 32 000 (two: 64 000 + 32 000 of Y = 96 000; one chunk before); 20: 80 000 | 16 000 + 16 000
    // with 16 000 of Y = 48 000
    a = capped;
    a.free_bytes = 8 * 4400 * 40;
    expect(a, true, {{0, 40, 0, 1, 160000}, {0, 40, 1, 1, 32000}, {0, 40, 2, 1, 32000}, {40, 40, 0, 1, 160000},
                     {40, 40, 1, 1, 32000}, {40, 40, 2, 1, 32000}, {80, 20, 0, 1, 80000}, {80, 20, 1, 2, 32000}});
    // ... and to 31 (< the 32 entries a packed chunk needs): whole rows after all, in host_chunk_units' block (all 100)
    a.free_bytes = 8 * 4400 * 31;
    expect(a, false, {{0, 100, 0, 3, 0}});
    // 10 outer indices (>= 8, < 32) are still packed level-major: the default 256-MiB target takes all three levels
    // (56 000 of X, 12 000 of Y), 16 KiB (cap 65 536, bo = 16 -> 10) takes 40 000 | 8 000 | 8 000 (two: 16 000 + 8 000
    // of Y = 24 000 > 16 384; one chunk before Y counted); 7 outer indices are not packed
    a = capped;
    a.n_outer = 10;
    a.budget_kb = 0;
    expect(a, true, {{0, 10, 0, 3, 56000}});
    a.budget_kb = 16;
    expect(a, true, {{0, 10, 0, 1, 40000}, {0, 10, 1, 1, 8000}, {0, 10, 2, 1, 8000}});
    a.n_outer = 7;
    expect(a, false, {{0, 7, 0, 3, 0}});
    // n_inner = 2: a packed chunk needs 16 outer indices.  The widest level is 8 000 B per outer index, cap / that = 32
    // -> 20: 160 000 | 32 000 | 32 000 (two: 64 000 + 2 * 20 * 800 = 32 000 of Y; one chunk before Y counted).  Free
    // memory for 16 (per outer index 8 000 + 2 * 50 * 8): blocks of 16 (128 000 | 25 600 | 25 600: two are 51 200 +
    // 25 600 of Y = 76 800) and 4 (32 000 + 6 400 + 6 400 = 44 800 and 3 * 4 * 800 = 9 600 of Y, all three levels); for
    // 15: whole rows
    a = capped;
    a.n_outer = 20;
    a.n_inner = 2;
    expect(a, true, {{0, 20, 0, 1, 160000}, {0, 20, 1, 1, 32000}, {0, 20, 2, 1, 32000}});
    a.free_bytes = 8 * 8800 * 16;
    expect(a, true, {{0, 16, 0, 1, 128000}, {0, 16, 1, 1, 25600}, {0, 16, 2, 1, 25600}, {16, 4, 0, 3, 44800}});
    a.free_bytes = 8 * 8800 * 15;
    expect(a, false, {{0, 20, 0, 3, 0}});
    // config 3's sizes (120 steps x 75 levels of 1442 x 1021 -> 64 800 cells) with levels thinning from 10^6 used
    // cells by 12 800 a level (39.5 M in all): 32 steps of all levels exceed 1 GiB, so level-major, and no chunk's
    // packed X goes beyond the cap of four targets.  bo = min(1 GiB / 8 MB = 134, 200 GiB / 8 / (8 000 000 + 518 400)
    // = 3151, 120) = 120: level l is x_l = 960 000 000 - 12 288 000 l bytes of X and 120 * 64 800 * 8 = 62 208 000 of
    // Y, the target 268 435 456.  Levels 0 - 56 exceed the target alone (x_56 = 271 872 000), 57 - 66 by X in pairs
    // (x_66 + x_67 = 285 696 000): one chunk each.  Before Y counted the rest paired by X: {67, 68} 261 120 000,
    // {69, 70} 211 968 000, {71, 72, 73} 225 792 000, {74}: 71 chunks.  With two levels' Y (124 416 000) a pair needs
    // X <= 144 019 456: x_71 + x_72 = 162 816 000 does not, x_72 + x_73 = 138 240 000 does, and a third level
    // (188 928 000 + 186 624 000) does not: 67 - 71 alone, {72, 73}, {74}: 74 chunks.
    {
      Args c3{120, 75, 1, 1442 * 1021, 64800, 8, 8, {}, true, 0, 200 * GiB, 0};
      for (int64_t l = 0; l < 75; ++l) c3.used.push_back(1000000 - 12800 * l);
      const smm::GroupChunkPlan p = plan_of(c3);
      if (!p.pack || p.chunks.size() <= 1) ++gbad;
      for (const smm::GroupChunk& c : p.chunks) gbad += c.x_bytes > 4 * 256 * MiB;
      std::vector<C> want;
      for (int64_t l = 0; l < 72; ++l) want.push_back({0, 120, l, 1, (size_t)(960000000 - 12288000 * l)});
      want.push_back({0, 120, 72, 2, 138240000});
      want.push_back({0, 120, 74, 1, 50688000});
      if (want.size() != 74) ++gbad;
      expect(c3, true, want);
    }
    // ADVICE.md's case: D >= S, one wide level and 24 thin or empty ones, the free memory of a 288-GB card.  S = 100 000,
    // D = 200 000, f64, 64 outer indices; level 0 uses 60 000 cells, level l >= 1 uses (l - 1) % 3 = 0, 1, 2, 0, ... cells
    // (60 024 of 2 500 000: packed).  32 outer indices of all levels are 32 * (480 192 + 25 * 1 600 000) B = 1.3 GB > 1 GiB:
    // level-major.  bo = min(1 GiB / 480 000 = 2236, 256 GiB / 8 / (480 000 + 1 600 000) = 16 519, 64) = 64.  A level
    // is 64 * 200 000 * 8 = 102 400 000 B of Y and U * 512 B of X (level 0: 30 720 000): two levels' Y (204 800 000) fit
    // the 268 435 456 with any of these X, three (307 200 000) never do.  So {0, 1} 30 720 000 + 0, then pairs
    // {2, 3} (1 + 2) * 512 = 1536, {4, 5} 512, {6, 7} 1024, ... repeating, and {24} (U = 2) alone: 13 chunks of at most
    // 235 520 000 B.  Bounded by X alone, all 25 levels made ONE chunk with 2 560 000 000 B of Y, four times over in
    // device and pinned memory.
    {
      Args adv{64, 25, 1, 100000, 200000, 8, 8, {60000}, true, 0, 256 * GiB, 0};
      for (int64_t l = 1; l < 25; ++l) adv.used.push_back((l - 1) % 3);
      expect(adv, true, {{0, 64, 0, 2, 30720000}, {0, 64, 2, 2, 1536}, {0, 64, 4, 2, 512}, {0, 64, 6, 2, 1024},
                         {0, 64, 8, 2, 1536}, {0, 64, 10, 2, 512}, {0, 64, 12, 2, 1024}, {0, 64, 14, 2, 1536},
                         {0, 64, 16, 2, 512}, {0, 64, 18, 2, 1024}, {0, 64, 20, 2, 1536}, {0, 64, 22, 2, 512},
                         {0, 64, 24, 1, 1024}});
      const smm::GroupChunkPlan p = plan_of(adv);
      if (p.max_y > 2 * (size_t)102400000 || p.max_x != 30720000) ++gbad;
    }
    // Seeded sweep: every plan of 3000 drawn calls keeps the invariants of plan_of.  Sizes from a handful of cells to
    // config 3's, D / S from 1 / 64 to 64, 2-, 4- and 8-byte cells, four shapes of used counts (dense; thinning with depth
    // as config 3; one wide level and runs of levels with 0, 1 or 2 used cells; thinning into an all-empty tail), packing
    // allowed or not, a requested chunk size, unknown / little / a card's free memory, the default and small budgets.
    const long long hand_bad = gbad;
    {
      uint64_t state = 0x9e3779b97f4a7c15ull;
      auto next = [&]() {   // splitmix64
        uint64_t z = (state += 0x9e3779b97f4a7c15ull);
        z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
        z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
        return z ^ (z >> 31);
      };
      auto below = [&](uint64_t n) { return (int64_t)(next() % n); };
      const int64_t sizes[] = {16, 288, 5000, 64800, 259200, 1472282, 2000000};
      const int64_t ratio_num[] = {1, 1, 1, 1, 2, 8, 64}, ratio_den[] = {64, 8, 2, 1, 1, 1, 1};
      const size_t cell[] = {2, 4, 8};
      const int64_t requested[] = {0, 0, 0, 1, 7};
      for (int it = 0; it < 3000; ++it) {
        Args a;
        a.n_outer = it % 5 == 0 ? 1 + below(400) : 1 + below(40) * below(11);   // short batches as often as long ones
        a.n_lev = 1 + below(90);
        a.n_inner = 1 + below(3);
        a.S = sizes[below(7)] + below(3);
        const int64_t r = below(7);
        a.D = std::max<int64_t>(1, a.S * ratio_num[r] / ratio_den[r]);
        a.xsz = cell[below(3)];
        a.ysz = cell[below(3)];
        const int64_t pattern = below(4), wide = 1 + below(a.S * 4 / 5);
        for (int64_t l = 0; l < a.n_lev; ++l) {
          int64_t u;
          if (pattern == 0) u = a.S - below(a.S / 4 + 1);                                   // dense: rarely packed
          else if (pattern == 1) u = std::max<int64_t>(0, wide - wide * l / a.n_lev);       // thinning with depth
          else if (pattern == 2) u = l % 23 == 0 ? wide : below(3);                         // wide, then runs of 0, 1, 2
          else u = l < a.n_lev / 3 ? std::max<int64_t>(1, wide - wide * 3 * l / a.n_lev) : 0;   // an all-empty tail
          a.used.push_back(u);
        }
        a.allowed = below(8) != 0;
        a.requested = requested[below(5)];
        const int64_t f = below(4);
        a.free_bytes = f == 0 ? 0 : f == 1 ? (size_t)(1 + below(4096)) << 20 : f == 2 ? 6 * GiB : 256 * GiB;
        const int64_t b = below(3);
        a.budget_kb = b == 0 ? 0 : b == 1 ? 1 + below(512) : 4096 << below(7);
        plan_of(a);
      }
      // the sweep reached what it is for: level-major plans with chunks of several levels, chunks that the Y bound
      // ended, plans that the free memory bounds, whole rows
      if (n_level_major < 300 || n_multi < 1000 || n_y_ended < 300 || n_mem_bound < 10 || n_whole < 300) ++gbad;
    }
    printf("GSWEEPBAD %lld %lld %lld %lld %lld %lld\n", gbad - hand_bad, n_level_major, n_multi, n_y_ended, n_mem_bound, n_whole);
    printf("GCHUNKBAD %lld\n", gbad);
  }
  // exact-zero links dropped: what is left is the same matrix without its zeros
  {
    long long pbad = 0;
    smm::HostCsr pr = csr;
    const int64_t dropped = smm::prune_zero_links(pr);
    int64_t zeros = 0;
    for (double v : csr.val) zeros += v == 0.0;
    if (dropped != zeros || pr.nnz != csr.nnz - zeros || (int64_t)pr.col.size() != pr.nnz || pr.rowptr.back() != pr.nnz) ++pbad;
    int64_t max_row = 0;
    for (int64_t d = 0; d < csr.n_dst; ++d) {
      int64_t k2 = pr.rowptr[(size_t)d];
      for (int64_t k = csr.rowptr[(size_t)d]; k < csr.rowptr[(size_t)d + 1]; ++k) {
        if (csr.val[(size_t)k] == 0.0) continue;
        if (k2 >= pr.rowptr[(size_t)d + 1] || pr.col[(size_t)k2] != csr.col[(size_t)k] || pr.val[(size_t)k2] != csr.val[(size_t)k]) ++pbad;
        ++k2;
      }
      if (k2 != pr.rowptr[(size_t)d + 1]) ++pbad;
      max_row = std::max<int64_t>(max_row, pr.rowptr[(size_t)d + 1] - pr.rowptr[(size_t)d]);
    }
    if (max_row != pr.max_row_nnz) ++pbad;
    printf("PRUNEBAD %lld %lld\n", pbad, (long long)dropped);
  }
  // launch grids beyond the limit: smm::split_batch cuts the (outer x inner) batch into parts that fit, every
  // batch row in exactly one part; a single row that cannot fit is reported, not launched
  {
    long long sbad = 0;
    struct Case { int64_t n_o, n_i, n_dblocks, n_lev, limit; };
    const Case cases[] = {{3600, 1, 254, 1, 0x7fffffffLL}, {3600, 1, 254, 1, 5000}, {120, 7, 1013, 75, 100000},
                          {1, 1000, 64, 3, 999}, {5, 5, 10, 1, 10}, {1, 1, 10, 1, 10}, {17, 3, 49152, 1, 49152}};
    for (const Case& c : cases) {
      // the tile kernel's rule (smm_launch.hpp): walks of 64 rows, halved while the grid stays below 4096
      auto blocks = [&](int64_t n_o, int64_t n_i) {
        const int64_t n_j = n_o * n_i;
        int64_t walk = 64;
        while (walk > 1 && c.n_dblocks * ((n_j + walk - 1) / walk) * c.n_lev < 4096) walk /= 2;
        walk = std::min(walk, n_j);
        return c.n_dblocks * ((n_j + walk - 1) / walk) * c.n_lev;
      };
      std::vector<int> seen((size_t)(c.n_o * c.n_i), 0);
      int64_t parts = 0;
      auto emit = [&](int64_t o0, int64_t n_o, int64_t i0, int64_t n_i) {
        if (blocks(n_o, n_i) > c.limit) ++sbad;
        for (int64_t o = o0; o < o0 + n_o; ++o)
          for (int64_t i = i0; i < i0 + n_i; ++i) ++seen[(size_t)(o * c.n_i + i)];
        ++parts;
        return 0;
      };
      const int rc = smm::split_batch(0, c.n_o, 0, c.n_i, c.limit, blocks, emit);
      const bool one_row_fits = blocks(1, 1) <= c.limit;
      if (rc != (one_row_fits ? 0 : -1)) ++sbad;
      if (one_row_fits)
        for (int v : seen) sbad += v != 1;
      if (c.limit == 0x7fffffffLL && parts != 1) ++sbad;
    }
    // an error of one part stops the walk and is passed on
    int calls = 0;
    if (smm::split_batch(0, 8, 0, 1, 1, [](int64_t a, int64_t b) { return a * b; },
                         [&](int64_t, int64_t, int64_t, int64_t) { return ++calls == 3 ? 7 : 0; }) != 7 || calls != 3)
      ++sbad;
    printf("SPLITBAD %lld\n", sbad);
  }
  // worker pools of the builders: a task that throws (std::bad_alloc from a worker's scratch vectors) must come
  // back as an exception on the calling thread after every started thread has been joined -- never
  // std::terminate --, and a thread that cannot be started costs parallelism, not the result
  {
    long long fbad = 0, thrown = 0;
    auto same_csr = [&](const smm::HostCsr& a) {
      return a.rowptr == csr.rowptr && a.col == csr.col && a.val == csr.val && a.n_used_src == csr.n_used_src;
    };
    smm::debug_builder_faults(true, -1);            // no thread can be started: every task runs on the caller
    {
      smm::HostCsr again;
      std::string e3;
      if (!smm::build_csr(n_src, n_dst, nnz, src.data(), dst.data(), w.data(), again, e3) || !same_csr(again)) ++fbad;
    }
    for (int no_threads = 0; no_threads < 2; ++no_threads) {
      for (int64_t at = 0; at < 40; ++at) {
        smm::debug_builder_faults(no_threads != 0, at);
        try {
          smm::HostCsr again;
          std::string e3;
          smm::HostSell sell2;
          smm::HostTilePlan plan2;
          if (!smm::build_csr(n_src, n_dst, nnz, src.data(), dst.data(), w.data(), again, e3)) ++fbad;
          smm::build_sell(again, sell2);
          smm::build_tile_plan(again, sell2, 256, 16, 512, plan2);
          if (!same_csr(again)) ++fbad;             // the fault counter ran past every task: a clean build
        } catch (const std::bad_alloc&) {
          ++thrown;
        }
      }
    }
    smm::debug_builder_faults(false, -1);
    smm::HostCsr again;
    std::string e3;
    if (!smm::build_csr(n_src, n_dst, nnz, src.data(), dst.data(), w.data(), again, e3) || !same_csr(again)) ++fbad;
    printf("FAULTBAD %lld %lld\n", fbad, thrown);
  }
  // the host pipelines' staging stages on the persistent pool (smm_hostpool.cpp): the pack gives the same block with
  // 1, 3 and 16 threads, plain and non-temporal stores, rows that do not fill a 16-row block; a worker that cannot
  // be started costs parallelism only; a task that throws comes back as a status (1 = bad_alloc) -- never
  // std::terminate -- and the pool is usable afterwards
  {
    long long qbad = 0, statuses = 0;
    const int64_t S = 5003, rows = 83, n_inner = 5, stride_i = S, stride_o = 2 * n_inner * S;   // a level of an (o, 2, 5, S) field
    const int64_t n_o = (rows + n_inner - 1) / n_inner;
    std::vector<double> x((size_t)(n_o * stride_o));
    for (size_t i = 0; i < x.size(); ++i) x[i] = 0.5 * (double)i;
    std::vector<int32_t> used;
    for (int32_t c = 3; c < S; c += 1 + (c % 7)) used.push_back(c);
    const int64_t U = (int64_t)used.size();
    auto entry = [&](int64_t r, int32_t c) { return x[(size_t)((r / n_inner) * stride_o + (r % n_inner) * stride_i + c)]; };
    auto check = [&](const std::vector<double>& out) {
      long long b2 = 0;
      for (int64_t u = 0; u < U; ++u)
        for (int64_t r = 0; r < rows; ++r) b2 += out[(size_t)(u * rows + r)] != entry(r, used[(size_t)u]);
      return b2;
    };
    for (int threads : {1, 3, 16})
      for (int streaming = 0; streaming < 2; ++streaming) {
        smm::set_host_threads(threads);
        std::vector<double> out((size_t)(U * rows), -1.0);
        if (smm::host_pack(out.data(), x.data(), 8, n_inner, stride_o, stride_i, used.data(), U, rows, streaming != 0)) ++qbad;
        qbad += check(out);
      }
    // f32, rows a multiple of 16 so that the streaming path is taken for every block
    {
      std::vector<float> xf(x.begin(), x.end()), outf((size_t)(U * 96), -1.f);
      std::vector<float> xrows((size_t)(96 * S));
      for (size_t i = 0; i < xrows.size(); ++i) xrows[i] = (float)(i % 100003);
      smm::set_host_threads(4);
      if (smm::host_pack(outf.data(), xrows.data(), 4, 96, 0, S, used.data(), U, 96, true)) ++qbad;
      for (int64_t u = 0; u < U; ++u)
        for (int64_t r = 0; r < 96; ++r) qbad += outf[(size_t)(u * 96 + r)] != xrows[(size_t)(r * S + used[(size_t)u])];
    }
    // big enough for the pool to be used: 1500 x 5003 doubles packed (> 4 MiB), and a 64-MiB copy
    const int64_t big_rows = 1504;
    std::vector<double> xb((size_t)(big_rows * S));
    for (size_t i = 0; i < xb.size(); ++i) xb[i] = (double)(i % 1000003);
    std::vector<double> outb((size_t)(U * big_rows));
    auto pack_big = [&]() { return smm::host_pack(outb.data(), xb.data(), 8, big_rows, 0, S, used.data(), U, big_rows, true); };
    auto big_ok = [&]() {
      long long b2 = 0;
      for (int64_t u = 0; u < U; u += 17)
        for (int64_t r = 0; r < big_rows; r += 5) b2 += outb[(size_t)(u * big_rows + r)] != xb[(size_t)(r * S + used[(size_t)u])];
      return b2;
    };
    smm::set_host_threads(6);
    if (pack_big() || big_ok()) ++qbad;
    const int workers_after_first = smm::pool_workers();
    if (pack_big() || smm::pool_workers() != workers_after_first) ++qbad;       // persistent: no new threads per call
    std::vector<char> ca((size_t)64 << 20), cb((size_t)64 << 20, 0);
    for (size_t i = 0; i < ca.size(); i += 4099) ca[i] = (char)(i * 31);
    if (smm::host_copy(cb.data(), ca.data(), ca.size()) || memcmp(ca.data(), cb.data(), ca.size()) != 0) ++qbad;
    // no worker can be started: the caller does everything, same block
    smm::debug_pool_faults(true, -1);
    std::fill(outb.begin(), outb.end(), -1.0);
    if (pack_big() || big_ok()) ++qbad;
    // a task throws: status 1, no terminate, with and without workers; then a clean run
    for (int no_threads = 0; no_threads < 2; ++no_threads)
      for (int64_t at = 0; at < 12; ++at) {
        smm::debug_pool_faults(no_threads != 0, at);
        const int rc = pack_big();
        if (rc == 1) ++statuses;
        else if (rc != 0) ++qbad;
      }
    smm::debug_pool_faults(false, -1);
    std::fill(outb.begin(), outb.end(), -1.0);
    if (pack_big() || big_ok()) ++qbad;
    smm::set_host_threads(argc > 1 ? atoi(argv[1]) : 0);
    printf("POOLBAD %lld %lld %d %d\n", qbad, statuses, workers_after_first, smm::usable_cpus());
  }
  printf("SELLBAD %lld\n", bad);
  return 0;
}
