// GRIB simple-packed fields shipped raw: the host side of smm_apply_grib(_bm), smm_apply_host_grib(_bm),
// smm_group_apply_grib and smm_group_apply_host_grib, and of their four SMM_APPLY_SKIPNA twins (_na); and the way back,
// float64 results into GRIB simple packing: smm_grib_out_layout, smm_grib_pack, smm_apply_host_grib_pk and
// smm_group_apply_host_grib_pk (kernels: smm_grib_pack.hip).  The kernels and their launchers are in smm_grib.hip; what
// needs no device -- the refusals of a row table, the chunk plan and the layout of a staged chunk -- in
// smm_grib_plan.cpp.  An operator and a group differ in how a launch grid is cut into parts and in where Y goes;
// everything else is written once.
#include "smm_device.hpp"

namespace {

// Everything the entries refuse before the handle is looked at and before any device is touched.  na: a _na entry -- on
// return *flags_io carries SMM_APPLY_SKIPNA, which those entries imply (so SMM_APPLY_NO_FILL is check_flags' refusal) and
// the others refuse.
int check_grib_call(const void* x, bool x_device, int64_t x_bytes, const smm_grib_row_t* rows, const void* y, int y_dtype,
                    int64_t n_batch, double area_min, unsigned* flags_io, bool na) {
  if (na) *flags_io |= SMM_APPLY_SKIPNA;
  const unsigned flags = *flags_io;
  if (int frc = check_flags(flags)) return frc;
  if (flags & ~(unsigned)(SMM_APPLY_MASKED | SMM_APPLY_NO_FILL | SMM_APPLY_KERNEL_SELL | (na ? SMM_APPLY_SKIPNA : 0u)))
    return fail(SMM_ERR_UNSUPPORTED, std::string("GRIB fields run the SELL kernel on whole rows: ") +
                                         (na ? "" : "SMM_APPLY_SKIPNA, ") + "SMM_APPLY_KERNEL_TILE "
                                         "and the batch-fastest / host-pack flags are not built for them");
  if (y_dtype != SMM_F64) return fail(SMM_ERR_UNSUPPORTED, "GRIB fields produce SMM_F64 results");
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (x_bytes < 0) return fail(SMM_ERR_INVALID, "negative x_bytes");
  if ((!x && x_bytes > 0) || !y || (!rows && n_batch > 0)) return fail(SMM_ERR_INVALID, "null field, result or row-table pointer");
  if (x_device && (uintptr_t)x % 4) return fail(SMM_ERR_INVALID, "field pointer is not 4-byte aligned");
  if ((uintptr_t)y % 8) return fail(SMM_ERR_INVALID, "result pointer is not element aligned");
  if (int arc = check_area_min(area_min)) return arc;
  std::string err;
  if (!smm::check_grib_rules(rows, n_batch, err)) return fail(SMM_ERR_INVALID, err);
  return SMM_OK;
}
// ... and what needs the operator's sizes
int check_grib_operator(smm_operator_t op, int64_t x_bytes, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                        int64_t ldy, int64_t n_batch, double area_min, unsigned flags) {
  if (!op) return fail(SMM_ERR_INVALID, "null operator");
  if (n_batch > 0 && ldy < op->csr.n_dst) return fail(SMM_ERR_INVALID, "ldy smaller than the grid size");
  std::string err;
  if (!smm::check_grib_ranges(rows, bitmaps, n_batch, op->csr.n_src, x_bytes, err)) return fail(SMM_ERR_INVALID, err);
  return check_epilogue(op, flags & SMM_APPLY_MASKED, area_min, "the operator");
}
// ... or the group: the group itself, its level_index, where the rows lie in the buffer (the members share n_src) and
// each used member's epilogue
int check_grib_group(smm_group_t g, int64_t x_bytes, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                     int64_t n_rows, int64_t n_lev, const int32_t* level_index, const uint8_t* masked_levels, double area_min,
                     unsigned flags) {
  if (!g) return fail(SMM_ERR_INVALID, "null group");
  if (int rc = check_levels(g, n_lev, level_index, masked_levels, 0.0, 0u)) return rc;   // level_index alone
  std::string err;
  if (!smm::check_grib_ranges(rows, bitmaps, n_rows, g->ops[0]->csr.n_src, x_bytes, err)) return fail(SMM_ERR_INVALID, err);
  return check_levels(g, n_lev, level_index, masked_levels, area_min, flags);
}
// rows of a group call, or -1 when a count is negative (check_grib_call refuses it in its place)
int64_t grib_group_rows(int64_t n_outer, int64_t n_lev, int64_t n_inner) {
  return (n_outer < 0 || n_lev < 0 || n_inner < 0) ? -1 : n_outer * n_lev * n_inner;
}
bool grib_needs_division(const smm_grib_row_t* rows, int64_t n_batch) {
  for (int64_t b = 0; b < n_batch; ++b)
    if (rows[b].ddiv != 1.0) return true;
  return false;
}

// What a launch reads on the device: the buffers of a device-entry call, or one chunk's in its pipeline slot.
struct GribIn {
  const void* x;                 // the packed bytes, 4-byte aligned, x_bytes of them
  int64_t x_bytes;
  const smm_grib_row_t* rows;    // the row table
  const GribRowBitmap* bm;       // the rows' bitmap records (read when n_tables > 0)
  char* rank;                    // room for n_tables rank tables of ceil(n_src / 32) entries and, behind them, n_tables x
  size_t n_tables;               // segments totals; n_tables: the bitmapped rows -- 0: the plain gather runs
  bool div;                      // some row has ddiv != 1.0 (grib_needs_division)
};

// What every GRIB launch fills into the GribArgs base.  *with_tables: the gather consults rank tables -- then the tables
// of the n_rows rows' bitmaps are built here first, on the same stream (launch_grib_build).
int grib_launch_base(GribArgs& a, bool* with_tables, const GribIn& in, const LevelDesc* descs, int64_t n_src, int64_t n_dst,
                     int64_t n_rows, double area_min, unsigned flags, hipStream_t s) {
  a.descs = descs;
  // no data bytes at all (every row has 0 bits): the loads, clamped to word 0, read the table instead
  a.x = in.x_bytes > 0 ? (const uint32_t*)in.x : (const uint32_t*)in.rows;
  a.last_word = in.x_bytes > 0 ? smm_grib::align4((uint64_t)in.x_bytes) / 4 - 1 : 0;
  a.n_dst = n_dst;
  a.n_dblocks = ((n_dst + 63) / 64 + kWavesPerBlock - 1) / kWavesPerBlock;
  a.area_min = area_min;
  a.masked = (flags & SMM_APPLY_MASKED) ? 1 : 0;
  const uint64_t n_blocks = smm_grib::bitmap_blocks((uint64_t)n_src);
  *with_tables = in.bm && in.n_tables > 0 && n_blocks > 0;
  if (!*with_tables) return SMM_OK;
  GribBuildArgs b{};
  b.x = a.x;
  b.bm = in.bm;
  b.table = (smm_grib::GribRankEntry*)in.rank;
  b.totals = (uint32_t*)(in.rank + in.n_tables * (size_t)n_blocks * sizeof(smm_grib::GribRankEntry));
  b.last_word = a.last_word;
  b.n_j = n_rows;
  b.n_src = (uint32_t)n_src;
  b.n_blocks = (uint32_t)n_blocks;
  b.n_segs = (uint32_t)smm_grib::bitmap_segments((uint64_t)n_src);
  return smm_launch::launch_grib_build(b, s);
}

// n_batch rows of an operator: one launch, or parts of the batch when the grid would pass the limit (smm::split_batch, as
// run_apply)
int launch_grib_rows(smm_operator_t op, const GribIn& in, void* y, int64_t ldy, int64_t n_batch, double area_min,
                     unsigned flags, hipStream_t s) {
  GribArgs a{};
  bool with_tables = false;
  if (int rc = grib_launch_base(a, &with_tables, in, op->d_desc.get(), op->csr.n_src, op->csr.n_dst, n_batch, area_min, flags, s))
    return rc;
  a.ldy = ldy;
  const bool fill = !(flags & SMM_APPLY_NO_FILL), na = (flags & SMM_APPLY_SKIPNA) != 0;
  auto blocks_for = [&](int64_t n_o, int64_t) -> int64_t {
    const int bt = smm_launch::sell_batch_rows(n_o);
    return a.n_dblocks * ((n_o + bt - 1) / bt);
  };
  auto launch_part = [&](int64_t o0, int64_t n_o, int64_t, int64_t) -> int {
    GribBitmapArgs p{};
    static_cast<GribArgs&>(p) = a;
    p.rows = in.rows + o0;
    p.y = (double*)y + o0 * ldy;
    p.n_j = n_o;
    if (!with_tables) return smm_launch::launch_grib(p, in.div, na, fill, s);
    p.bm = in.bm + o0;
    p.table = (const smm_grib::GribRankEntry*)in.rank;
    return smm_launch::launch_grib_bitmap(p, in.div, na, fill, s);
  };
  const int rc = smm::split_batch(0, n_batch, 0, 1, grid_limit(), blocks_for, launch_part);
  if (rc == -1)
    return fail(SMM_ERR_INVALID, "one batch row alone needs a launch grid beyond " + std::to_string(grid_limit()) +
                                     " workgroups (destination blocks)");
  return rc;
}

// The rows of (n_outer, n_lev, n_inner) of a group -- record (o * n_lev + l) * n_inner + i of in.rows / in.bm -- all levels
// in one launch.  A grid beyond the limit is cut over the outer and the inner range (smm::split_batch, as run_apply); a
// single batch row whose levels still do not fit is cut over the levels.
int launch_grib_group_rows(smm_group_t g, const int32_t* d_map, const uint8_t* d_masked, const GribIn& in, void* y, int64_t ys_o,
                           int64_t ys_l, int64_t ys_i, int64_t n_outer, int64_t n_lev, int64_t n_inner, double area_min,
                           unsigned flags, hipStream_t s) {
  GribGroupArgs a{};
  bool with_tables = false;
  if (int rc = grib_launch_base(a, &with_tables, in, g->d_descs.get(), g->ops[0]->csr.n_src, g->ops[0]->csr.n_dst,
                                n_outer * n_lev * n_inner, area_min, flags, s))
    return rc;
  a.lev_masked = d_masked;
  a.rec_o = n_lev * n_inner;
  a.rec_l = n_inner;
  a.ys_o = ys_o;
  a.ys_l = ys_l;
  a.ys_i = ys_i;
  const bool fill = !(flags & SMM_APPLY_NO_FILL), na = (flags & SMM_APPLY_SKIPNA) != 0;
  const int64_t limit = grid_limit();
  // the kernel's row indices inside a level are 32-bit: a part of 2^31 rows or more per level counts as too large
  auto blocks_for = [&](int64_t n_o, int64_t n_i, int64_t n_l) -> int64_t {
    const int64_t n_j = n_o * n_i;
    if (n_j > 0x7fffffffLL) return limit + 1;
    const int bt = smm_launch::sell_batch_rows(n_j);
    return a.n_dblocks * ((n_j + bt - 1) / bt) * n_l;
  };
  auto launch_part = [&](int64_t o0, int64_t n_o, int64_t i0, int64_t n_i, int64_t l0, int64_t n_l) -> int {
    GribGroupArgs p = a;
    const int64_t first = (o0 * n_lev + l0) * n_inner + i0;
    p.rows = in.rows + first;
    p.lev_map = d_map + l0;
    p.y = (double*)y + (o0 * ys_o + l0 * ys_l + i0 * ys_i);
    p.n_j = n_o * n_i;
    p.n_inner = n_i;
    if (with_tables) {
      p.bm = in.bm + first;
      p.table = (const smm_grib::GribRankEntry*)in.rank;
    }
    return smm_launch::launch_grib_group(p, n_l, with_tables, in.div, na, fill, s);
  };
  // a part of several rows is cut further while it does not fit; a single row goes to the level split whatever it needs
  const int rc = smm::split_batch(
      0, n_outer, 0, n_inner, limit,
      [&](int64_t n_o, int64_t n_i) -> int64_t { return n_o * n_i == 1 ? 0 : blocks_for(n_o, n_i, n_lev); },
      [&](int64_t o0, int64_t n_o, int64_t i0, int64_t n_i) -> int {
        return smm::split_batch(
            0, n_lev, 0, 1, limit, [&](int64_t n_l, int64_t) { return blocks_for(n_o, n_i, n_l); },
            [&](int64_t l0, int64_t n_l, int64_t, int64_t) { return launch_part(o0, n_o, i0, n_i, l0, n_l); });
      });
  if (rc == -1)
    return fail(SMM_ERR_INVALID, "one batch row of one level alone needs a launch grid beyond " + std::to_string(limit) +
                                     " workgroups (destination blocks)");
  return rc;
}

// ---- the device entries

// The host tables of a device-entry call into the buffers its handle keeps for them (gs, under gs.mu): the row table, and
// when some row has a bitmap the bitmap records, with the rank buffer sized for the tables.  Fills in.rows / bm / rank /
// n_tables.
int upload_grib_tables(GribState& gs, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_batch,
                       int64_t n_src, hipStream_t s, GribIn& in) {
  if (gs.d_rows.bytes() < (size_t)n_batch * sizeof(smm_grib_row_t)) {
    // freeing the old table waits for the device: no kernel still reads it
    const size_t have = gs.d_rows.bytes() / sizeof(smm_grib_row_t);
    SMM_HIP(gs.d_rows.alloc(std::max<size_t>((size_t)n_batch, 2 * have)));
  }
  // `rows` may be reused on return: from pageable memory the runtime has taken the bytes when hipMemcpyAsync returns,
  // from page-locked memory it has not -- such a table goes through a pageable copy first.  The copy itself is ordered
  // on the stream behind the kernel of an earlier call that still reads the device table.
  std::vector<smm_grib_row_t> pageable;
  if (is_pinned(rows)) {
    pageable.assign(rows, rows + n_batch);
    rows = pageable.data();
  }
  SMM_HIP(hipMemcpyAsync(gs.d_rows.get(), rows, (size_t)n_batch * sizeof(smm_grib_row_t), hipMemcpyHostToDevice, s));
  // the bitmap records go up beside it, each bitmapped row with the place of its rank table; a pageable vector in any
  // case.  Only bitmapped rows take table space; a call without one runs the plain gather.
  std::vector<GribRowBitmap> bm;
  size_t n_tables = 0, rank_bytes = 0;
  if (bitmaps) {
    const uint64_t n_blocks = smm_grib::bitmap_blocks((uint64_t)n_src);
    bm.resize((size_t)n_batch);
    for (int64_t b = 0; b < n_batch; ++b) {
      const smm::GribRowCost c = smm::grib_row_cost(rows[b], &bitmaps[b], n_src);
      bm[(size_t)b] = GribRowBitmap{bitmaps[b].bitmap_off, c.has_bitmap ? n_tables * n_blocks : 0};
      n_tables += c.has_bitmap;
      rank_bytes += c.rank;
    }
  }
  if (n_tables > 0) {
    if (gs.d_bm.bytes() < bm.size() * sizeof(GribRowBitmap)) {
      const size_t have = gs.d_bm.bytes() / sizeof(GribRowBitmap);
      SMM_HIP(gs.d_bm.alloc(std::max<size_t>(bm.size(), 2 * have)));
    }
    if (gs.d_rank.bytes() < rank_bytes) SMM_HIP(gs.d_rank.alloc(std::max(rank_bytes, 2 * gs.d_rank.bytes())));
    SMM_HIP(hipMemcpyAsync(gs.d_bm.get(), bm.data(), bm.size() * sizeof(GribRowBitmap), hipMemcpyHostToDevice, s));
  }
  in.rows = gs.d_rows.get();
  in.bm = gs.d_bm.get();
  in.rank = gs.d_rank.get();
  in.n_tables = n_tables;
  return SMM_OK;
}

// bitmaps: null, or the records of smm_apply_grib_bm
int smm_apply_grib_impl(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                        const smm_grib_bitmap_t* bitmaps, void* y, int64_t ldy, int64_t n_batch, double area_min, unsigned flags,
                        void* stream) {
  if (n_batch == 0 || op->csr.n_dst == 0) return SMM_OK;
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(op->grib.mu);
  GribIn in{x, x_bytes, nullptr, nullptr, nullptr, 0, grib_needs_division(rows, n_batch)};
  if (int rc = upload_grib_tables(op->grib, rows, bitmaps, n_batch, op->csr.n_src, s, in)) return rc;
  return launch_grib_rows(op, in, y, ldy, n_batch, area_min, flags, s);
}

int smm_group_apply_grib_impl(smm_group_t g, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                              const smm_grib_bitmap_t* bitmaps, void* y, int64_t ys_o, int64_t ys_l, int64_t ys_i, int64_t n_outer,
                              int64_t n_lev, int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                              double area_min, unsigned flags, void* stream) {
  const int64_t n_rows = n_outer * n_lev * n_inner;
  if (n_rows == 0 || g->ops[0]->csr.n_dst == 0) return SMM_OK;
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  const int32_t* d_map;
  const uint8_t* d_masked;
  if (int rc = group_level_cfg(g, n_lev, level_index, masked_levels, area_min, flags, &d_map, &d_masked)) return rc;
  hipStream_t s = (hipStream_t)stream;
  std::lock_guard<std::mutex> lock(g->grib.mu);
  GribIn in{x, x_bytes, nullptr, nullptr, nullptr, 0, grib_needs_division(rows, n_rows)};
  if (int rc = upload_grib_tables(g->grib, rows, bitmaps, n_rows, g->ops[0]->csr.n_src, s, in)) return rc;
  return launch_grib_group_rows(g, d_map, d_masked, in, y, ys_o, ys_l, ys_i, n_outer, n_lev, n_inner, area_min, flags, s);
}

// ---- the host entries

// Staging of a chunk (rows [ch.r0, ch.r0 + ch.nr) of the call) into the pinned buffer hx: smm::layout_grib_chunk writes
// the table and the bitmap records and so says where every piece goes; each row's data bytes and, with a bitmap, its own
// copy of its bitmap are copied there.  A pinned x_host is staged all the same: the rows of a chunk need not be adjacent
// in it.  *n_tables: the bitmapped rows of the chunk.
int stage_grib_chunk(char* hx, const smm::GribChunk& ch, const void* x_host, const smm_grib_row_t* rows,
                     const smm_grib_bitmap_t* bitmaps, int64_t S, size_t* n_tables) {
  *n_tables = smm::layout_grib_chunk(hx, ch, rows, bitmaps, S).n_tables;
  const smm_grib_row_t* table = (const smm_grib_row_t*)hx;
  const GribRowBitmap* bm = (const GribRowBitmap*)(hx + (size_t)ch.nr * sizeof(smm_grib_row_t));
  for (int64_t r = 0; r < ch.nr; ++r) {   // each row's copy is spread over the staging pool (host_copy)
    const int64_t b = ch.r0 + r;
    const smm::GribRowCost c = smm::grib_row_cost(rows[b], bitmaps ? &bitmaps[b] : nullptr, S);
    if (int rc = host_copy(hx + table[r].byte_off, (const char*)x_host + rows[b].byte_off, c.data_bytes)) return rc;
    if (c.has_bitmap)
      if (int rc = host_copy(hx + bm[r].bitmap_off, (const char*)x_host + bitmaps[b].bitmap_off, c.bitmap_bytes)) return rc;
  }
  return SMM_OK;
}

// ---- results packed back into GRIB (smm_grib_pack, smm_apply_host_grib_pk)

// Where the packed result of a host call goes: offs[b] = row b's slot in out_host (n_batch + 1 entries, the last the total)
struct GribOut {
  const smm_grib_encode_t* enc;
  const uint64_t* offs;
  char* out_host;
  smm_grib_row_t* rows_out;
  smm_grib_bitmap_t* bitmaps_out;
};

// The pack tables of nr rows into t (nr GribPackRow, then nr GribRowBitmap for the rank-table build: every row has a
// bitmap there, table r).  The rows' slots lie back to back from slot_base of the device buffer; offs[r] is where the
// caller sees row r's slot.  Returns the stream words of the widest row.
uint32_t fill_pack_tables(char* t, const smm_grib_encode_t* enc, int64_t nr, int64_t D, size_t slot_base, const uint64_t* offs) {
  GribPackRow* rows = (GribPackRow*)t;
  GribRowBitmap* bm = (GribRowBitmap*)(t + (size_t)nr * sizeof(GribPackRow));
  const uint64_t n_blocks = smm_grib::bitmap_blocks((uint64_t)D);
  uint32_t max_words = 0;
  for (int64_t r = 0; r < nr; ++r) {
    const uint64_t slot = slot_base + (offs[r] - offs[0]);
    rows[r] = GribPackRow{enc[r].ddiv, slot, offs[r], enc[r].nbits, 0};
    bm[r] = GribRowBitmap{slot, (uint64_t)r * n_blocks};
    max_words = std::max(max_words, (uint32_t)(smm_grib::align4(smm_grib::row_bytes((uint64_t)D, enc[r].nbits)) / 4));
  }
  return max_words;
}
// What each of n_rows rows' packed result takes on the device beside its Y (smm::plan_grib_chunks' out_row_bytes): its
// slot, its records, its pack tables and one row's scratch.  Empty without pk.
std::vector<size_t> grib_out_row_bytes(const GribOut* pk, int64_t n_rows, int64_t D) {
  std::vector<size_t> out_row;
  if (!pk) return out_row;
  const size_t scratch = smm::grib_pack_scratch(D, 1).bytes;
  for (int64_t b = 0; b < n_rows; ++b)
    out_row.push_back((size_t)(pk->offs[b + 1] - pk->offs[b]) + smm::kGribOutRecordBytes + smm::kGribPackTableBytes + scratch);
  return out_row;
}
static_assert(sizeof(GribPackRow) + sizeof(GribRowBitmap) == smm::kGribPackTableBytes, "the pack tables of a row");
static_assert(sizeof(smm_grib_row_t) + sizeof(smm_grib_bitmap_t) == smm::kGribOutRecordBytes, "the records of a row");

// The four pack steps on stream s: nr rows of D cells of the device result y into d_out (out_bytes of it hold the slots,
// a multiple of 4), the records into d_recs (nr smm_grib_row_t, then nr smm_grib_bitmap_t); d_tables: fill_pack_tables
// on the device; scratch: smm::grib_pack_scratch(D, nr) bytes.
int launch_pack(int64_t D, int64_t nr, const double* y, int64_t ldy, const char* d_tables, char* d_out, size_t out_bytes,
                char* d_recs, char* scratch, uint32_t max_words, hipStream_t s) {
  const smm::GribPackScratch sc = smm::grib_pack_scratch(D, nr);
  GribPackArgs a{};
  a.y = y;
  a.ldy = ldy;
  a.n_j = nr;
  a.n_dst = (uint32_t)D;
  a.n_blocks = (uint32_t)smm_grib::bitmap_blocks((uint64_t)D);
  a.n_segs = (uint32_t)smm_grib::bitmap_segments((uint64_t)D);
  a.max_words = max_words;
  a.rows = (const GribPackRow*)d_tables;
  a.out = (uint32_t*)d_out;
  a.part_min = (double*)(scratch + sc.part_min);
  a.part_max = (double*)(scratch + sc.part_max);
  a.part_cnt = (uint32_t*)(scratch + sc.part_cnt);
  a.rules = (smm_grib::GribPackRule*)(scratch + sc.rules);
  a.rec_rows = (smm_grib_row_t*)d_recs;
  a.rec_bm = (smm_grib_bitmap_t*)(d_recs + (size_t)nr * sizeof(smm_grib_row_t));
  a.table = (const smm_grib::GribRankEntry*)(scratch + sc.table);
  GribBuildArgs b{};
  b.x = (const uint32_t*)d_out;
  b.bm = (const GribRowBitmap*)(d_tables + (size_t)nr * sizeof(GribPackRow));
  b.table = (smm_grib::GribRankEntry*)(scratch + sc.table);
  b.totals = (uint32_t*)(scratch + sc.totals);
  b.last_word = out_bytes / 4 - 1;
  b.n_j = nr;
  b.n_src = a.n_dst;
  b.n_blocks = a.n_blocks;
  b.n_segs = a.n_segs;
  return smm_launch::launch_grib_pack(a, b, grid_limit(), s);
}

// A chunk plan of host rows through a handle's pipeline (the caller holds its pipe_mu; gs: the handle's, for the slots'
// rank buffers).  Per chunk: stage, H2D, launch_chunk(in, ch, dy, stream) -- the chunk's launch from its slot's device
// buffers, Y into dy -- then Y to the host: y_to_host(ch, src, async, stream) copies the chunk's results from src to
// their place in the caller's Y, from the slot's device buffer on the stream when Y is page-locked (y_direct), else from
// the slot's pinned buffer once the chunk has drained.  div: grib_needs_division of the whole call.
// pk (smm_apply_host_grib_pk, smm_group_apply_host_grib_pk), or null: the chunk's Y -- launch_chunk writes it as
// (ch.nr, D), its rows in record order -- stays in the slot's device buffer and is packed there, on the chunk's stream,
// into the slot's packed buffer -- the chunk's row and bitmap records, then its slots.  The pack tables of the chunk
// ride behind its staged X (8-byte aligned).  y_direct then says that pk->out_host is page-locked: the slots go there
// straight from the device and only the records pass through the pinned buffer; else both come back in one copy and
// the slots are copied out once the chunk has drained.  y_to_host is not called.
template <typename Launch, typename YToHost>
int run_grib_pipeline(HostPipe& pipe, GribState& gs, const smm::GribChunkPlan& plan, const void* x_host,
                      const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t S, int64_t D, bool div, bool y_direct,
                      Launch&& launch_chunk, YToHost&& y_to_host, const GribOut* pk = nullptr) {
  const size_t y_chunk = (size_t)plan.max_rows * D * 8;
  auto align8 = [](size_t v) { return (v + 7) & ~(size_t)7; };
  auto rec_bytes = [](const smm::GribChunk& ch) { return (size_t)ch.nr * smm::kGribOutRecordBytes; };
  auto slot_bytes = [&](const smm::GribChunk& ch) { return (size_t)(pk->offs[ch.r0 + ch.nr] - pk->offs[ch.r0]); };
  if (!pk) {
    SMM_HIP(pipe.ensure(plan.max_x, y_chunk, plan.max_x, y_direct ? 0 : y_chunk));
  } else {
    size_t max_pk = 0;
    for (const smm::GribChunk& ch : plan.chunks) max_pk = std::max(max_pk, rec_bytes(ch) + slot_bytes(ch));
    const size_t x_all = align8(plan.max_x) + (size_t)plan.max_rows * smm::kGribPackTableBytes;
    SMM_HIP(pipe.ensure(x_all, y_chunk, x_all, y_direct ? (size_t)plan.max_rows * smm::kGribOutRecordBytes : max_pk));
    const size_t scratch = smm::grib_pack_scratch(D, plan.max_rows).bytes;
    if (max_pk > std::min(gs.d_pipe_pk[0].bytes(), gs.d_pipe_pk[1].bytes()))
      for (int i = 0; i < 2; ++i) SMM_HIP(gs.d_pipe_pk[i].alloc(max_pk));
    if (scratch > std::min(gs.d_pipe_scratch[0].bytes(), gs.d_pipe_scratch[1].bytes()))
      for (int i = 0; i < 2; ++i) SMM_HIP(gs.d_pipe_scratch[i].alloc(scratch));
  }
  if (plan.max_rank > std::min(gs.d_pipe_rank[0].bytes(), gs.d_pipe_rank[1].bytes()))   // device-only, one per slot
    for (int i = 0; i < 2; ++i) SMM_HIP(gs.d_pipe_rank[i].alloc(plan.max_rank));

  CallStats st;
  auto deliver = [&](int64_t c, int b) -> int {   // results of chunk c: pinned -> the caller's Y
    if (pk) {
      const smm::GribChunk& ch = plan.chunks[(size_t)c];
      StageTimer t(st.v[SMM_HOST_STAT_COPY_OUT_MS]);
      const char* h = (const char*)pipe.hy[b].get();
      memcpy(pk->rows_out + ch.r0, h, (size_t)ch.nr * sizeof(smm_grib_row_t));
      memcpy(pk->bitmaps_out + ch.r0, h + (size_t)ch.nr * sizeof(smm_grib_row_t), (size_t)ch.nr * sizeof(smm_grib_bitmap_t));
      if (y_direct) return SMM_OK;
      return host_copy(pk->out_host + pk->offs[ch.r0], h + rec_bytes(ch), slot_bytes(ch));
    }
    if (y_direct) return SMM_OK;
    StageTimer t(st.v[SMM_HOST_STAT_COPY_OUT_MS]);
    return y_to_host(plan.chunks[(size_t)c], (const char*)pipe.hy[b].get(), false, nullptr);
  };
  auto launch = [&](int64_t c, int b) -> int {
    const smm::GribChunk& ch = plan.chunks[(size_t)c];
    char* hx = (char*)pipe.hx[b].get();
    char* dx = pipe.dx[b].get();
    size_t n_tables = 0;
    {
      StageTimer t(st.v[SMM_HOST_STAT_STAGE_IN_MS]);
      if (int rc = stage_grib_chunk(hx, ch, x_host, rows, bitmaps, S, &n_tables)) return rc;
    }
    size_t h2d = ch.x_bytes;
    uint32_t max_words = 0;
    if (pk) {   // the chunk's pack tables behind its X
      h2d = align8(ch.x_bytes);
      max_words = fill_pack_tables(hx + h2d, pk->enc + ch.r0, ch.nr, D, rec_bytes(ch), pk->offs + ch.r0);
      h2d += (size_t)ch.nr * smm::kGribPackTableBytes;
    }
    SMM_HIP(pipe.mark(b, 0));
    SMM_HIP(hipMemcpyAsync(dx, hx, h2d, hipMemcpyHostToDevice, pipe.stream[b]));
    st.v[SMM_HOST_STAT_H2D_BYTES] += (double)h2d;
    SMM_HIP(pipe.mark(b, 1));
    const GribIn in{dx, (int64_t)ch.x_bytes, (const smm_grib_row_t*)dx,
                    bitmaps ? (const GribRowBitmap*)(dx + (size_t)ch.nr * sizeof(smm_grib_row_t)) : nullptr,
                    gs.d_pipe_rank[b].get(), n_tables, div};
    if (int rc = launch_chunk(in, ch, pipe.dy[b].get(), pipe.stream[b])) return rc;
    if (pk) {
      char* dpk = gs.d_pipe_pk[b].get();
      const size_t recs = rec_bytes(ch), slots = slot_bytes(ch);
      if (int rc = launch_pack(D, ch.nr, (const double*)pipe.dy[b].get(), D, dx + align8(ch.x_bytes), dpk, recs + slots, dpk,
                               gs.d_pipe_scratch[b].get(), max_words, pipe.stream[b]))
        return rc;
      st.v[SMM_HOST_STAT_D2H_BYTES] += (double)(recs + slots);
      SMM_HIP(pipe.mark(b, 2));
      if (y_direct) {
        SMM_HIP(hipMemcpyAsync(pk->out_host + pk->offs[ch.r0], dpk + recs, slots, hipMemcpyDeviceToHost, pipe.stream[b]));
        SMM_HIP(hipMemcpyAsync(pipe.hy[b].get(), dpk, recs, hipMemcpyDeviceToHost, pipe.stream[b]));
      } else {
        SMM_HIP(hipMemcpyAsync(pipe.hy[b].get(), dpk, recs + slots, hipMemcpyDeviceToHost, pipe.stream[b]));
      }
      SMM_HIP(pipe.mark(b, 3));
      return SMM_OK;
    }
    st.v[SMM_HOST_STAT_D2H_BYTES] += (double)((size_t)ch.nr * D * 8);
    SMM_HIP(pipe.mark(b, 2));
    if (!y_direct) {
      SMM_HIP(hipMemcpyAsync(pipe.hy[b].get(), pipe.dy[b].get(), (size_t)ch.nr * D * 8, hipMemcpyDeviceToHost, pipe.stream[b]));
    } else if (int rc = y_to_host(ch, (const char*)pipe.dy[b].get(), true, pipe.stream[b])) {
      return rc;
    }
    SMM_HIP(pipe.mark(b, 3));
    return SMM_OK;
  };
  return run_host_pipeline(pipe, (int64_t)plan.chunks.size(), st, launch, deliver);
}

// Host buffers, an operator: chunks of consecutive rows, sized by their bytes (rows differ in width: smm::plan_grib_chunks
// with units of one row); Y is (n_batch, ldy).
int smm_apply_host_grib_impl(smm_operator_t op, const void* x_host, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                             void* y_host, int64_t ldy, int64_t n_batch, double area_min, unsigned flags, int64_t chunk_rows,
                             const GribOut* pk = nullptr) {
  const int64_t S = op->csr.n_src, D = op->csr.n_dst;
  if (n_batch == 0 || D == 0) return SMM_OK;
  DeviceGuard guard(op->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the operator's device");
  const std::vector<size_t> out_row = grib_out_row_bytes(pk, n_batch, D);
  const smm::GribChunkPlan plan = smm::plan_grib_chunks(rows, bitmaps, n_batch, 1, S, D, chunk_rows, free_device_bytes(),
                                                        pk ? out_row.data() : nullptr);
  const size_t yrow = (size_t)ldy * 8;
  auto launch_chunk = [&](const GribIn& in, const smm::GribChunk& ch, void* dy, hipStream_t s) -> int {
    return launch_grib_rows(op, in, dy, D, ch.nr, area_min, flags, s);
  };
  auto y_to_host = [&](const smm::GribChunk& ch, const char* src, bool async, hipStream_t s) -> int {
    char* dst = (char*)y_host + (size_t)ch.r0 * yrow;
    if (async) {
      SMM_HIP(hipMemcpy2DAsync(dst, yrow, src, (size_t)D * 8, (size_t)D * 8, (size_t)ch.nr, hipMemcpyDeviceToHost, s));
      return SMM_OK;
    }
    if (ldy == D) return host_copy(dst, src, (size_t)ch.nr * D * 8);
    for (int64_t r = 0; r < ch.nr; ++r) memcpy(dst + (size_t)r * yrow, src + (size_t)r * D * 8, (size_t)D * 8);
    return SMM_OK;
  };
  std::lock_guard<std::mutex> pipe_lock(op->pipe_mu);
  return run_grib_pipeline(op->pipe, op->grib, plan, x_host, rows, bitmaps, S, D, grib_needs_division(rows, n_batch),
                           is_pinned(pk ? (const void*)pk->out_host : y_host), launch_chunk, y_to_host, pk);
}

// smm_grib_pack: any float64 device result.  The tables go up from pageable vectors (taken when hipMemcpyAsync returns),
// the records come back into one, and the stream is synchronised before the scratch is freed.
int smm_grib_pack_impl(int device, const void* y, int64_t ldy, int64_t D, int64_t n_batch, const smm_grib_encode_t* enc,
                       void* out, const uint64_t* offs, smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out, void* stream) {
  if (n_batch == 0 || D == 0) return SMM_OK;
  DeviceGuard guard(device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the device");
  hipStream_t s = (hipStream_t)stream;
  const size_t n = (size_t)n_batch, tables = n * smm::kGribPackTableBytes, recs = n * smm::kGribOutRecordBytes;
  const smm::GribPackScratch sc = smm::grib_pack_scratch(D, n_batch);
  std::vector<uint64_t> t8(tables / 8);   // 8-byte aligned
  const uint32_t max_words = fill_pack_tables((char*)t8.data(), enc, n_batch, D, 0, offs);
  DeviceBuf<char> d;   // tables, records, scratch
  SMM_HIP(d.alloc(tables + recs + sc.bytes));
  SMM_HIP(hipMemcpyAsync(d.get(), t8.data(), tables, hipMemcpyHostToDevice, s));
  if (int rc = launch_pack(D, n_batch, (const double*)y, ldy, d.get(), (char*)out, (size_t)offs[n_batch], d.get() + tables,
                           d.get() + tables + recs, max_words, s)) {
    (void)hipStreamSynchronize(s);
    (void)hipGetLastError();
    return rc;
  }
  std::vector<uint64_t> r8(recs / 8);
  SMM_HIP(hipMemcpyAsync(r8.data(), d.get() + tables, recs, hipMemcpyDeviceToHost, s));
  SMM_HIP(hipStreamSynchronize(s));
  memcpy(rows_out, r8.data(), n * sizeof(smm_grib_row_t));
  memcpy(bitmaps_out, (const char*)r8.data() + n * sizeof(smm_grib_row_t), n * sizeof(smm_grib_bitmap_t));
  return SMM_OK;
}

// Host buffers, a group: chunks of whole outer indices (units of n_lev * n_inner consecutive records); Y is delivered as
// the whole-row mode of smm_group_apply_host delivers it, (n_outer, n_inner, n_lev, D) when transpose, else
// (n_lev, n_outer, n_inner, D).  pk (smm_group_apply_host_grib_pk): no Y is delivered -- a chunk's Y is written in record
// order, the (ch.nr, D) rows the pipeline's pack reads; transpose is not looked at.
int smm_group_apply_host_grib_impl(smm_group_t g, const void* x_host, const smm_grib_row_t* rows,
                                   const smm_grib_bitmap_t* bitmaps, void* y_host, int64_t n_outer, int64_t n_lev, int64_t n_inner,
                                   int transpose, const int32_t* level_index, const uint8_t* masked_levels, double area_min,
                                   unsigned flags, int64_t chunk_outer, const GribOut* pk = nullptr) {
  const int64_t S = g->ops[0]->csr.n_src, D = g->ops[0]->csr.n_dst;
  const int64_t unit = n_lev * n_inner, n_rows = n_outer * unit;
  if (n_rows == 0 || D == 0) return SMM_OK;
  DeviceGuard guard(g->device);
  if (!guard.ok) return fail(SMM_ERR_HIP, "cannot select the group's device");
  const int32_t* d_map;
  const uint8_t* d_masked;
  if (int rc = group_level_cfg(g, n_lev, level_index, masked_levels, area_min, flags, &d_map, &d_masked)) return rc;
  const std::vector<size_t> out_row = grib_out_row_bytes(pk, n_rows, D);
  const smm::GribChunkPlan plan = smm::plan_grib_chunks(rows, bitmaps, n_outer, unit, S, D, chunk_outer, free_device_bytes(),
                                                        pk ? out_row.data() : nullptr);
  auto launch_chunk = [&](const GribIn& in, const smm::GribChunk& ch, void* dy, hipStream_t s) -> int {
    const int64_t no = ch.nr / unit;
    int64_t ys_o, ys_l, ys_i;   // the chunk's Y on the device, as smm_group_apply_host lays out a whole-row chunk
    if (pk) {                   // ... or in record order: row (o, l, i) of the chunk is row (o * n_lev + l) * n_inner + i
      ys_o = unit * D, ys_l = n_inner * D, ys_i = D;
    } else if (transpose) {
      ys_o = n_inner * n_lev * D, ys_l = D, ys_i = n_lev * D;
    } else {
      ys_o = n_inner * D, ys_l = no * n_inner * D, ys_i = D;
    }
    return launch_grib_group_rows(g, d_map, d_masked, in, dy, ys_o, ys_l, ys_i, no, n_lev, n_inner, area_min, flags, s);
  };
  // Y of a chunk of `no` outer indices from o0: on the device (no, n_inner, n_lev, D) when transpose -- one block of
  // the host array -- else (n_lev, no, n_inner, D): one run per level
  auto y_to_host = [&](const smm::GribChunk& ch, const char* src, bool async, hipStream_t s) -> int {
    const int64_t o0 = ch.r0 / unit, no = ch.nr / unit;
    const size_t blk = (size_t)no * n_inner * D * 8;
    const int64_t runs = transpose ? 1 : n_lev;
    for (int64_t r = 0; r < runs; ++r) {
      const size_t bytes = transpose ? blk * (size_t)n_lev : blk;
      char* dst = (char*)y_host + (transpose ? (size_t)o0 * unit : (size_t)r * n_outer * n_inner + (size_t)o0 * n_inner) * D * 8;
      if (async) {
        SMM_HIP(hipMemcpyAsync(dst, src + (size_t)r * blk, bytes, hipMemcpyDeviceToHost, s));
      } else if (int rc = host_copy(dst, src + (size_t)r * blk, bytes)) {
        return rc;
      }
    }
    return SMM_OK;
  };
  std::lock_guard<std::mutex> pipe_lock(g->pipe_mu);
  return run_grib_pipeline(g->pipe, g->grib, plan, x_host, rows, bitmaps, S, D, grib_needs_division(rows, n_rows),
                           is_pinned(pk ? (const void*)pk->out_host : y_host), launch_chunk, y_to_host, pk);
}

// ---- the four entries behind the extern "C" names.  na: the _na twin -- check_grib_call puts SMM_APPLY_SKIPNA into
// flags, and from there the flag travels with them down to the launch
int grib_entry(bool na, smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
               const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ldy, int64_t n_batch, double remap_area_min,
               unsigned flags, void* stream) {
  return guarded([&] {
    if (int rc = check_grib_call(x, true, x_bytes, rows, y, y_dtype, n_batch, remap_area_min, &flags, na)) return rc;
    if (int rc = check_grib_operator(op, x_bytes, rows, bitmaps, ldy, n_batch, remap_area_min, flags)) return rc;
    return smm_apply_grib_impl(op, x, x_bytes, rows, bitmaps, y, ldy, n_batch, remap_area_min, flags, stream);
  });
}

int grib_host_entry(bool na, smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                    const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t ldy, int64_t n_batch,
                    double remap_area_min, unsigned flags, int64_t chunk_rows) {
  return guarded([&] {
    if (int rc = check_grib_call(x_host, false, x_bytes, rows, y_host, y_dtype, n_batch, remap_area_min, &flags, na)) return rc;
    if (int rc = check_grib_operator(op, x_bytes, rows, bitmaps, ldy, n_batch, remap_area_min, flags)) return rc;
    return smm_apply_host_grib_impl(op, x_host, rows, bitmaps, y_host, ldy, n_batch, remap_area_min, flags, chunk_rows);
  });
}

// What the two packing entries refuse about the result side, before any device is touched; fills offs (n_batch + 1)
int check_grib_out(const smm_grib_encode_t* enc, const void* out, bool out_device, int64_t out_bytes,
                   const smm_grib_row_t* rows_out, const smm_grib_bitmap_t* bitmaps_out, int64_t n_dst, int64_t n_batch,
                   std::vector<uint64_t>& offs) {
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (out_bytes < 0) return fail(SMM_ERR_INVALID, "negative out_bytes");
  if (n_batch > 0 && (!enc || !rows_out || !bitmaps_out)) return fail(SMM_ERR_INVALID, "null encode, row or bitmap record pointer");
  std::string err;
  if (!smm::check_grib_encode(enc, n_batch, n_dst, err)) return fail(SMM_ERR_INVALID, err);
  offs.assign((size_t)n_batch + 1, 0);
  offs[(size_t)n_batch] = smm::grib_out_layout(n_dst, enc, n_batch, offs.data());
  if ((uint64_t)out_bytes < offs[(size_t)n_batch])
    return fail(SMM_ERR_INVALID, "out_bytes " + std::to_string(out_bytes) + " is below the layout's " +
                                     std::to_string(offs[(size_t)n_batch]) + " bytes");
  if (!out && offs[(size_t)n_batch] > 0) return fail(SMM_ERR_INVALID, "null result pointer");
  if (out_device && (uintptr_t)out % 4) return fail(SMM_ERR_INVALID, "result pointer is not 4-byte aligned");
  return SMM_OK;
}

int grib_group_entry(bool na, smm_group_t g, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                     const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                     int64_t n_outer, int64_t n_lev, int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                     double remap_area_min, unsigned flags, void* stream) {
  return guarded([&] {
    const int64_t n_rows = grib_group_rows(n_outer, n_lev, n_inner);
    if (int rc = check_grib_call(x, true, x_bytes, rows, y, y_dtype, n_rows, remap_area_min, &flags, na)) return rc;
    if (int rc = check_grib_group(g, x_bytes, rows, bitmaps, n_rows, n_lev, level_index, masked_levels, remap_area_min, flags))
      return rc;
    return smm_group_apply_grib_impl(g, x, x_bytes, rows, bitmaps, y, ys_outer, ys_lev, ys_inner, n_outer, n_lev, n_inner,
                                     level_index, masked_levels, remap_area_min, flags, stream);
  });
}

int grib_group_host_entry(bool na, smm_group_t g, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                          const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t n_outer, int64_t n_lev,
                          int64_t n_inner, int transpose, const int32_t* level_index, const uint8_t* masked_levels,
                          double remap_area_min, unsigned flags, int64_t chunk_outer) {
  return guarded([&] {
    const int64_t n_rows = grib_group_rows(n_outer, n_lev, n_inner);
    if (int rc = check_grib_call(x_host, false, x_bytes, rows, y_host, y_dtype, n_rows, remap_area_min, &flags, na)) return rc;
    if (int rc = check_grib_group(g, x_bytes, rows, bitmaps, n_rows, n_lev, level_index, masked_levels, remap_area_min, flags))
      return rc;
    return smm_group_apply_host_grib_impl(g, x_host, rows, bitmaps, y_host, n_outer, n_lev, n_inner, transpose, level_index,
                                          masked_levels, remap_area_min, flags, chunk_outer);
  });
}

}  // namespace

// ---- the guarded entry points (include/smmregrid_amd.h): nothing crosses the extern "C" boundary but a status
extern "C" {

int smm_apply_grib(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows, void* y, int y_dtype,
                   int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, void* stream) {
  return smm_apply_grib_bm(op, x, x_bytes, rows, nullptr, y, y_dtype, ldy, n_batch, remap_area_min, flags, stream);
}

// bitmaps == NULL: the entry above
int smm_apply_grib_bm(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                      const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ldy, int64_t n_batch,
                      double remap_area_min, unsigned flags, void* stream) {
  return grib_entry(false, op, x, x_bytes, rows, bitmaps, y, y_dtype, ldy, n_batch, remap_area_min, flags, stream);
}

int smm_apply_grib_na(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                      const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ldy, int64_t n_batch,
                      double remap_area_min, unsigned flags, void* stream) {
  return grib_entry(true, op, x, x_bytes, rows, bitmaps, y, y_dtype, ldy, n_batch, remap_area_min, flags, stream);
}

int smm_apply_host_grib(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows, void* y_host,
                        int y_dtype, int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags,
                        int64_t chunk_rows) {
  return smm_apply_host_grib_bm(op, x_host, x_bytes, rows, nullptr, y_host, y_dtype, ldy, n_batch, remap_area_min, flags,
                                chunk_rows);
}

int smm_apply_host_grib_bm(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t ldy, int64_t n_batch,
                           double remap_area_min, unsigned flags, int64_t chunk_rows) {
  return grib_host_entry(false, op, x_host, x_bytes, rows, bitmaps, y_host, y_dtype, ldy, n_batch, remap_area_min, flags,
                         chunk_rows);
}

int smm_apply_host_grib_na(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t ldy, int64_t n_batch,
                           double remap_area_min, unsigned flags, int64_t chunk_rows) {
  return grib_host_entry(true, op, x_host, x_bytes, rows, bitmaps, y_host, y_dtype, ldy, n_batch, remap_area_min, flags,
                         chunk_rows);
}

int smm_grib_out_layout(int64_t n_dst, const smm_grib_encode_t* enc, int64_t n_batch, uint64_t* byte_off,
                        uint64_t* total_bytes) {
  return guarded([&] {
    if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
    if (!total_bytes || (n_batch > 0 && !enc)) return fail(SMM_ERR_INVALID, "null encode or total pointer");
    std::string err;
    if (!smm::check_grib_encode(enc, n_batch, n_dst, err)) return fail(SMM_ERR_INVALID, err);
    *total_bytes = smm::grib_out_layout(n_dst, enc, n_batch, byte_off);
    return (int)SMM_OK;
  });
}

int smm_grib_pack(int device, const void* y, int64_t ldy, int64_t n_dst, int64_t n_batch, const smm_grib_encode_t* enc,
                  void* out, int64_t out_bytes, smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out, void* stream) {
  return guarded([&] {
    std::vector<uint64_t> offs;
    if (int rc = check_grib_out(enc, out, true, out_bytes, rows_out, bitmaps_out, n_dst, n_batch, offs)) return rc;
    if (!y && n_batch > 0 && n_dst > 0) return fail(SMM_ERR_INVALID, "null field pointer");
    if ((uintptr_t)y % 8) return fail(SMM_ERR_INVALID, "field pointer is not element aligned");
    if (n_batch > 0 && ldy < n_dst) return fail(SMM_ERR_INVALID, "ldy smaller than the grid size");
    return smm_grib_pack_impl(device, y, ldy, n_dst, n_batch, enc, out, offs.data(), rows_out, bitmaps_out, stream);
  });
}

int smm_apply_host_grib_pk(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps, const smm_grib_encode_t* enc, void* out_host, int64_t out_bytes,
                           smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out, int64_t n_batch, double remap_area_min,
                           unsigned flags, int64_t chunk_rows) {
  return guarded([&] {
    static const double no_y = 0.0;   // the float64 Y of this entry never leaves the device: nothing of the caller's to check
    const bool na = (flags & SMM_APPLY_SKIPNA) != 0;
    if (int rc = check_grib_call(x_host, false, x_bytes, rows, &no_y, SMM_F64, n_batch, remap_area_min, &flags, na)) return rc;
    if (!op) return fail(SMM_ERR_INVALID, "null operator");
    std::vector<uint64_t> offs;
    if (int rc = check_grib_out(enc, out_host, false, out_bytes, rows_out, bitmaps_out, op->csr.n_dst, n_batch, offs)) return rc;
    if (int rc = check_grib_operator(op, x_bytes, rows, bitmaps, op->csr.n_dst, n_batch, remap_area_min, flags)) return rc;
    const GribOut pk{enc, offs.data(), (char*)out_host, rows_out, bitmaps_out};
    return smm_apply_host_grib_impl(op, x_host, rows, bitmaps, nullptr, op->csr.n_dst, n_batch, remap_area_min, flags,
                                    chunk_rows, &pk);
  });
}

int smm_group_apply_host_grib_pk(smm_group_t g, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                                 const smm_grib_bitmap_t* bitmaps, const smm_grib_encode_t* enc, void* out_host, int64_t out_bytes,
                                 smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out, int64_t n_outer, int64_t n_lev,
                                 int64_t n_inner, const int32_t* level_index, const uint8_t* masked_levels,
                                 double remap_area_min, unsigned flags, int64_t chunk_outer) {
  return guarded([&] {
    static const double no_y = 0.0;   // as smm_apply_host_grib_pk: no Y of the caller's to check
    const bool na = (flags & SMM_APPLY_SKIPNA) != 0;
    const int64_t n_rows = grib_group_rows(n_outer, n_lev, n_inner);
    // the result side first; the layout needs the group's n_dst -- without a group the records alone are looked at
    // (no cell, no slot bytes) and check_grib_group below refuses the handle
    std::vector<uint64_t> offs;
    if (int rc = check_grib_out(enc, out_host, false, out_bytes, rows_out, bitmaps_out, g ? g->ops[0]->csr.n_dst : 0, n_rows, offs))
      return rc;
    if (int rc = check_grib_call(x_host, false, x_bytes, rows, &no_y, SMM_F64, n_rows, remap_area_min, &flags, na)) return rc;
    if (int rc = check_grib_group(g, x_bytes, rows, bitmaps, n_rows, n_lev, level_index, masked_levels, remap_area_min, flags))
      return rc;
    const GribOut pk{enc, offs.data(), (char*)out_host, rows_out, bitmaps_out};
    return smm_group_apply_host_grib_impl(g, x_host, rows, bitmaps, nullptr, n_outer, n_lev, n_inner, 1, level_index,
                                          masked_levels, remap_area_min, flags, chunk_outer, &pk);
  });
}

int smm_group_apply_grib(smm_group_t g, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                         const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev,
                         int64_t ys_inner, int64_t n_outer, int64_t n_lev, int64_t n_inner, const int32_t* level_index,
                         const uint8_t* masked_levels, double remap_area_min, unsigned flags, void* stream) {
  return grib_group_entry(false, g, x, x_bytes, rows, bitmaps, y, y_dtype, ys_outer, ys_lev, ys_inner, n_outer, n_lev, n_inner,
                          level_index, masked_levels, remap_area_min, flags, stream);
}

int smm_group_apply_grib_na(smm_group_t g, const void* x, int64_t x_bytes, const smm_grib_row_t* rows,
                            const smm_grib_bitmap_t* bitmaps, void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev,
                            int64_t ys_inner, int64_t n_outer, int64_t n_lev, int64_t n_inner, const int32_t* level_index,
                            const uint8_t* masked_levels, double remap_area_min, unsigned flags, void* stream) {
  return grib_group_entry(true, g, x, x_bytes, rows, bitmaps, y, y_dtype, ys_outer, ys_lev, ys_inner, n_outer, n_lev, n_inner,
                          level_index, masked_levels, remap_area_min, flags, stream);
}

int smm_group_apply_host_grib(smm_group_t g, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                              const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t n_outer,
                              int64_t n_lev, int64_t n_inner, int transpose, const int32_t* level_index,
                              const uint8_t* masked_levels, double remap_area_min, unsigned flags, int64_t chunk_outer) {
  return grib_group_host_entry(false, g, x_host, x_bytes, rows, bitmaps, y_host, y_dtype, n_outer, n_lev, n_inner, transpose,
                               level_index, masked_levels, remap_area_min, flags, chunk_outer);
}

int smm_group_apply_host_grib_na(smm_group_t g, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                                 const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t n_outer,
                                 int64_t n_lev, int64_t n_inner, int transpose, const int32_t* level_index,
                                 const uint8_t* masked_levels, double remap_area_min, unsigned flags, int64_t chunk_outer) {
  return grib_group_host_entry(true, g, x_host, x_bytes, rows, bitmaps, y_host, y_dtype, n_outer, n_lev, n_inner, transpose,
                               level_index, masked_levels, remap_area_min, flags, chunk_outer);
}

}  // extern "C"
