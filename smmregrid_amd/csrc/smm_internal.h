// Internal structures shared by the host builder (smm_build.cpp) and the
// device side (smm_device.hip).  Not part of the ABI.
#pragma once

#include <cstdint>
#include <string>
#include <vector>

struct smm_grib_row_t;   // include/smmregrid_amd.h
struct smm_grib_bitmap_t;
struct smm_grib_encode_t;
struct smm_grib_aec_t;
struct smm_grib_cpx_t;

namespace smm {

// Canonical CSR: row = destination cell, columns ascending, duplicates summed.
// This is the structure scipy's coo_matrix((w,(dst,src))).tocsr() +
// sum_duplicates() + sort_indices() yields, and what the reference's
// sparse.COO([src,dst], w) holds after its constructor sorted the coords
// (weights.py:37-39).
struct HostCsr {
  int64_t n_src = 0, n_dst = 0, nnz = 0;
  int64_t n_used_src = 0;   // distinct source cells carrying >= 1 link (U of SURVEY 8d)
  int64_t max_row_nnz = 0;
  std::vector<int64_t> rowptr;  // n_dst + 1
  std::vector<int32_t> col;     // nnz
  std::vector<double> val;      // nnz
};

// SELL-64: destination rows in slices of 64 consecutive rows (= one wavefront);
// inside a slice the links are stored slot-major (slot k of lane r at
// off + k*64 + r) and padded to the longest row of the slice, so a wave reads
// col/val with one coalesced 256-B / 512-B access per slot.
struct HostSell {
  int64_t n_slices = 0;
  int64_t n_slots = 0;              // total padded slots (multiple of 64)
  std::vector<int64_t> slice_off;   // n_slices + 1, element offsets (multiples of 64)
  std::vector<int32_t> rowlen;      // n_slices * 64 (rows past n_dst have length 0)
  std::vector<int32_t> col;         // n_slots (padding: 0)
  std::vector<double> val;          // n_slots (padding: 0.0)
};

// Threads of the host-side builders below.  set_host_threads(n): n > 0 fixes the count, 0 = automatic
// (hardware threads, at most 16, shared between the builders running at that moment, and never more
// than the work is worth); returns the previous setting.  The results do not depend on the count.
int set_host_threads(int n);
int fixed_host_threads();   // the count set by set_host_threads (0 = automatic)
int host_threads(int64_t work_items, int64_t min_items_per_thread);
// CPUs this process may really use: the scheduler affinity capped by the cgroup CPU quota (a 16-CPU share of a
// 256-thread host has affinity 256 and a quota of 16); >= 1, read once.
int usable_cpus();
// Test hook of the builders' worker pools (tests/cpp/build_harness.cpp): no_threads = behave as if no thread could
// be started (every task then runs on the caller); throw_in_task >= 0 = the task body started after that many
// others throws std::bad_alloc (-1 = off).  Whatever a worker throws is rethrown on the calling thread after
// every started thread has been joined.
void debug_builder_faults(bool no_threads, int64_t throw_in_task);

// ---- host side of the host-buffer pipelines (smm_hostpool.cpp).  None of these throws; the int results are
// 0 = done, 1 = out of memory inside a task, 2 = any other failure inside a task.
// One persistent worker pool per process: fn(ctx, i) for i in [0, n_tasks), claimed one by one by the calling
// thread and up to max_threads - 1 workers (started on first need, kept).  A worker that cannot be started
// costs parallelism only; jobs of concurrent callers take turns.
int pool_run(int64_t n_tasks, int max_threads, void (*fn)(void*, int64_t), void* ctx) noexcept;
int pool_workers();        // workers alive in this process (tests)
int staging_threads();     // threads a staging stage uses: set_host_threads(n) if n > 0, else min(16, usable_cpus())
// Test hooks of the pool (tests/cpp/build_harness.cpp): no_threads = behave as if no worker could be started;
// throw_in_task >= 0 = the task body started after that many others throws std::bad_alloc (-1 = off).
void debug_pool_faults(bool no_threads, int64_t throw_in_task);
// parallel memcpy (pageable <-> pinned staging): one thread tops out far below PCIe
int host_copy(void* dst, const void* src, size_t bytes) noexcept;
// the same for `height` rows of `width` bytes at row pitches dpitch / spitch (the level range of a chunk inside Y)
int host_copy_2d(void* dst, size_t dpitch, const void* src, size_t spitch, size_t width, int64_t height) noexcept;
// Pack of the host pipelines: out[u * rows + r] = X[entry r][used[u]] -- the used source cells of a chunk of batch
// entries, batch-fastest, ready for smm_apply_sb (SMM_APPLY_SB_PACKED).  Batch entry r is the source row at
// x + (r / n_inner) * stride_o + (r % n_inner) * stride_i (elements of xsz bytes): plain row blocks have
// n_inner >= rows and stride_i = ldx; one level of an (outer, level, inner, S) field has stride_o = n_lev * n_inner * S,
// stride_i = S.  streaming = write the packed block with non-temporal stores (a staging buffer only the DMA reads).
int host_pack(void* out, const void* x, size_t xsz, int64_t n_inner, int64_t stride_o, int64_t stride_i,
              const int32_t* used, int64_t U, int64_t rows, bool streaming) noexcept;

// Returns false and fills err on invalid input.
bool build_csr(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src1,
               const int32_t* dst1, const double* w, HostCsr& out, std::string& err);
// Adopts an already canonical CSR (what smm_operator_export_csr wrote): validates it (rowptr
// monotone from 0, columns strictly ascending inside a row and < n_src) instead of sorting.
bool adopt_csr(int64_t n_src, int64_t n_dst, const int64_t* rowptr, const int32_t* col,
               const double* val, HostCsr& out, std::string& err);
// Drops links whose (duplicate-summed) weight is exactly +-0.0; returns how many went.  With the 1e20
// fill every gathered value is finite, so such a link contributes +-0.0 to a sum that starts at +0.0:
// the results are bit-identical with or without it (not so under SMM_APPLY_NO_FILL with non-finite X,
// whose contract excludes them).  Bilinear weights between aligned grids are full of them: r1440x721 ->
// r360x180 keeps 1 link of 4.
int64_t prune_zero_links(HostCsr& csr);
void build_sell(const HostCsr& csr, HostSell& out);

// ---- operators with weight columns (smm_operator_create_cols): remap_matrix rows of n_cols weights, 1..4 -- the value
// weight and the gradient weights of bicubic (4) and second-order conservative (3) files.  w is [nnz * n_cols], link k's
// weights at w + k * n_cols.  out is the canonical CSR of column 0, exactly what build_csr makes of that column alone;
// extra[k - 1][p] is column k of link p of that CSR: the sort by (dst, src), the tie-break and the sequential duplicate
// summing are those of build_csr, applied to every column with the same permutation.  n_cols outside 1..4: false + err.
constexpr int kMaxWeightCols = 4;
bool build_csr_cols(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src1, const int32_t* dst1, const double* w,
                    int n_cols, HostCsr& out, std::vector<std::vector<double>>& extra, std::string& err);
// prune_zero_links for such an operator: a link goes only when ALL its columns are exactly +-0.0
int64_t prune_zero_links_cols(HostCsr& csr, std::vector<std::vector<double>>& extra);
// The SELL-64 slot planes of the extra columns beside HostSell.val: plane k - 1 at out[(k - 1) * n_slots ..], the slot
// layout of build_sell, padded slots +0.0
void build_sell_cols(const HostCsr& csr, const HostSell& sell, const std::vector<std::vector<double>>& extra,
                     std::vector<double>& out);

// Source-tile plan for the LDS-staged kernel.  Destination rows are grouped in
// blocks of `rows_per_block` consecutive rows (4 SELL slices, 1 slice, or 1/2, 1/4, 1/8 of a slice
// for rows whose footprint is wide); the distinct source cells a block
// references are covered by aligned chunks of `chunk_elems` source elements
// (4 elements: 32 B of f64, one 16-B staging piece of f32 -- the L2 fetches whole 128-B lines whatever
// is staged, but fine chunks keep rows that do not start on a line boundary, and sparse stencils, from
// staging and straddling lines they do not need).  The kernel copies a block's chunks to
// LDS in list order with 16-B-per-lane coalesced loads, so LDS element
// (c*chunk_elems + e) holds source element chunk_src[c]*chunk_elems + e, and
// the block's links address LDS through lcol.
struct HostTilePlan {
  bool valid = false;
  int32_t rows_per_block = 0;
  int32_t chunk_elems = 0;
  int64_t n_blocks = 0;
  int64_t max_block_chunks = 0;       // largest chunk count of any block
  int64_t total_chunks = 0;           // sum over blocks = staged chunks per batch row
  int64_t total_lines = 0;            // sum over staged blocks of the distinct 16-element groups (128-B lines of
                                      // f64) their chunks touch: what HBM moves per batch row
  std::vector<int32_t> blk_lines;     // n_blocks: that count per block
  int64_t total_distinct = 0;         // sum over blocks of distinct source cells referenced
  int64_t distinct_chunks = 0;        // distinct source chunks over the whole operator
  int64_t direct_links = 0;           // links of blocks too wide to stage (gathered from X directly)
  std::vector<uint8_t> blk_direct;    // n_blocks: 1 = footprint beyond the LDS budget, no chunks listed
  std::vector<int64_t> blk_chunk_off; // n_blocks + 1 -> index into chunk_src
  std::vector<int32_t> chunk_src;     // source chunk index (element = idx * chunk_elems)
  std::vector<int32_t> lcol;          // per SELL slot: LDS element index (layout of HostSell.col)
};
// Blocks needing more than max_chunks_per_block chunks are marked direct; plan.valid == false when
// they carry more than a quarter of the links (then the SELL kernel serves the operator better).
// A few very wide blocks (polar caps of HEALPix targets) would size the LDS tile -- and with it the
// workgroups per CU -- for every block.  Picks the smallest of full_budget/8, /4, /2 chunks that
// leaves at most 1 % of the links in over-budget blocks, marks those blocks direct and drops their
// chunk lists.  Returns the budget in force (full_budget when nothing changed).
int64_t tighten_tile_plan(const HostCsr& csr, HostTilePlan& plan, int64_t full_budget);
void build_tile_plan(const HostCsr& csr, const HostSell& sell, int32_t rows_per_block,
                     int32_t chunk_elems, int64_t max_chunks_per_block, HostTilePlan& plan);

// Launch grids are 1-D and hold at most 2^31 - 1 workgroups.  A batch of (n_outer x n_inner) rows whose
// grid would be larger is cut into parts -- halves of the outer range first, then of the inner range --
// until every part fits; `blocks(n_o, n_i)` is the grid a part of that shape needs (it depends on the
// part: short batches walk fewer rows per workgroup), `emit(o0, n_o, i0, n_i)` launches one part and
// returns 0 on success.  Returns 0, emit's first non-zero status, or -1 when a single batch row alone
// exceeds the limit (nothing is launched for that part; earlier parts have been).
template <typename Blocks, typename Emit>
int split_batch(int64_t o0, int64_t n_o, int64_t i0, int64_t n_i, int64_t limit, Blocks&& blocks, Emit&& emit) {
  if (n_o <= 0 || n_i <= 0) return 0;
  if (blocks(n_o, n_i) <= limit) return emit(o0, n_o, i0, n_i);
  if (n_o > 1) {
    const int64_t h = (n_o + 1) / 2;
    if (int rc = split_batch(o0, h, i0, n_i, limit, blocks, emit)) return rc;
    return split_batch(o0 + h, n_o - h, i0, n_i, limit, blocks, emit);
  }
  if (n_i > 1) {
    const int64_t h = (n_i + 1) / 2;
    if (int rc = split_batch(o0, n_o, i0, h, limit, blocks, emit)) return rc;
    return split_batch(o0, n_o, i0 + h, n_i - h, limit, blocks, emit);
  }
  return -1;
}

// Chunk sizing of the host-buffer pipelines (smm_apply_host / smm_group_apply_host).  A chunk's X
// AND Y staging are each allocated twice on the device and twice as pinned host memory, so a chunk
// is sized from the bytes one batch unit (a row; an outer index of a level group) needs on both
// sides -- an operator with few used source cells and a large target (U << D) is bound by its Y.
struct HostChunk {
  int64_t units = 0;   // batch rows (or outer indices) per chunk, >= 1
  bool pack = false;   // the packing variant is in force for this call
};
// x_unit / y_unit: device bytes per unit of the whole-row form; xp_unit: packed X bytes per unit
// (0 = packing not applicable).  min_pack_units: fewest units per chunk that still feed the pack loops
// and the batch-fastest kernel (32 batch entries); pack_align: packed chunks are whole multiples of
// this when they are at least that long (the kernel's 128-entry batch tile).  requested > 0 = the
// caller's chunk size (kept; packing is dropped if it is below min_pack_units and does not cover
// the batch).  free_bytes = free device memory (0 = unknown): a chunk never asks for more than a
// quarter of it across its four device buffers.
HostChunk host_chunk_units(int64_t n_units, size_t x_unit, size_t y_unit, size_t xp_unit,
                           int64_t min_pack_units, int64_t pack_align, int64_t requested,
                           size_t free_bytes);

// Chunk plan of smm_group_apply_host: which outer indices x data levels each chunk of the pipeline holds.
struct GroupChunk {
  int64_t o0, no, l0, nl;   // outer indices [o0, o0 + no) of data levels [l0, l0 + nl)
  size_t x_bytes;           // packed X bytes of the chunk (pack mode; 0 for whole rows)
};
struct GroupChunkPlan {
  bool pack = false;                 // chunks ship each level's used cells batch-fastest, else whole rows
  size_t x_row = 0;                  // device bytes of a whole row of X: rows start on 128-B lines
  std::vector<GroupChunk> chunks;    // tile [0, n_outer) x [0, n_lev) exactly once, in pipeline order
  size_t max_x = 0, max_y = 0, max_rows = 0;   // largest device X / Y bytes and whole batch rows of one chunk
};
// X (n_outer, n_lev, n_inner, S) of xsz-byte cells, Y (.., D) of ysz-byte cells; used_per_level[l] = n_used_src of data
// level l.  packing_allowed: no flag of the call rules packing out.  requested_outer, free_bytes: as host_chunk_units.
// budget_kb > 0 (SMM_TUNE_HOST_CHUNK_KB) forces level-major chunks of that staging budget.  Rules: with the body.
GroupChunkPlan plan_group_chunks(int64_t n_outer, int64_t n_lev, int64_t n_inner, int64_t S, int64_t D, size_t xsz,
                                 size_t ysz, const int64_t* used_per_level, bool packing_allowed,
                                 int64_t requested_outer, size_t free_bytes, int64_t budget_kb);

// ---- GRIB simple-packed fields shipped raw (the smm_*apply*_grib* entries; smm_grib_plan.cpp, plain C++).  `bitmaps` is
// null in a call without bitmap records (smm_apply_grib, smm_apply_host_grib) and has one record per row otherwise.
// What the entries refuse about their row table before any device is touched: false + err.  check_grib_rules looks at the
// rules alone (nbits, reserved, bscale a normal power of two, ddiv finite and > 0, ref finite); check_grib_ranges at where
// each row's bytes lie in [0, x_bytes): ceil(n_src * nbits / 8) data bytes, or with a bitmap ceil(n_values * nbits / 8) of
// them and the ceil(n_src / 8) bytes of the bitmap -- and at n_values <= n_src in every record.
bool check_grib_rules(const smm_grib_row_t* rows, int64_t n_batch, std::string& err);
bool check_grib_ranges(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_batch, int64_t n_src,
                       int64_t x_bytes, std::string& err);
// What a row costs a host entry.  Staged through the pinned buffer: its table record (40 B), its bitmap record (16 B, when
// the call has records), its data bytes and, with a bitmap, its bitmap bytes, each rounded up to 4.  Device-only: its
// share of the rank buffer -- with a bitmap one 8-byte entry per 32 cells and its 4-byte segment totals.  bm: the row's
// record, or null.  The planner sums these and the layout of a chunk advances by them: there is no second arithmetic.
struct GribRowCost {
  bool has_bitmap = false;
  size_t records = 0;
  size_t data_bytes = 0, bitmap_bytes = 0;       // as they lie in the caller's buffer
  size_t staged_data = 0, staged_bitmap = 0;     // the same rounded up to 4
  size_t rank = 0;
  size_t staged() const { return records + staged_data + staged_bitmap; }
};
GribRowCost grib_row_cost(const smm_grib_row_t& row, const smm_grib_bitmap_t* bm, int64_t n_src);
// Chunk plan of the host entries: consecutive rows [r0, r0 + nr) per chunk, in whole units -- a unit is one row for
// smm_apply_host_grib(_bm) (n_outer = n_batch, unit = 1) and the n_lev * n_inner consecutive records of an outer index
// for smm_group_apply_host_grib: r0 and nr of every chunk are multiples of `unit`.  Rows differ in width, so a chunk is
// sized by bytes, not by rows: its staged bytes, its rank bytes and nr * D * 8 of Y stay within the target (~256 MiB; an
// eighth of the call so that chunks overlap, but no less than 32 MiB; an eighth of free_bytes when that is known: the
// four device buffers of a chunk take a quarter of it at most).  A unit that alone exceeds the target still gets a chunk
// of its own.  requested_units > 0: that many units per chunk (the last may be short).  n_outer <= 0 or unit <= 0: no chunks.
struct GribChunk {
  int64_t r0, nr;
  size_t x_bytes;          // staged bytes of the chunk: the sum of its rows' GribRowCost::staged()
  size_t rank_bytes = 0;   // the chunk's device-only rank tables and segment totals
};
struct GribChunkPlan {
  std::vector<GribChunk> chunks;   // cover [0, n_outer * unit) exactly once, in order
  size_t target = 0;               // the byte bound in force (0 with requested_units)
  size_t max_x = 0;                // largest staged X of one chunk
  int64_t max_rows = 0;            // most rows of one chunk
  size_t max_rank = 0;             // largest rank_bytes of one chunk
};
// out_row_bytes: null, or per row what its packed result adds on the device beside its Y (smm_apply_host_grib_pk and
// smm_group_apply_host_grib_pk: the row's slot, records, pack tables and scratch): counted into the chunk's bytes with
// the rest, per unit.
GribChunkPlan plan_grib_chunks(const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps, int64_t n_outer, int64_t unit,
                               int64_t n_src, int64_t D, int64_t requested_units, size_t free_bytes,
                               const size_t* out_row_bytes = nullptr);

// ---- results packed back into GRIB (smm_grib_pack, smm_apply_host_grib_pk; smm_grib_plan.cpp).  What the entries refuse
// about the encode records (nbits 1..32, ddiv finite and > 0, reserved 0) and the sizes (n_dst in [0, 2^31)): false + err
bool check_grib_encode(const smm_grib_encode_t* enc, int64_t n_batch, int64_t n_dst, std::string& err);
// the layout: byte_off[b] (byte_off may be null) = start of row b's slot; returns the bytes of all slots
uint64_t grib_out_layout(int64_t n_dst, const smm_grib_encode_t* enc, int64_t n_batch, uint64_t* byte_off);
// Device scratch of a pack of n_rows rows of n_dst cells, one block cut into pieces at these byte offsets (each a
// multiple of 8): the segments' partial tmin / tmax / counts, the rows' rules, the rank tables and their segment totals
struct GribPackScratch {
  size_t part_min = 0, part_max = 0, part_cnt = 0, rules = 0, table = 0, totals = 0, bytes = 0;
};
GribPackScratch grib_pack_scratch(int64_t n_dst, int64_t n_rows);
// the records of a packed row as they travel in front of a chunk's slots: smm_grib_row_t + smm_grib_bitmap_t
constexpr size_t kGribOutRecordBytes = 40 + 16;
// the pack tables of a row staged behind a chunk's X: GribPackRow + GribRowBitmap (smm_grib.hpp, smm_grib_codec.hpp)
constexpr size_t kGribPackTableBytes = 32 + 16;
// ---- CCSDS-packed fields (smm_grib_aec_unpack, smm_grib_aec_decode_host; smm_grib_plan.cpp).  What the entries refuse
// about the records -- nbits 0..32, reserved 0, n_values < 2^31 and, for a row with a stream (nbits > 0), a block size of
// 8 / 16 / 32 / 64, rsi 1..4096, the refused flags and a stream inside [0, x_bytes): false + err
bool check_grib_aec(const smm_grib_aec_t* recs, int64_t n_batch, int64_t x_bytes, std::string& err);
// the layout of the transcoded streams: byte_off[b] (may be null) = start of row b's; returns the bytes of all
uint64_t grib_aec_layout(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off);
// ---- complex-packed fields (smm_grib_cpx_unpack, smm_grib_cpx_decode_host; smm_grib_plan.cpp).  What the entries refuse
// about the records of rows that are not marked simple-packed -- order 0..2, n_oct 1..4 with an order, the three bit counts
// 0..32, the two one-octet parameters 0..255, reserved 0, n_values < 2^31 and > order (or 0), a group for any value, a
// stream inside [0, x_bytes): false + err
bool check_grib_cpx(const smm_grib_cpx_t* recs, int64_t n_batch, int64_t x_bytes, std::string& err);
// the layout of the transcoded rows, n_values * 4 bytes per coded row: byte_off[b] (may be null); returns the bytes of all
uint64_t grib_cpx_layout(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off);
// missing value management per row (the _mv entries; mvm may be null: all zero): a value above 2 is refused: false + err
bool check_grib_cpx_mvm(const uint8_t* mvm, int64_t n_batch, std::string& err);
// the layout with mvm: a coded row with mvm != 0 gets, behind its slot, a bitmap slot of ceil(n_values / 8) bytes rounded
// up to 4; bitmap_off[b] (may be null) = where it starts, SMM_GRIB_NO_BITMAP for a row without one
uint64_t grib_cpx_layout_mv(const smm_grib_cpx_t* recs, const uint8_t* mvm, int64_t n_batch, uint64_t* byte_off,
                            uint64_t* bitmap_off);
// Where a chunk's pieces lie in its staging buffer hx (ch.x_bytes bytes, 8-byte aligned), written into hx: the table first
// -- the rows' records with byte_off the staged offset of the row's data -- then, with bitmaps, their records
// (GribRowBitmap, smm_grib_codec.hpp: bitmap_off a staged offset too, table_off the place of the row's rank table among
// the chunk's: its number among the bitmapped rows x ceil(n_src / 32)), then row by row the room for the data and, behind
// it, for the row's own copy of its bitmap.  Only the records are written; the caller copies the bytes.
struct GribChunkLayout {
  size_t end = 0;        // first byte behind the last piece: ch.x_bytes
  size_t n_tables = 0;   // bitmapped rows of the chunk
};
GribChunkLayout layout_grib_chunk(char* hx, const GribChunk& ch, const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                                  int64_t n_src);

}  // namespace smm
