// smm_grib_cpx_unpack (gfx950): the complex-packed streams of GRIB-2 templates 5.2 / 5.3 turned into simple-packed
// streams on the device, and the two host-only entries beside it (smm_grib_cpx_layout, smm_grib_cpx_decode_host).  The
// format and the two rules that bound every loop and read are the text of smm_grib_cpx.hpp; the kernels read the stream
// through its Stream::peek and take the tables apart with its sections / group_of / group_ref / descriptors.  Kernels
// in stream order -- a kernel boundary is the only ordering between passes, no workgroup ever waits for another one:
//   groups   a lane per group: stored width and length -> w_g, L_g, w_g L_g; a workgroup scan leaves every group its
//            value and bit offset within its tile of 256 groups, and the tile's sums
//   offsets  a wave per row scans the tile sums, 64 at a step; checks the sum of the lengths and the bits' end
//   values   a lane per value: its group by binary search (the tiles' value offsets, then the groups of the tile),
//            one extraction for the reference and one for the value; z + g (or the seed h) into 8 bytes of scratch
//   order 1 and 2, once or twice: reduce (a workgroup per tile of 1024 values), carries (a wave per row over the tile
//            sums), apply (the tile's inclusive prefix sum in place).  The last pass over a row -- the values kernel at
//            order 0 -- checks X < 2^32 and raises the row's maximum with atomicMax
//   store    a thread per 32-bit output word at the row's own width, the bit length of that maximum
// A row with missing values inside its groups (mvm 1 or 2, the _mv entries) goes through three kernels in place of the
// values kernel -- a row with mvm 0 runs the kernels above and no other:
//   values_mv  a lane per coded POSITION: the same search and extractions, the missing-value rule; z + g into a second
//            scratch array (8 more bytes per position), the wave's ballot as two big-endian words of the row's bitmap
//            in out, the workgroup's present count per 256 positions
//   ranks    a wave per row scans those counts; the row's P goes into a device word
//   compact  a lane per position reads its bitmap bit; a present one puts a_rank (the seed h for rank < order) at its
//            rank.  The prefix sums, the maximum and the store then run over P read from that word (grids sized by
//            n_values: the surplus workgroups leave); P comes back with the statuses in the one read-back
// A row that fails gets its status and is skipped by every later pass.  No lane reads a word that another lane of the
// same kernel writes: `structure` is written by groups / offsets and gates what follows, `range` is written by the last
// pass and read by the store; the bitmap words are written by values_mv and read by compact, P is written by ranks and
// read from reduce on.  The one in-place pattern is scan_parts': the lane that read a part overwrites that part with
// the sum before it, no other lane touches it -- the tile sums in offsets and carries, the counts in ranks (written by
// values_mv, read by compact).  Plain vector stores and vector atomics (atomicMax on a 32-bit word per row).  The scans
// (block_scan, scan_parts), raise, the store, the cut launches, the host shell and the entry checks are
// smm_grib_xcode.hpp's, shared with the other transcoders.
#include "smm_grib_xcode.hpp"

#include "smm_grib_cpx.hpp"

namespace {

constexpr int kCpxThreads = 256;
constexpr int kGroupTile = kCpxThreads;       // groups of a tile: one per lane
constexpr int kPerLane = 4;
constexpr int kValueTile = kCpxThreads * kPerLane;   // values of a tile of the prefix sums

struct CpxRow {   // what a row of the call brings to the device
  smm_cpx::Row r;
  uint64_t group_off;   // the row's first entry in CpxArgs::groups
  uint64_t gtile_off;   // ... in gtiles
  uint64_t value_off;   // ... in values
  uint64_t vtile_off;   // ... in vtiles
  uint64_t out_off;     // the row's slot in out, in bytes: a multiple of 4
  uint32_t coded;       // 0: the row is simple-packed already, or holds no value: nothing is done
  uint32_t mvm;         // missing value management: 0, or 1 / 2 -- codes inside the groups, the row gets a bitmap
  uint64_t bm_off;      // mvm != 0: the row's bitmap slot in out, in bytes: a multiple of 4
  uint64_t stage_off;   // ... its first entry in CpxArgs::staged
  uint64_t block_off;   // ... in counts
};
struct CpxGroup {       // a group after the groups kernel; 16 B
  uint64_t bit_excl;    // bits of the tile's groups before it
  uint32_t value_excl;  // values of the tile's groups before it
  uint32_t width;
};
struct CpxTile {        // a tile of groups: its sums, after the offsets kernel the sums of the row's tiles before it
  uint64_t values, bits;
};
struct CpxArgs {
  const void* x;
  const CpxRow* rows;
  CpxGroup* groups;
  CpxTile* gtiles;
  uint64_t* values;     // 8 B per value: a_i, then its prefix sums
  uint64_t* vtiles;     // a tile of values: its sum, then the sum of the row's tiles before it
  uint32_t* out;
  int32_t* structure;   // [n_j] status from the tables (the host puts what sections() says)
  int32_t* range;       // [n_j] status from the integers
  uint32_t* xmax;       // [n_j] the row's largest X
  uint32_t* present;    // [n_j] P of a row with mvm != 0: its present values
  uint64_t* staged;     // rows with mvm != 0, 8 B per position: z + g where the position lies, before the compaction
  uint32_t* counts;     // ... per 256 positions: the present ones, after the ranks kernel those of the row's blocks before
};

// what scan_parts needs to scan both sums of the tiles at once
__device__ __forceinline__ CpxTile operator+(CpxTile a, CpxTile b) { return CpxTile{a.values + b.values, a.bits + b.bits}; }
__device__ __forceinline__ CpxTile operator-(CpxTile a, CpxTile b) { return CpxTile{a.values - b.values, a.bits - b.bits}; }
__device__ __forceinline__ CpxTile wave_scan(CpxTile v) { return CpxTile{wave_scan(v.values), wave_scan(v.bits)}; }
__device__ __forceinline__ CpxTile wave_last(CpxTile v) { return CpxTile{wave_last(v.values), wave_last(v.bits)}; }

// ---- groups.  Workgroup (row, tile) takes groups [256 tile, 256 tile + 256).
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_groups_kernel(CpxArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint64_t lds[kCpxThreads];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part, tid = threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const smm_cpx::Row& r = row.r;
  if (!row.coded || (uint64_t)tile * kGroupTile >= r.n_groups) return;
  const smm_cpx::Sections sec = smm_cpx::sections(r);
  if (sec.status != smm_cpx::kOk) return;   // the tables do not fit: nothing is read
  const smm_cpx::Stream s = smm_cpx::stream_of(a.x, r);
  const uint32_t g = tile * kGroupTile + tid;
  uint64_t w = 0, len = 0;
  bool bad = false;
  if (g < r.n_groups) {
    smm_cpx::group_of(s, r, sec, g, &w, &len);
    bad = w > 32 || len > r.n_values;
    if (bad) w = len = 0;
  }
  const uint64_t bits = w * len;
  const uint64_t len_incl = block_scan<kCpxThreads>(len, lds, tid);
  const uint64_t bits_incl = block_scan<kCpxThreads>(bits, lds, tid);
  if (g < r.n_groups) a.groups[row.group_off + g] = CpxGroup{bits_incl - bits, (uint32_t)(len_incl - len), (uint32_t)w};
  if (tid == kCpxThreads - 1) {
    a.gtiles[row.gtile_off + tile] = CpxTile{len_incl, bits_incl};
    bad = bad || len_incl > r.n_values;
  }
  if (bad) atomicMax(&a.structure[j], (int32_t)smm_cpx::kInvalid);
}

// ---- offsets.  One wave per row: the tile sums become the sums before each tile; the row's totals are checked.
__global__ __launch_bounds__(kWave) void smm_grib_cpx_offsets_kernel(CpxArgs a, int64_t b0) {
  const int64_t j = b0 + blockIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const smm_cpx::Row& r = row.r;
  if (!row.coded || a.structure[j] != smm_cpx::kOk) return;   // every tile sum is <= n_values from here on
  const smm_cpx::Sections sec = smm_cpx::sections(r);
  const uint32_t n_tiles = (r.n_groups + kGroupTile - 1) / kGroupTile;
  CpxTile* __restrict__ tiles = a.gtiles + row.gtile_off;
  const CpxTile sum = scan_parts<CpxTile>(
      n_tiles, [&](uint32_t t) { return tiles[t]; }, [&](uint32_t t, CpxTile before) { tiles[t] = before; });
  if (threadIdx.x == 0) {
    if (sum.values != r.n_values)
      a.structure[j] = smm_cpx::kInvalid;
    else if (sum.bits > sec.bit_end - sec.data_bit)
      a.structure[j] = smm_cpx::kExhausted;
  }
}

// the largest X of a wave's lanes and whether one of them left [0, 2^32): one atomic per wave at most
__device__ __forceinline__ void raise_row(const CpxArgs& a, int64_t j, uint32_t m, bool high) {
#pragma unroll
  for (int o = kWave / 2; o > 0; o >>= 1) {
    const uint32_t t = __shfl_xor(m, o, kWave);
    m = t > m ? t : m;
  }
  const bool any_high = __any(high);
  if ((threadIdx.x & (kWave - 1)) == 0) {
    raise(&a.xmax[j], m);
    if (any_high) raise(&a.range[j], (int32_t)smm_cpx::kInvalid);   // kOk < kInvalid
  }
}

// ---- values.  Lane (row, i) finds the group of value i: the last tile whose value offset is <= i, then the last group
// of that tile whose offset is <= i -- groups of no values share their offset with the group behind them, and the last
// of equals is the one that holds i (the lengths sum to n_values > i).
struct CpxPlace {   // where value i of a row lies: its group, the group's width, the value's first bit in x
  uint32_t group, width;
  uint64_t bit;
};
__device__ __forceinline__ CpxPlace place_of(const CpxArgs& a, const CpxRow& row, const smm_cpx::Sections& sec, uint32_t i) {
  const smm_cpx::Row& r = row.r;
  const CpxTile* __restrict__ tiles = a.gtiles + row.gtile_off;
  const CpxGroup* __restrict__ groups = a.groups + row.group_off;
  uint32_t lo = 0, hi = (r.n_groups + kGroupTile - 1) / kGroupTile - 1;
  while (lo < hi) {
    const uint32_t mid = lo + (hi - lo + 1) / 2;
    if (tiles[mid].values <= i)
      lo = mid;
    else
      hi = mid - 1;
  }
  const CpxTile tile = tiles[lo];
  const uint32_t rest = i - (uint32_t)tile.values;   // tile.values <= i: tile 0 starts at 0
  uint32_t g0 = lo * kGroupTile, g1 = g0 + kGroupTile - 1;
  if (g1 > r.n_groups - 1) g1 = r.n_groups - 1;
  while (g0 < g1) {
    const uint32_t mid = g0 + (g1 - g0 + 1) / 2;
    if (groups[mid].value_excl <= rest)
      g0 = mid;
    else
      g1 = mid - 1;
  }
  const CpxGroup grp = groups[g0];
  const uint64_t k = rest - grp.value_excl;
  return CpxPlace{g0, grp.width, sec.data_bit + tile.bits + grp.bit_excl + k * grp.width};
}

__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_values_kernel(CpxArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t i = at.part * kCpxThreads + threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const smm_cpx::Row& r = row.r;
  if (!row.coded || row.mvm || a.structure[j] != smm_cpx::kOk) return;
  if ((uint64_t)at.part * kCpxThreads >= r.n_values) return;
  const bool live = i < r.n_values;
  uint64_t v = 0;
  if (live) {
    const smm_cpx::Sections sec = smm_cpx::sections(r);
    const smm_cpx::Stream s = smm_cpx::stream_of(a.x, r);
    uint64_t h1, h2, gmin;
    smm_cpx::descriptors(s, r, &h1, &h2, &gmin);
    if (i < (uint32_t)r.order) {
      v = smm_cpx::seed(i, h1, h2);
    } else {
      const CpxPlace p = place_of(a, row, sec, i);
      // the offsets kernel has checked that the row's bits end inside the stream; a width is at most 32
      v = smm_cpx::group_ref(s, r, sec, p.group) + s.peek(p.bit, (int)p.width) + gmin;
    }
    a.values[row.value_off + i] = v;
  }
  if (r.order <= 0) raise_row(a, j, live ? (uint32_t)v : 0u, live && (v >> 32) != 0);
}

// ---- rows with missing values inside the groups (mvm 1 or 2; the rule: smm_grib_cpx.hpp).  Three kernels stand in for
// the values kernel: values_mv, ranks, compact.  After them a.values holds a_0 .. a_(P-1) of the row's present values
// and a.present[j] holds P: the prefix sums, raise_row and the store run over P instead of n_values.
// values_mv: lane (row, i) extracts the stored value of POSITION i (no placeholder is skipped: they go by rank), decides
// whether it is present and leaves z + g in a.staged.  A wave's ballot is two words of the row's bitmap (bit i of the
// ballot is lane i, the bitmap wants position i as bit 31 - i of a big-endian word): lanes 0 and 32 store one each, a
// plain vector store.  The workgroup's present positions are counted through LDS.
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_values_mv_kernel(CpxArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t wave_count[kCpxThreads / kWave];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t i = at.part * kCpxThreads + threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const smm_cpx::Row& r = row.r;
  if (!row.coded || !row.mvm || a.structure[j] != smm_cpx::kOk) return;
  if ((uint64_t)at.part * kCpxThreads >= r.n_values) return;
  bool here = false;
  if (i < r.n_values) {
    const smm_cpx::Sections sec = smm_cpx::sections(r);
    const smm_cpx::Stream s = smm_cpx::stream_of(a.x, r);
    uint64_t h1, h2, gmin;
    smm_cpx::descriptors(s, r, &h1, &h2, &gmin);
    const CpxPlace p = place_of(a, row, sec, i);
    const uint64_t ref = smm_cpx::group_ref(s, r, sec, p.group), stored = s.peek(p.bit, (int)p.width);
    here = !smm_cpx::is_missing((int)row.mvm, p.width, r.nbits, ref, stored);
    a.staged[row.stage_off + i] = ref + stored + gmin;
  }
  const uint64_t mask = __ballot(here);
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  // word i / 32 of the bitmap slot: i < n_values keeps it inside the slot's ceil(n_values / 32) words; positions past
  // n_values are zero bits
  if ((lane & 31u) == 0u && i < r.n_values)
    a.out[(row.bm_off >> 2) + (i >> 5)] = __builtin_bswap32(__brev((uint32_t)(lane ? mask >> 32 : mask)));
  if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  if (threadIdx.x == 0) {
    uint32_t sum = 0;
    for (int w = 0; w < kCpxThreads / kWave; ++w) sum += wave_count[w];
    a.counts[row.block_off + at.part] = sum;
  }
}

// ranks: one wave per row.  The blocks' counts become the present positions before each block, their sum is P.
__global__ __launch_bounds__(kWave) void smm_grib_cpx_ranks_kernel(CpxArgs a, int64_t b0) {
  const int64_t j = b0 + blockIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  if (!row.coded || !row.mvm || a.structure[j] != smm_cpx::kOk) return;
  const uint32_t n_blocks = (row.r.n_values + kCpxThreads - 1) / kCpxThreads;
  uint32_t* __restrict__ counts = a.counts + row.block_off;
  const uint64_t sum = scan_parts<uint64_t>(
      n_blocks, [&](uint32_t t) { return (uint64_t)counts[t]; }, [&](uint32_t t, uint64_t before) { counts[t] = (uint32_t)before; });
  if (threadIdx.x == 0) a.present[j] = (uint32_t)sum;   // <= n_values
}

// compact: lane (row, i) reads its bit of the bitmap that values_mv stored; a present position's rank is the count
// before its block, before its wave in the block and before its lane in the wave's ballot.  a_rank goes to a.values:
// the seed for rank < order, else what a.staged holds for the position.  At order 0 this is the last pass over the row.
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_compact_kernel(CpxArgs a, int64_t b0, uint32_t per_row) {
  __shared__ uint32_t wave_count[kCpxThreads / kWave];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t i = at.part * kCpxThreads + threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const smm_cpx::Row& r = row.r;
  if (!row.coded || !row.mvm || a.structure[j] != smm_cpx::kOk) return;
  if ((uint64_t)at.part * kCpxThreads >= r.n_values) return;
  bool here = false;
  if (i < r.n_values) {
    const uint32_t word = __builtin_bswap32(a.out[(row.bm_off >> 2) + (i >> 5)]);
    here = ((word >> (31u - (i & 31u))) & 1u) != 0u;
  }
  const uint64_t mask = __ballot(here);
  const uint32_t lane = threadIdx.x & (kWave - 1), wave = threadIdx.x / kWave;
  if (lane == 0u) wave_count[wave] = (uint32_t)__popcll(mask);
  __syncthreads();
  uint32_t rank = a.counts[row.block_off + at.part];
  for (uint32_t w = 0; w < wave; ++w) rank += wave_count[w];
  rank += (uint32_t)__popcll(mask & (((uint64_t)1 << lane) - 1));
  uint64_t v = 0;
  if (here) {   // rank < P <= n_values: inside the row's values
    if (rank < (uint32_t)r.order) {
      const smm_cpx::Stream s = smm_cpx::stream_of(a.x, r);
      uint64_t h1, h2, gmin;
      smm_cpx::descriptors(s, r, &h1, &h2, &gmin);
      v = smm_cpx::seed(rank, h1, h2);
    } else {
      v = a.staged[row.stage_off + i];
    }
    a.values[row.value_off + rank] = v;
  }
  if (r.order <= 0) raise_row(a, j, here ? (uint32_t)v : 0u, here && (v >> 32) != 0);
}

// the values the prefix sums and the store run over: P of a row with mvm != 0 (written by the ranks kernel)
__device__ __forceinline__ uint32_t values_of(const CpxArgs& a, const CpxRow& row, int64_t j) {
  return row.mvm ? a.present[j] : row.r.n_values;
}

// ---- the prefix sums of order 1 and 2; pass p (1 or 2) runs on the rows whose order is >= p
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_reduce_kernel(CpxArgs a, int64_t b0, uint32_t per_row, int pass) {
  __shared__ uint64_t lds[kCpxThreads];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part, tid = threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const uint32_t n = values_of(a, row, j);
  if (!row.coded || row.r.order < pass || a.structure[j] != smm_cpx::kOk || (uint64_t)tile * kValueTile >= n) return;
  const uint64_t* __restrict__ v = a.values + row.value_off;
  uint64_t sum = 0;
#pragma unroll
  for (int q = 0; q < kPerLane; ++q) {
    const uint64_t i = (uint64_t)tile * kValueTile + (uint64_t)q * kCpxThreads + tid;
    if (i < n) sum += v[i];
  }
  const uint64_t incl = block_scan<kCpxThreads>(sum, lds, tid);
  if (tid == kCpxThreads - 1) a.vtiles[row.vtile_off + tile] = incl;
}

__global__ __launch_bounds__(kWave) void smm_grib_cpx_carries_kernel(CpxArgs a, int64_t b0, int pass) {
  const int64_t j = b0 + blockIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  if (!row.coded || row.r.order < pass || a.structure[j] != smm_cpx::kOk) return;
  const uint32_t n_tiles = (values_of(a, row, j) + kValueTile - 1) / kValueTile;
  uint64_t* __restrict__ tiles = a.vtiles + row.vtile_off;
  (void)scan_parts<uint64_t>(
      n_tiles, [&](uint32_t t) { return tiles[t]; }, [&](uint32_t t, uint64_t before) { tiles[t] = before; });
}

// lane tid owns the 4 consecutive values from 1024 tile + 4 tid on
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_apply_kernel(CpxArgs a, int64_t b0, uint32_t per_row, int pass) {
  __shared__ uint64_t lds[kCpxThreads];
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const uint32_t tile = at.part, tid = threadIdx.x;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  const uint32_t n = values_of(a, row, j);
  if (!row.coded || row.r.order < pass || a.structure[j] != smm_cpx::kOk || (uint64_t)tile * kValueTile >= n) return;
  uint64_t* __restrict__ v = a.values + row.value_off;
  const uint64_t first = (uint64_t)tile * kValueTile + (uint64_t)tid * kPerLane;
  uint64_t mine[kPerLane];
  uint64_t sum = 0;
#pragma unroll
  for (int q = 0; q < kPerLane; ++q) {
    mine[q] = first + q < n ? v[first + q] : 0;
    sum += mine[q];
    mine[q] = sum;
  }
  const uint64_t before = a.vtiles[row.vtile_off + tile] + block_scan<kCpxThreads>(sum, lds, tid) - sum;
  const bool last = pass == row.r.order;
  uint32_t m = 0;
  bool high = false;
#pragma unroll
  for (int q = 0; q < kPerLane; ++q) {
    const uint64_t X = before + mine[q];
    if (first + q < n) {
      v[first + q] = X;
      m = (uint32_t)X > m ? (uint32_t)X : m;
      high = high || (X >> 32) != 0;
    }
  }
  if (last) raise_row(a, j, m, high);
}

// ---- store.  One thread per 32-bit word of the row's stream at its own width (the grid covers 32 bits a value; the
// surplus threads leave), the values that overlap the word put in place as smm_grib_codec.hpp's grib_word_part has it.
__global__ __launch_bounds__(kCpxThreads) void smm_grib_cpx_store_kernel(CpxArgs a, int64_t b0, uint32_t per_row) {
  const RowPart at = row_part(b0, per_row);
  const int64_t j = at.j;
  const CpxRow* __restrict__ rows = a.rows;
  const CpxRow row = rows[j];
  if (!row.coded || a.structure[j] != smm_cpx::kOk || a.range[j] != smm_cpx::kOk) return;
  const uint64_t* __restrict__ v = a.values + row.value_off;
  // the row's words are at most n_values: inside the slot
  store_row_word(a.out, row.out_off, at.part * kCpxThreads + threadIdx.x, smm_cpx::width_of(a.xmax[j]), values_of(a, row, j),
                 [&](uint64_t i) { return (uint32_t)v[i]; });
}

struct CpxShape {   // the widest row of the call
  uint32_t gtiles = 0, vtiles = 0, blocks = 0;
  int order = 0;
  bool plain = false, mv = false;   // some row with mvm == 0, some row with mvm != 0
};

int launch_cpx(const CpxArgs& a, int64_t n_j, const CpxShape& sh, hipStream_t s) {
  if (int rc = launch_flat(smm_grib_cpx_groups_kernel, kCpxThreads, n_j * sh.gtiles, s, a, sh.gtiles)) return rc;
  if (int rc = launch_flat(smm_grib_cpx_offsets_kernel, kWave, n_j, s, a)) return rc;
  if (sh.plain)
    if (int rc = launch_flat(smm_grib_cpx_values_kernel, kCpxThreads, n_j * sh.blocks, s, a, sh.blocks)) return rc;
  if (sh.mv) {
    if (int rc = launch_flat(smm_grib_cpx_values_mv_kernel, kCpxThreads, n_j * sh.blocks, s, a, sh.blocks)) return rc;
    if (int rc = launch_flat(smm_grib_cpx_ranks_kernel, kWave, n_j, s, a)) return rc;
    if (int rc = launch_flat(smm_grib_cpx_compact_kernel, kCpxThreads, n_j * sh.blocks, s, a, sh.blocks)) return rc;
  }
  for (int pass = 1; pass <= sh.order; ++pass) {
    if (int rc = launch_flat(smm_grib_cpx_reduce_kernel, kCpxThreads, n_j * sh.vtiles, s, a, sh.vtiles, pass)) return rc;
    if (int rc = launch_flat(smm_grib_cpx_carries_kernel, kWave, n_j, s, a, pass)) return rc;
    if (int rc = launch_flat(smm_grib_cpx_apply_kernel, kCpxThreads, n_j * sh.vtiles, s, a, sh.vtiles, pass)) return rc;
  }
  return launch_flat(smm_grib_cpx_store_kernel, kCpxThreads, n_j * sh.blocks, s, a, sh.blocks);
}

// everything the entries with records refuse about them
int check_cpx_records(const smm_grib_cpx_t* recs, int64_t n_batch, int64_t x_bytes) {
  if (n_batch < 0) return fail(SMM_ERR_INVALID, "negative batch size");
  if (x_bytes < 0) return fail(SMM_ERR_INVALID, "negative x_bytes");
  if (!recs && n_batch > 0) return fail(SMM_ERR_INVALID, "null record pointer");
  std::string err;
  if (!smm::check_grib_cpx(recs, n_batch, x_bytes, err)) return fail(SMM_ERR_INVALID, err);
  return SMM_OK;
}

const char* status_text(int status) {
  return status == smm_cpx::kExhausted ? "ends before its tables or its groups' bits do"
                                       : "is invalid (a group wider than 32 bits, group lengths that do not sum to "
                                         "n_values, or an integer outside [0, 2^32))";
}

// mvm: null, or a row's missing value management; bm_offs: the rows' bitmap slots (smm::grib_cpx_layout_mv);
// bitmaps_out: null (smm_grib_cpx_unpack), or what the gather needs to know of them
int smm_grib_cpx_unpack_impl(int device, const void* x, const smm_grib_cpx_t* recs, const uint8_t* mvm,
                             const smm_grib_row_t* rows_in, int64_t n_batch, void* out, const uint64_t* offs,
                             const uint64_t* bm_offs, smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out, void* stream) {
  const size_t n = (size_t)n_batch;
  std::vector<CpxRow> table(n);
  std::vector<int32_t> words(4 * n, 0);   // structure, range, xmax, present
  uint64_t n_groups = 0, n_gtiles = 0, n_values = 0, n_vtiles = 0, n_staged = 0, n_blocks = 0;
  CpxShape sh;
  for (size_t b = 0; b < n; ++b) {
    const smm_grib_cpx_t& c = recs[b];
    CpxRow& r = table[b];
    r = CpxRow{smm_cpx::row_of(c), n_groups, n_gtiles, n_values, n_vtiles, offs[b], 0u, 0u, 0, n_staged, n_blocks};
    rows_out[b] = rows_in[b];
    if (bitmaps_out) bitmaps_out[b] = smm_grib_bitmap_t{SMM_GRIB_NO_BITMAP, c.n_values};
    if (c.order == SMM_GRIB_CPX_SIMPLE) continue;
    rows_out[b].byte_off = offs[b];
    rows_out[b].nbits = 0;
    if (mvm && mvm[b] != 0) {
      r.mvm = mvm[b];
      r.bm_off = bm_offs[b];
      bitmaps_out[b] = smm_grib_bitmap_t{bm_offs[b], 0};
    }
    if (c.n_values == 0) continue;
    r.coded = 1u;
    const smm_cpx::Sections sec = smm_cpx::sections(r.r);
    words[b] = sec.status;
    if (sec.status != smm_cpx::kOk) continue;   // n_groups <= n_values from here on: the record bounds the scratch
    const uint32_t gt = (uint32_t)((c.n_groups + (uint64_t)kGroupTile - 1) / kGroupTile);
    const uint32_t vt = (uint32_t)((c.n_values + (uint64_t)kValueTile - 1) / kValueTile);
    n_groups += c.n_groups;
    n_gtiles += gt;
    n_values += c.n_values;
    n_vtiles += vt;
    sh.gtiles = std::max(sh.gtiles, gt);
    sh.vtiles = std::max(sh.vtiles, vt);
    sh.blocks = std::max(sh.blocks, (uint32_t)((c.n_values + (uint64_t)kCpxThreads - 1) / kCpxThreads));
    sh.order = std::max(sh.order, (int)c.order);
    if (r.mvm) {
      n_staged += c.n_values;
      n_blocks += (c.n_values + (uint64_t)kCpxThreads - 1) / kCpxThreads;
      sh.mv = true;
    } else {
      sh.plain = true;
    }
  }
  std::vector<int32_t> got(words);
  if (n_values > 0) {
    Arena arena;
    const size_t table_at = arena.add<CpxRow>(n), words_at = arena.add<int32_t>(4 * n), groups_at = arena.add<CpxGroup>(n_groups),
                 gtiles_at = arena.add<CpxTile>(n_gtiles), values_at = arena.add<uint64_t>(n_values), vtiles_at = arena.add<uint64_t>(n_vtiles),
                 staged_at = arena.add<uint64_t>(n_staged), counts_at = arena.add<uint32_t>(n_blocks);
    if (int rc = run_transcode(
            device, stream, arena.bytes(),
            {Span{table_at, table.data(), n * sizeof(CpxRow)}, Span{words_at, words.data(), 4 * n * sizeof(int32_t)}},
            [&](char* d, hipStream_t s) {
              int32_t* w = Arena::at<int32_t>(d, words_at);
              const CpxArgs a{x, Arena::at<CpxRow>(d, table_at), Arena::at<CpxGroup>(d, groups_at), Arena::at<CpxTile>(d, gtiles_at),
                              Arena::at<uint64_t>(d, values_at), Arena::at<uint64_t>(d, vtiles_at), (uint32_t*)out, w, w + n,
                              (uint32_t*)(w + 2 * n), (uint32_t*)(w + 3 * n), Arena::at<uint64_t>(d, staged_at),
                              Arena::at<uint32_t>(d, counts_at)};
              return launch_cpx(a, n_batch, sh, s);
            },
            Span{words_at, got.data(), 4 * n * sizeof(int32_t)}, "statuses"))
      return rc;
  }
  for (size_t b = 0; b < n; ++b) {
    const int status = got[b] != smm_cpx::kOk ? got[b] : got[n + b];
    if (status != smm_cpx::kOk)
      return fail(SMM_ERR_INVALID, "recs[" + std::to_string(b) + "]: the complex-packed stream " + status_text(status));
    if (table[b].coded) rows_out[b].nbits = smm_cpx::width_of((uint32_t)got[2 * n + b]);
    if (table[b].mvm) bitmaps_out[b].n_values = (uint32_t)got[3 * n + b];
  }
  return SMM_OK;
}

// the body of smm_grib_cpx_unpack (mvm and bitmaps_out null, with_bitmaps false) and smm_grib_cpx_unpack_mv
int unpack_entry(int device, const void* x, int64_t x_bytes, const smm_grib_cpx_t* recs, const uint8_t* mvm,
                 const smm_grib_row_t* rows_in, int64_t n_batch, void* out, int64_t out_bytes, smm_grib_row_t* rows_out,
                 smm_grib_bitmap_t* bitmaps_out, bool with_bitmaps, void* stream) {
  if (int rc = check_cpx_records(recs, n_batch, x_bytes)) return rc;
  std::string err;
  if (!smm::check_grib_cpx_mvm(mvm, n_batch, err)) return fail(SMM_ERR_INVALID, err);
  if (with_bitmaps && n_batch > 0 && !bitmaps_out) return fail(SMM_ERR_INVALID, "null bitmap-table pointer");
  std::vector<uint64_t> offs, bm_offs((size_t)n_batch);
  if (int rc = check_unpack_call(
          x, recs, rows_in, n_batch, out, out_bytes, rows_out, offs,
          [&](const smm_grib_cpx_t* r, int64_t n, uint64_t* at) { return smm::grib_cpx_layout_mv(r, mvm, n, at, bm_offs.data()); },
          [](int64_t) { return (int)SMM_OK; }))
    return rc;
  return smm_grib_cpx_unpack_impl(device, x, recs, mvm, rows_in, n_batch, out, offs.data(), bm_offs.data(), rows_out, bitmaps_out,
                                  stream);
}

}  // namespace

extern "C" {

int smm_grib_cpx_layout(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes) {
  return offsets_entry(
      recs, n_batch, byte_off, total_bytes, [](const smm_grib_cpx_t* r, int64_t n) { return check_cpx_records(r, n, INT64_MAX); },
      smm::grib_cpx_layout);
}

int smm_grib_cpx_unpack(int device, const void* x, int64_t x_bytes, const smm_grib_cpx_t* recs, const smm_grib_row_t* rows_in,
                        int64_t n_batch, void* out, int64_t out_bytes, smm_grib_row_t* rows_out, void* stream) {
  return guarded([&] {
    return unpack_entry(device, x, x_bytes, recs, nullptr, rows_in, n_batch, out, out_bytes, rows_out, nullptr, false, stream);
  });
}

int smm_grib_cpx_decode_host(const void* x_host, int64_t x_bytes, const smm_grib_cpx_t* rec, uint32_t* values, int* status) {
  return guarded([&] {
    if (!rec || !status) return fail(SMM_ERR_INVALID, "null record or status pointer");
    if (int rc = check_cpx_records(rec, 1, x_bytes)) return rc;
    if (rec->order == SMM_GRIB_CPX_SIMPLE) return fail(SMM_ERR_INVALID, "rec is marked simple-packed: it has no complex-packed stream");
    if (rec->n_values > 0 && !values) return fail(SMM_ERR_INVALID, "null values pointer");
    if (!x_host && rec->byte_len > 0) return fail(SMM_ERR_INVALID, "null field pointer");
    *status = smm_cpx::decode_row(x_host, smm_cpx::row_of(*rec), values);
    return (int)SMM_OK;
  });
}

int smm_grib_cpx_layout_mv(const smm_grib_cpx_t* recs, const uint8_t* mvm, int64_t n_batch, uint64_t* byte_off,
                           uint64_t* bitmap_off, uint64_t* total_bytes) {
  return offsets_entry(
      recs, n_batch, byte_off, total_bytes,
      [&](const smm_grib_cpx_t* r, int64_t n) {
        if (int rc = check_cpx_records(r, n, INT64_MAX)) return rc;
        std::string err;
        return smm::check_grib_cpx_mvm(mvm, n, err) ? (int)SMM_OK : fail(SMM_ERR_INVALID, err);
      },
      [&](const smm_grib_cpx_t* r, int64_t n, uint64_t* at) { return smm::grib_cpx_layout_mv(r, mvm, n, at, bitmap_off); });
}

int smm_grib_cpx_unpack_mv(int device, const void* x, int64_t x_bytes, const smm_grib_cpx_t* recs, const uint8_t* mvm,
                           const smm_grib_row_t* rows_in, int64_t n_batch, void* out, int64_t out_bytes, smm_grib_row_t* rows_out,
                           smm_grib_bitmap_t* bitmaps_out, void* stream) {
  return guarded([&] {
    return unpack_entry(device, x, x_bytes, recs, mvm, rows_in, n_batch, out, out_bytes, rows_out, bitmaps_out, true, stream);
  });
}

int smm_grib_cpx_decode_host_mv(const void* x_host, int64_t x_bytes, const smm_grib_cpx_t* rec, const uint8_t* mvm,
                                uint32_t* values, uint8_t* present, uint64_t* n_present, int* status) {
  return guarded([&] {
    if (!rec || !status || !n_present) return fail(SMM_ERR_INVALID, "null record, count or status pointer");
    if (int rc = check_cpx_records(rec, 1, x_bytes)) return rc;
    std::string err;
    if (!smm::check_grib_cpx_mvm(mvm, 1, err)) return fail(SMM_ERR_INVALID, err);
    if (rec->order == SMM_GRIB_CPX_SIMPLE) return fail(SMM_ERR_INVALID, "rec is marked simple-packed: it has no complex-packed stream");
    if (rec->n_values > 0 && (!values || !present)) return fail(SMM_ERR_INVALID, "null values or flags pointer");
    if (!x_host && rec->byte_len > 0) return fail(SMM_ERR_INVALID, "null field pointer");
    *status = smm_cpx::decode_row_mv(x_host, smm_cpx::row_of(*rec), mvm ? (int)*mvm : 0, values, present, n_present);
    return (int)SMM_OK;
  });
}

}  // extern "C"
