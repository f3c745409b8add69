// GRIB simple-packed fields regridded raw (smm_apply_grib): the kernel's arguments and its launcher, which is compiled
// in an object of its own (smm_grib.hip).  The kernel is kernel A (smm_kernels.hpp: SELL-64, one destination row per
// lane, BT batch rows register-blocked) with the X access replaced by the bit extraction and decode of smm_grib_codec.hpp.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

#include "../../include/smmregrid_amd.h"
#include "smm_grib_codec.hpp"
#include "smm_kernels.hpp"

struct GribArgs {
  const LevelDesc* descs;        // device, one element: the operator's SELL layout and epilogue vectors
  const uint32_t* x;             // device: the packed bytes as 32-bit words (4-byte aligned)
  const smm_grib_row_t* rows;    // device [n_j]: where batch row j starts in x and how it decodes
  double* y;                     // device: row j at y + j * ldy
  int64_t ldy, n_j, n_dblocks, n_jtiles, n_dst;
  uint64_t last_word;            // index of the last word of x: no load goes past it
  double area_min;
  int masked;
};

// smm_apply_grib_bm (GribRowBitmap: smm_grib_codec.hpp)
struct GribBitmapArgs : GribArgs {
  const GribRowBitmap* bm;                 // device [n_j], parallel to rows
  const smm_grib::GribRankEntry* table;    // device: the rank tables of the call's bitmapped rows
};
// smm_group_apply_grib: one launch over the data levels of a group.  descs holds the group's members, lev_map[l] names
// the member of the launch's level l and lev_masked[member] its mask switch (null: every member masks) -- the group's
// cfg_cache upload.  n_j = n_o * n_inner batch rows PER LEVEL; row (o, l, i) of the launch is record
// o * rec_o + l * rec_l + i of rows / bm (the launch's first record at rows[0]: a part of a call advances the pointers)
// and writes y + o * ys_o + l * ys_l + i * ys_i, all in 64-bit arithmetic.  ldy is unused; bm / table are null when no
// row of the call has a bitmap (the BM = false instantiations).
struct GribGroupArgs : GribBitmapArgs {
  const int32_t* lev_map;
  const uint8_t* lev_masked;
  int64_t n_inner, rec_o, rec_l;
  int64_t ys_o, ys_l, ys_i;
};
// the table build: n_j rows of n_src cells over the words of x.  Every table has n_blocks entries, so table_off / n_blocks
// numbers the tables: totals[(that number) * n_segs + s] = set bits of segment s
struct GribBuildArgs {
  const uint32_t* x;
  const GribRowBitmap* bm;
  smm_grib::GribRankEntry* table;
  uint32_t* totals;
  uint64_t last_word;
  int64_t n_j;
  uint32_t n_src, n_blocks, n_segs;
};

// smm_grib_pack / smm_apply_host_grib_pk: float64 results into GRIB simple packing (the rule: smm_grib_codec.hpp).
// What a row of the call brings to the device
struct GribPackRow {     // 32 B
  double ddiv;
  uint64_t slot_off;     // of the row's slot -- bitmap part, then stream part -- from `out`; a multiple of 4
  uint64_t pub_off;      // the same place as the records report it: the slot's offset in the caller's buffer
  int32_t nbits;         // the requested width, 1..32
  int32_t pad;
};
struct GribPackArgs {
  const double* y;                // device: row j at y + j * ldy
  int64_t ldy, n_j;
  uint32_t n_dst, n_blocks, n_segs;   // cells, 32-cell blocks and kGribSegBlocks-block segments of a row
  uint32_t max_words;             // stream words of the widest row: the pack grid covers that many per row
  const GribPackRow* rows;        // device [n_j]
  uint32_t* out;                  // device: the slots, as 32-bit words
  double* part_min;               // device scratch [n_j * n_segs] each: the segments' tmin / tmax / present cells
  double* part_max;
  uint32_t* part_cnt;
  smm_grib::GribPackRule* rules;  // device [n_j]: what the rule pass leaves for the pack
  smm_grib_row_t* rec_rows;       // device [n_j]: the records of the result as the caller gets them
  smm_grib_bitmap_t* rec_bm;      // device [n_j]
  const smm_grib::GribRankEntry* table;   // device: row j's rank table at table + j * n_blocks (launch_grib_build)
};

namespace smm_launch {
// the four steps of a pack in stream order: range + bitmap, rule, the rank tables of the bitmaps just written
// (launch_grib_build over `build`: x = a.out, one table per row), pack.  limit: the largest launch grid (rows are
// launched in parts beyond it)
int launch_grib_pack(const GribPackArgs& a, const GribBuildArgs& build, int64_t limit, hipStream_t s);
// div: some row of the call has ddiv != 1.0 (the instantiation with the f64 division); na: the SMM_APPLY_SKIPNA rule
// (the NA instantiations, which take the values raw whatever fill says); fill: the 1e20 fill is on
int launch_grib(const GribArgs& a, bool div, bool na, bool fill, hipStream_t s);
// the gather that consults the rank tables (rows without a bitmap take rank = c on a block-uniform branch) ...
int launch_grib_bitmap(const GribBitmapArgs& a, bool div, bool na, bool fill, hipStream_t s);
// the grouped gather over n_lev levels (grid = destination blocks x batch tiles x levels); bitmaps: a.bm / a.table are set
int launch_grib_group(const GribGroupArgs& a, int64_t n_lev, bool bitmaps, bool div, bool na, bool fill, hipStream_t s);
// ... and the two kernels that fill the rank tables, in stream order ahead of it: segment totals, then the scan
int launch_grib_build(const GribBuildArgs& a, hipStream_t s);
}
