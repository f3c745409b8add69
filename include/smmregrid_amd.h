/*
 * smmregrid_amd.h -- C ABI of libsmmregrid_hip.so (MI355X / gfx950).
 *
 * This library replaces the third-party arithmetic that the reference
 * (jhardenberg/smmregrid) invokes on its hot path -- the seam is
 *
 *   weights.py:25-44   compute_weights_matrix     sparse.COO([src,dst], w, (S,D))
 *   weights.py:7-23    compute_weights_matrix3d   one COO per level, links[:link_length]
 *   weights.py:47-52   mask_tensordot             (src_imask . W) < 0.5 ? 0 : 1
 *   regrid.py:545-547  non-finite -> 1e20 fill of the source array
 *   regrid.py:550      dask.array.tensordot(X(B,S), W(S,D), axes=1)
 *   regrid.py:553-570  where(dst_imask) / where(frac < remap_area_min) / where(> 1e19)
 *   regrid.py:387-418  regrid3d level loop + concat (+ transpose)
 *
 * The reference is pure Python: a maintainer binds this ABI with ctypes
 * (see INTEGRATION.md for the stub). No torch / C++ types cross the boundary:
 * plain pointers, sizes and opaque handles only.
 *
 * Conventions
 *   - every function returns an int status (SMM_OK == 0); it never throws.
 *     The message of the last failure on the calling thread is returned by
 *     smm_last_error().
 *   - "host" pointers are ordinary process memory, borrowed for the call only.
 *     "device" pointers are HBM addresses (from smm_malloc or any hipMalloc).
 *   - operator handles are immutable once their epilogue vectors are set;
 *     smm_apply* is re-entrant on them (the reference's dask scheduler calls
 *     one matrix from several threads, regrid.py:29-30).
 *   - there is NO CPU fallback in this library: without a HIP device every
 *     compute entry point fails with SMM_ERR_NO_DEVICE.
 */
#ifndef SMMREGRID_AMD_H
#define SMMREGRID_AMD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define SMM_ABI_VERSION 6

/* status codes */
enum {
  SMM_OK = 0,
  SMM_ERR_INVALID = 1,    /* bad argument (address out of range, negative size, ...) */
  SMM_ERR_NO_DEVICE = 2,  /* no HIP device / device ordinal out of range            */
  SMM_ERR_HIP = 3,        /* a HIP runtime call failed (message has the hipError)    */
  SMM_ERR_ALLOC = 4,      /* host allocation failed                                  */
  SMM_ERR_UNSUPPORTED = 5,/* dtype / flag combination not built                      */
  SMM_ERR_INTERNAL = 6    /* an unexpected failure inside the library (message says what) */
};

/* element types of the dense field buffers */
enum {
  SMM_F32 = 0,
  SMM_F64 = 1,
  SMM_I16 = 2,  /* CF-packed fields: X through the _cf entries below, Y through the _pk entries (every other entry: SMM_ERR_UNSUPPORTED) */
  SMM_U16 = 3
};
/* half-precision element types, the codes that follow SMM_U16 (rule below) */
enum {
  SMM_F16 = SMM_U16 + 1,  /* 4: IEEE binary16, X and Y of the plain entries */
  SMM_BF16 = SMM_U16 + 2  /* 5: bfloat16, the same */
};

/* Half-precision fields and results (SMM_F16 / SMM_BF16), valid as x_dtype and y_dtype of the plain entries --
 * smm_apply, smm_apply_sb, smm_apply_host, smm_group_apply, smm_group_apply_sb, smm_group_apply_host -- and as
 * x_dtype of the two *_launch_info entries.  Elements are 2 bytes, pointers 2-byte aligned, strides in elements.
 *   Half X: an element is widened exactly to float32 in registers and from there treated exactly as an element of a
 *     float32 field (fill float32(1e20), promotion f32 -> f64, plain or SMM_APPLY_SKIPNA epilogue): the result bits are
 *     those of the float32 entry on the widened field.  NaN, +-inf and subnormals are not special-cased and nothing is
 *     flushed to zero.
 *   Half Y: the float64 value v the epilogue produces (after the > 1e19 -> NaN test, the mask and dst_frac) is stored
 *     with ONE correctly rounded conversion, ties to even, never through float32.  Overflow becomes +-inf, subnormal
 *     results are kept, NaN is stored as the canonical quiet NaN (0x7E00 / 0x7FC0).
 *   Built pairs (x -> y), each plain and with SMM_APPLY_SKIPNA, kernel 0 and the batch-fastest kernels (the LDS tile
 *     kernel is not built for them: SMM_APPLY_KERNEL_TILE is SMM_ERR_UNSUPPORTED):
 *       F16 -> F64, F16 -> F16, BF16 -> F64, BF16 -> BF16, F32 -> F16, F64 -> F16, F32 -> BF16, F64 -> BF16
 *     any other pair with a half type is SMM_ERR_UNSUPPORTED; a half type in a call that carries a decode or an encode
 *     rule (the _cf / _pk entries) is SMM_ERR_INVALID. */

/* CF "packed data" (scale_factor / add_offset / _FillValue / missing_value): how a raw int16 / uint16 element q
 * becomes a field value, with T = float (decode_dtype SMM_F32) or double (SMM_F64):
 *     v = (T)q;  v = v * (T)scale;  v = v + (T)offset;        two rounded operations, never an FMA
 *     if (q == fill[0] || q == fill[1])  v = NaN;              the first n_fill entries, compared on the raw integer
 * v then takes the place of an element of a T-typed field (1e20 fill of non-finite values, SMM_APPLY_SKIPNA
 * validity, ...): the results are bit-identical to decoding on the host in type T and calling the plain entry with
 * the same flags.  An absent scale / offset is 1 / 0.  Fill values must be representable in the raw type. */
typedef struct smm_cf_decode_t {
  double scale, offset;
  int32_t fill[2];
  int n_fill;        /* 0, 1 or 2 */
  int decode_dtype;  /* SMM_F32 or SMM_F64 */
} smm_cf_decode_t;

/* CF-packed RESULTS (the _pk entries): how a float64 result v becomes a raw element q of y_dtype SMM_I16 / SMM_U16,
 * always in float64 arithmetic:
 *     t = (v - offset) / scale;                                 two rounded operations, IEEE division (no reciprocal)
 *     r = rint(t);                                              ties to even
 *     q = (!isfinite(v) || r < MIN || r > MAX) ? fill : (raw type)r
 * NaN results (masked cells, fills, remap_area_min) and values that round outside the raw range become `fill`: there
 * is no wrap-around and no saturation.  A valid value that rounds onto `fill` is stored as is.  The stored bits are
 * those of the same rule applied on the host to the float64 result of the plain / _cf entry.  An absent scale /
 * offset is 1 / 0; scale must be finite and non-zero, offset finite, fill representable in the raw type, reserved 0. */
typedef struct smm_cf_encode_t {
  double scale, offset;
  int32_t fill;
  int32_t reserved;  /* 0 */
} smm_cf_encode_t;

/* GRIB simple packing (smm_apply_grib / smm_apply_host_grib): the data section of a message goes to the kernel as it
 * is on disk and is unpacked there.  One rule per batch row -- a row is one GRIB field, with its own R, E, D and bit
 * width.  Element i of row b is the unsigned big-endian integer q of `nbits` bits at bit position
 * 8 * byte_off + i * nbits of x (any byte alignment, any width 0..32), and becomes a field value in float64:
 *     t = (double)q * bscale;                                   exact (bscale is a power of two)
 *     t = ref + t;                                              one rounding
 *     t = t / ddiv;                                             IEEE division; skipped, with the same bits, when ddiv == 1.0
 *     v = (float)t;                                             round to nearest even, subnormals kept
 * v then takes the place of an element of a float32 field (fill float32(1e20) for a non-finite v, promotion f32 -> f64,
 * the plain epilogue): the results are bit-identical to smm_apply with SMM_F32 X on the field decoded on the host by
 * (ref + q * 2^E) / 10.0^D in float64 and stored as float32.  nbits == 0 is a constant field (q = 0, no bits read). */
typedef struct smm_grib_row_t {   /* one batch row = one GRIB field, 40 B */
  uint64_t byte_off;  /* of the row's first packed value, from x */
  double ref;         /* R widened to double (IBM float of edition 1, IEEE f32 of edition 2) */
  double bscale;      /* 2^E, exactly a power of two in the normal range */
  double ddiv;        /* 10.0^D as the host computes it; finite, > 0 */
  int32_t nbits;      /* 0..32; 0 = constant field, no bits read */
  int32_t reserved;   /* 0 */
} smm_grib_row_t;

/* A GRIB field with a bitmap (smm_apply_grib_bm / smm_apply_host_grib_bm): one record per batch row, parallel to the
 * row table.  The packed stream of such a row holds the present cells only: the value of grid cell c is packed value
 * number rank(c), the count of set bitmap bits before c; a cell whose bit is 0 is a float32 NaN. */
#define SMM_GRIB_NO_BITMAP UINT64_MAX
typedef struct smm_grib_bitmap_t {   /* 16 B */
  uint64_t bitmap_off;   /* byte offset in x of the row's bitmap: bit i (MSB first) of the stream says whether grid
                            cell i has a value; SMM_GRIB_NO_BITMAP (UINT64_MAX): the row has none, every cell present */
  uint64_t n_values;     /* values in the row's packed stream = set bits among the first n_src; n_src without a bitmap */
} smm_grib_bitmap_t;

/* How one float64 result row goes back into GRIB simple packing (smm_grib_pack / smm_apply_host_grib_pk): the width
 * asked for and 10^D.  The row's reference value and binary scale follow from its own minimum and maximum:
 *     t = v * ddiv;                                             one rounding
 *     present iff v is finite and |t| <= FLT_MAX;               NaN, +-inf and overflow are missing cells
 *     R = the largest float32 <= min t;  ref = (double)R + 0.0; edition 2's IEEE reference value (-0 stored as +0)
 *     range = max t - ref;                                      one rounding
 *     E = the smallest integer with range * 2^-E <= 2^nbits - 1, at least -1022;  bscale = 2^E
 *     q = rint(ldexp(t - ref, -E));                             ties to even; 0 <= q <= 2^nbits - 1
 * A row whose range is 0 or that has no present cell is stored with width 0 (ref = 0 for the empty row).  These are not
 * the bits ecCodes would choose (it picks E by heuristics of its own); it is a valid simple packing that the decode above
 * inverts.  The text of the rule is smmregrid_amd/csrc/smm_grib_codec.hpp; smmregrid_amd.GribEncode states it in numpy. */
typedef struct smm_grib_encode_t {   /* 16 B */
  double ddiv;        /* 10.0^D as the host computes it; finite, > 0 */
  int32_t nbits;      /* 1..32 */
  int32_t reserved;   /* 0 */
} smm_grib_encode_t;

/* A GRIB-2 field in CCSDS packing (data representation template 5.42; smm_grib_aec_unpack, smm_grib_aec_decode_host):
 * where the adaptive-entropy-coded stream of one batch row lies in x and the parameters it was written with.  The
 * stream decodes to n_values unsigned integers of nbits bits -- the q of smm_grib_row_t's rule.  flags are the
 * message's ccsdsFlags octet as it is (libaec's AEC_* bits): SMM_GRIB_AEC_PREPROCESS switches the unit-delay predictor
 * on; SMM_GRIB_AEC_MSB and SMM_GRIB_AEC_3BYTE describe the encoder's sample container, not the stream, and are
 * ignored; SMM_GRIB_AEC_SIGNED, SMM_GRIB_AEC_RESTRICTED, SMM_GRIB_AEC_PAD_RSI and every other bit are refused. */
enum {
  SMM_GRIB_AEC_SIGNED = 1u << 0,
  SMM_GRIB_AEC_3BYTE = 1u << 1,
  SMM_GRIB_AEC_MSB = 1u << 2,
  SMM_GRIB_AEC_PREPROCESS = 1u << 3,
  SMM_GRIB_AEC_RESTRICTED = 1u << 4,
  SMM_GRIB_AEC_PAD_RSI = 1u << 5
};
typedef struct smm_grib_aec_t {   /* one batch row = one GRIB field, 48 B */
  uint64_t byte_off;    /* of the stream's first byte, from x */
  uint64_t byte_len;    /* bytes of the stream */
  uint64_t n_values;    /* samples the stream codes: the grid's points, or the set bits of the row's bitmap; < 2^31 */
  int32_t nbits;        /* 0..32; 0 = constant field, no stream (block_size, rsi and flags are not looked at) */
  int32_t block_size;   /* 8, 16, 32 or 64 */
  int32_t rsi;          /* reference sample interval in blocks, 1..4096 */
  uint32_t flags;       /* ccsdsFlags */
  uint64_t reserved;    /* 0 */
} smm_grib_aec_t;
/* how a row's stream ended */
enum { SMM_GRIB_AEC_OK = 0, SMM_GRIB_AEC_EXHAUSTED = 1, SMM_GRIB_AEC_INVALID = 2 };
/* bins of smm_grib_aec_decode_host's histogram, in order: zero-block run, zero-block run "to the end of the segment",
 * second extension, split-sample k = 0, split-sample k > 0, uncompressed, blocks that carry a reference sample */
#define SMM_GRIB_AEC_OPTIONS 7

/* A GRIB-2 field in complex packing (data representation templates 5.2 and 5.3; smm_grib_cpx_unpack,
 * smm_grib_cpx_decode_host): where section 7's bytes (from its octet 6 on) of one batch row lie in x, and section 5's
 * parameters.  The stream decodes to n_values integers X in [0, 2^32) -- the q of smm_grib_row_t's rule; the rule is the
 * text of smmregrid_amd/csrc/smm_grib_cpx.hpp.  order == SMM_GRIB_CPX_SIMPLE marks a row that is simple-packed already:
 * nothing else of its record is looked at, its smm_grib_row_t says it all.  Missing value management (octet 23) is not
 * in the record: the _mv entries take it in a parallel array, the others decode 0 only. */
#define SMM_GRIB_CPX_SIMPLE (-1)
typedef struct smm_grib_cpx_t {   /* one batch row = one GRIB field, 72 B */
  uint64_t byte_off;      /* of the stream's first byte (octet 6 of section 7), from x */
  uint64_t byte_len;      /* bytes of the stream */
  uint64_t n_values;      /* values the stream codes: the grid's points, or the set bits of the row's bitmap; < 2^31 */
  uint32_t n_groups;      /* NG (octets 32-35); <= n_values, or the row ends as invalid */
  int32_t nbits;          /* octet 20: width of the group reference values, 0..32 */
  uint32_t width_ref;     /* octet 36: reference for group widths */
  int32_t width_bits;     /* octet 37: bits per stored group width, 0..32 */
  uint32_t length_ref;    /* octets 38-41: reference for group lengths */
  uint32_t length_inc;    /* octet 42: length increment */
  uint32_t length_last;   /* octets 43-46: true length of the last group */
  int32_t length_bits;    /* octet 47: bits per stored scaled group length, 0..32 */
  int32_t order;          /* octet 48: order of spatial differencing, 0 (template 5.2), 1 or 2; SMM_GRIB_CPX_SIMPLE */
  int32_t n_oct;          /* octet 49: octets per extra descriptor, 1..4 (order > 0) */
  uint64_t reserved;      /* 0 */
} smm_grib_cpx_t;
/* how a row's stream ended: EXHAUSTED -- a section or a group's bits leave the stream; INVALID -- a group wider than 32
 * bits, more groups than values, group lengths that do not sum to n_values, an X outside [0, 2^32) */
enum { SMM_GRIB_CPX_OK = 0, SMM_GRIB_CPX_EXHAUSTED = 1, SMM_GRIB_CPX_INVALID = 2 };

/* smm_apply flags.  Bits outside this set are refused with SMM_ERR_INVALID by every entry that takes `flags`
 * (ABI <= 4 encoded kernel variants in bits 16..23: those are smm_debug_set_tuning knobs now). */
enum {
  SMM_APPLY_MASKED = 1u << 0,   /* apply dst_imask (regrid.py:553-559); per level in a group */
  SMM_APPLY_NO_FILL = 1u << 1,  /* skip the 1e20 fill: the caller guarantees finite X (results are undefined otherwise) */
  SMM_APPLY_SB_PACKED = 1u << 2, /* smm_apply_sb: X holds only the used source cells (smm_operator_used_sources order) */
  SMM_APPLY_HOST_NO_PACK = 1u << 3, /* smm_apply_host: always ship whole rows (no packing of the used source cells) */
  SMM_APPLY_SB_Y_SB = 1u << 4,   /* smm_apply_sb: the result is kept batch-fastest too, Y (n_dst, ldy >= n_batch) */
  SMM_APPLY_SKIPNA = 1u << 6,    /* renormalise over the valid source values of each batch row (see below) */
  SMM_APPLY_KERNEL_SELL = 1u << 8, /* force the row-per-lane SELL-64 kernel                  */
  SMM_APPLY_KERNEL_TILE = 1u << 9  /* force the LDS-staged source-tile kernel (if planned)   */
};
/* SMM_APPLY_SKIPNA, for destination row d and batch row b, links k of the canonical CSR in ascending source order:
 * a link is invalid when x[b, col_k] is not finite and w_k != 0.  In f64, from +0.0, multiply and add kept apart:
 *   num = sum over valid links of w * x     den = sum over valid links of w     tot = sum over all links of w
 * inv = the row has an invalid link;  r = inv ? den / tot : 1.0;  v = inv ? num * (tot / den) : num.
 * The row is dead when it is masked (SMM_APPLY_MASKED, dst_imask[d] == 0), when inv && !(r > 0.0), or when
 * remap_area_min > 0 && (the operator has dst_frac || inv) && frac_d * r < remap_area_min (frac_d = dst_frac[d],
 * 1.0 without dst_frac); y = (dead || v > 1e19) ? NaN : v.  A row without an invalid link is bit-identical to the
 * plain apply.  Finite values, huge ones included, are valid.  With SMM_APPLY_NO_FILL: SMM_ERR_INVALID. */
typedef struct smm_operator* smm_operator_t; /* one (S x D) weights matrix resident in HBM      */
typedef struct smm_group* smm_group_t;       /* ordered set of operators (one per masked level) */

/* ------------------------------------------------------------------ misc */
int smm_abi_version(void);
const char* smm_last_error(void);

/* ------------------------------------------------- device / memory / time */
int smm_device_count(int* count);
int smm_set_device(int device);
int smm_get_device(int* device);
int smm_device_name(int device, char* buf, size_t buflen);
int smm_mem_info(size_t* free_bytes, size_t* total_bytes);
int smm_malloc(void** dptr, size_t bytes);
int smm_free(void* dptr);
int smm_host_alloc(void** hptr, size_t bytes); /* pinned host memory */
int smm_host_free(void* hptr);
/* host -> host copy on the library's staging threads (what the host pipelines use between the caller's arrays and
 * their pinned staging): one thread tops out far below PCIe when it fills a pinned buffer.  The ranges must not overlap. */
int smm_host_memcpy(void* dst_host, const void* src_host, size_t bytes);
int smm_memcpy_h2d(void* dst_dev, const void* src_host, size_t bytes, void* stream);
int smm_memcpy_d2h(void* dst_host, const void* src_dev, size_t bytes, void* stream);
int smm_memcpy_d2d(void* dst_dev, const void* src_dev, size_t bytes, void* stream);
/* pitched copies: `height` rows of `width` BYTES, row r at base + r * pitch (pitches in bytes) -- fields
 * whose device rows start on 128-B lines, columns of a batch-fastest field */
int smm_memcpy2d_h2d(void* dst_dev, size_t dpitch, const void* src_host, size_t spitch, size_t width,
                     size_t height, void* stream);
int smm_memcpy2d_d2h(void* dst_host, size_t dpitch, const void* src_dev, size_t spitch, size_t width,
                     size_t height, void* stream);
int smm_memset(void* dst_dev, int value, size_t bytes, void* stream);
int smm_stream_create(void** stream);
int smm_stream_destroy(void* stream);
int smm_stream_sync(void* stream); /* NULL = default stream */
int smm_device_sync(void);
int smm_event_create(void** event);
int smm_event_destroy(void* event);
int smm_event_record(void* event, void* stream);
int smm_event_sync(void* event);
int smm_stream_wait_event(void* stream, void* event); /* work queued on stream after this call waits for event */
int smm_event_elapsed_ms(void* start, void* stop, float* ms);

/* Synthetic field generator for benchmarks and full-size tests: fills n elements
 * with a counter-based pseudo-normal sequence mean + sigma * N(0,1) (element i
 * depends only on (seed, i), so shards can be filled independently). */
int smm_fill_random(void* dst_dev, int dtype, int64_t n, uint64_t seed, double mean,
                    double sigma, void* stream);

/* ------------------------------------------------------------- operators */

/*
 * Build the operator from SCRIP/CDO links (replaces weights.py:31-42).
 *   src_addr_1based / dst_addr_1based : int32[nnz], 1-based as in the CDO file
 *   w                                  : double[nnz] = remap_matrix[:, 0]
 * Links are sorted by (dst, src) with the original order as tie-break and
 * duplicate (dst, src) pairs are summed in that order (the COO constructor's
 * semantics).  Explicit zero weights are kept.  The handle owns a device copy
 * on `device`; host arrays are only read during the call.
 */
int smm_operator_create(int64_t n_src, int64_t n_dst, int64_t nnz,
                        const int32_t* src_addr_1based,
                        const int32_t* dst_addr_1based,
                        const double* w, int device, smm_operator_t* out);
/*
 * Build the operator from a canonical CSR kept from an earlier smm_operator_export_csr (SURVEY
 * f1 "native CSR cache": skips the sort + duplicate pass of weights.py:37-39 on reload).  rowptr
 * int64[n_dst+1] from 0, col int32 0-based strictly ascending inside a row, val double; anything
 * else is SMM_ERR_INVALID.  Epilogue arrays are set separately as for smm_operator_create.
 */
int smm_operator_create_csr(int64_t n_src, int64_t n_dst, const int64_t* rowptr,
                            const int32_t* col, const double* val, int device,
                            smm_operator_t* out);
/*
 * smm_operator_create with options.
 *   SMM_CREATE_PRUNE_ZEROS  drop links whose (duplicate-summed) weight is exactly zero.  The reference
 *     multiplies them (`sparse.COO` keeps explicit zeros, weights.py:37-39); with the 1e20 fill every
 *     gathered value is finite, so such a link adds +-0.0 to a sum that starts at +0.0 and the results
 *     are bit-identical without it.  Bilinear weights between aligned grids are mostly zeros
 *     (r1440x721 -> r360x180: 2 links of 4).  smm_operator_info / export_csr then describe the pruned
 *     matrix.  Off by default: the operator holds exactly the links it was given.
 */
enum { SMM_CREATE_PRUNE_ZEROS = 1u << 0 };
int smm_operator_create_opt(int64_t n_src, int64_t n_dst, int64_t nnz,
                            const int32_t* src_addr_1based, const int32_t* dst_addr_1based,
                            const double* w, unsigned options, int device, smm_operator_t* out);
int smm_operator_destroy(smm_operator_t op);

/* sizes after duplicate-summing; n_used_src = distinct source cells with >= 1 link (U) */
int smm_operator_info(smm_operator_t op, int64_t* n_src, int64_t* n_dst,
                      int64_t* nnz, int64_t* n_used_src, int64_t* max_row_nnz);

/* canonical CSR (row = destination cell, 0-based, columns ascending) for parity tests.
 * rowptr: int64[n_dst+1], col: int32[nnz], val: double[nnz] (host buffers). */
int smm_operator_export_csr(smm_operator_t op, int64_t* rowptr, int32_t* col, double* val);

/*
 * Epilogue vectors of the weights file (host pointers, copied to HBM):
 *   dst_imask: int32[n_dst] (regrid.py:510, used when SMM_APPLY_MASKED)
 *   dst_frac : double[n_dst] (regrid.py:509, used when area_min > 0)
 * Either may be NULL to clear it.  Call before any concurrent smm_apply and before the operator
 * joins a group (smm_group_create copies the device pointers into the group's level table):
 * SMM_ERR_INVALID while the operator belongs to a group.  On failure the old vectors stay in force.
 */
int smm_operator_set_epilogue(smm_operator_t op, const int32_t* dst_imask,
                              const double* dst_frac);

/*
 * Destination-mask pre-compute (weights.py:47-52):
 *   dst_imask[d] = (sum_s src_imask[s] * W[s,d]) < 0.5 ? 0 : 1
 * src_imask int32[n_src] host, dst_imask int32[n_dst] host (output).
 * Runs on the device (SpMV + threshold).
 */
int smm_operator_mask_apply(smm_operator_t op, const int32_t* src_imask, int32_t* dst_imask);

/* kernel selection the library made for this operator -- kernel_kind bit 0: an LDS tile plan
 * exists, bit 1: it is the default kernel (else SELL row-per-lane), bits 8..: destination rows
 * per block of the plan (256, 64, or 32 / 16 / 8 for rows with very wide footprints) */
int smm_operator_plan_info(smm_operator_t op, int* kernel_kind, int64_t* lds_bytes,
                           int64_t* staged_src_elems);

/* Launch geometry smm_apply would use for n_batch rows of x_dtype under `flags` (nothing is
 * launched; for tests and tuning).  kernel: 0 = SELL row-per-lane, 1 = LDS tile staged through registers,
 * 2 = LDS tile staged by LDS-DMA into a ring of two slots (small tiles of 16-B aligned fields); j_per_block: batch
 * rows walked by one workgroup; rows_per_step: batch rows staged per barrier pair; rows_per_block:
 * destination rows per workgroup; n_blocks: grid size; lds_bytes: dynamic LDS per workgroup;
 * big_operator: the links do not stay in L2, walks are lengthened to amortise their re-read.
 * The answer assumes a field whose base, row pitch and strides are multiples of 16 B (what the LDS-DMA
 * staging needs): smm_apply checks the real field and falls back from kernel 2 to kernel 1 (with that
 * kernel's rows_per_step / lds_bytes) when it is not.  n_blocks is the whole batch; beyond 2^31 - 1
 * workgroups smm_apply launches it in parts.  Any out pointer may be NULL.
 * x_dtype SMM_I16 / SMM_U16 answers for smm_apply_cf: packed fields always run kernel 0 (the LDS tile kernel is
 * not built for 2-byte elements), whatever the operator's plan; with SMM_APPLY_KERNEL_TILE: SMM_ERR_UNSUPPORTED. */
int smm_operator_launch_info(smm_operator_t op, int x_dtype, int64_t n_batch, unsigned flags,
                             int* kernel, int* j_per_block, int* rows_per_step, int* rows_per_block,
                             int64_t* n_blocks, int64_t* lds_bytes, int* big_operator);

/* per-level set (replaces the list built by weights.py:7-23); borrows the operators: they must
 * outlive the group (smm_operator_destroy fails with SMM_ERR_INVALID on a member) */
int smm_group_create(const smm_operator_t* ops, int n_ops, smm_group_t* out);
int smm_group_destroy(smm_group_t g);
/* Uploads the device copy of one (level_index, masked_levels) configuration ahead of time, so
 * that smm_group_apply calls with the same configuration allocate nothing and never block
 * (stream-capturable).  Configurations stay cached until smm_group_destroy (n_lev * 4 + n_ops
 * bytes each); a first-seen configuration passed straight to smm_group_apply is uploaded there
 * (one small hipMalloc + blocking copy, no device synchronisation). */
int smm_group_prepare(smm_group_t g, int64_t n_lev, const int32_t* level_index,
                      const uint8_t* masked_levels);
int smm_group_launch_info(smm_group_t g, int x_dtype, int64_t n_outer, int64_t n_lev, int64_t n_inner,
                          unsigned flags, int* kernel, int* j_per_block, int* rows_per_step,
                          int* rows_per_block, int64_t* n_blocks, int64_t* lds_bytes, int* big_operator);
/* (smm_group_launch_info: x_dtype SMM_I16 / SMM_U16 answers for smm_group_apply_cf -- kernel 0, as for single operators;
 * with SMM_APPLY_KERNEL_TILE: SMM_ERR_UNSUPPORTED.  SMM_F16 / SMM_BF16 fields: the same, for either entry.) */
/* bit 0: every member has an LDS tile plan of the group's block shape, bit 1: the tile kernel is the default */
int smm_group_plan_info(smm_group_t g, int* kernel_kind, int* slices_per_block);

/* ----------------------------------------------------------------- apply */

/*
 * 2-D apply (regrid.py:536-570):   Y[b, :] = epilogue( fill(X[b, :]) . W ),  b in [0, n_batch)
 *   x : device, element type x_dtype, row b starts at x + b*ldx elements (ldx >= n_src)
 *   y : device, element type y_dtype, row b starts at y + b*ldy elements (ldy >= n_dst)
 * The reference always produces f64 (result_type(x, f64)); y_dtype == SMM_F32 is an
 * opt-in narrowing store.
 */
int smm_apply(smm_operator_t op,
              const void* x, int x_dtype, int64_t ldx,
              void* y, int y_dtype, int64_t ldy,
              int64_t n_batch, double remap_area_min, unsigned flags, void* stream);

/*
 * The same product for fields kept BATCH-FASTEST ("SB" layout) by a device-resident producer:
 *   x : device, (n_src, ldx) -- the n_batch values of source cell s are contiguous at x + s*ldx
 *       (ldx >= n_batch); with SMM_APPLY_SB_PACKED x holds only the U used source cells, row r =
 *       the r-th entry of smm_operator_used_sources (ascending source index)
 *   y : device, (n_batch, ldy) exactly as smm_apply writes it (regrid.py:550 layout); with
 *       SMM_APPLY_SB_Y_SB the result stays batch-fastest as well -- y (n_dst, ldy >= n_batch), entry b of
 *       destination cell d at y + d*ldy + b -- which is the x a following smm_apply_sb on the target
 *       grid consumes without any transpose (chains of regrids on device-resident fields)
 * In the reference's native (B, S) layout a stencil that needs 16-B pairs on a 32-B stride (config
 * 2: bilinear 4:1) wastes half of every 128-B line fetched; here every needed source cell is one
 * contiguous run, so HBM traffic equals the algorithmic bytes.  Results are bit-identical to
 * smm_apply on the transposed field.  The first call on an operator uploads its canonical CSR
 * (smm_operator_prepare_sb does that ahead of time); afterwards the call allocates nothing.
 */
int smm_operator_prepare_sb(smm_operator_t op);
/* ascending 0-based indices of the n_used_src source cells that carry a link (host int32[n_used_src]) */
int smm_operator_used_sources(smm_operator_t op, int32_t* used);
int smm_apply_sb(smm_operator_t op,
                 const void* x, int x_dtype, int64_t ldx,
                 void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream);

/*
 * Same product for fields in HOST memory (what Regridder.apply_weights receives,
 * regrid.py:537-541): the batch rows are cut into chunks that flow through a
 * double-buffered pipeline -- copy into pinned staging (skipped for pinned
 * buffers, e.g. from smm_host_alloc), H2D, kernel, D2H -- on two streams, so
 * transfers of one chunk overlap the kernel of the other.  Synchronous: Y is
 * complete on return.  chunk_rows <= 0 picks ~256 MiB of X per chunk.
 * This path is PCIe-bound (about 100x below the device-resident rate).  When the operator uses at most
 * four fifths of its source cells (bilinear / nearest downsampling, a masked ocean level) and the batch has >= 8 rows, the staging
 * copy packs only the used cells of a chunk, batch-fastest, and the chunk runs through the kernel of
 * smm_apply_sb: a quarter of the PCIe bytes for config 2, the same bits (SMM_APPLY_HOST_NO_PACK or a
 * forced kernel flag turns it off).
 */
int smm_apply_host(smm_operator_t op,
                   const void* x_host, int x_dtype, int64_t ldx,
                   void* y_host, int y_dtype, int64_t ldy,
                   int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows);

/*
 * The three entries above for CF-packed fields: x_dtype SMM_I16 / SMM_U16, x holds the raw 2-byte integers (2-byte
 * aligned, ldx in elements) and is decoded inside the kernels by *cf (smm_cf_decode_t above) -- a quarter of the
 * bytes of an f64 field in HBM, over PCIe and through the host pack.  y_dtype must be SMM_F64 (SMM_F32 results are
 * not built: SMM_ERR_UNSUPPORTED).  cf == NULL with a float x_dtype is the plain entry; cf == NULL with an integer
 * x_dtype, cf != NULL with a float one, a fill value outside the raw type, or SMM_APPLY_NO_FILL with n_fill > 0 (the
 * decode makes NaN) are SMM_ERR_INVALID.  MASKED, SKIPNA, HOST_NO_PACK, SB_PACKED, SB_Y_SB and KERNEL_SELL work as
 * for float fields; smm_apply_cf runs the SELL kernel whatever the operator's plan (smm_operator_launch_info says
 * so) and SMM_APPLY_KERNEL_TILE is SMM_ERR_UNSUPPORTED.  Level groups take packed input through the three
 * smm_group_apply*_cf entries further down.
 */
int smm_apply_cf(smm_operator_t op,
                 const void* x, int x_dtype, int64_t ldx,
                 void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream,
                 const smm_cf_decode_t* cf);
int smm_apply_sb_cf(smm_operator_t op,
                    const void* x, int x_dtype, int64_t ldx,
                    void* y, int y_dtype, int64_t ldy,
                    int64_t n_batch, double remap_area_min, unsigned flags, void* stream,
                    const smm_cf_decode_t* cf);
int smm_apply_host_cf(smm_operator_t op,
                      const void* x_host, int x_dtype, int64_t ldx,
                      void* y_host, int y_dtype, int64_t ldy,
                      int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows,
                      const smm_cf_decode_t* cf);

/*
 * The three _cf entries with a CF-packed RESULT: enc != NULL stores Y as raw 2-byte integers, encoded inside the
 * kernels' stores by *enc (smm_cf_encode_t above); y_dtype must then be SMM_I16 / SMM_U16, y 2-byte aligned and ldy in
 * 2-byte elements -- a quarter of the f64 result in HBM and over PCIe (smm_apply_host_pk stages, copies and counts
 * SMM_HOST_STAT_D2H_BYTES in 2-byte cells).  enc == NULL is the _cf entry unchanged.  X is float (cf == NULL) or packed
 * with Y's own raw type (a packed X of the other raw type: SMM_ERR_UNSUPPORTED).  SMM_ERR_INVALID, before any device
 * is touched: enc != NULL with a float y_dtype, an integer y_dtype without enc, a fill the raw type cannot hold, a
 * zero or non-finite scale, a non-finite offset, reserved != 0.  Packed results run the SELL kernel (smm_apply_pk, the
 * whole-row chunks of smm_apply_host_pk) or the batch-fastest kernel, for float X too: the LDS tile kernel is not
 * built for them and SMM_APPLY_KERNEL_TILE with enc is SMM_ERR_UNSUPPORTED.  MASKED, SKIPNA, SB_PACKED, SB_Y_SB,
 * HOST_NO_PACK, KERNEL_SELL and the split of grids beyond 2^31 - 1 blocks behave as for float Y; a batch-fastest
 * packed result (SB_Y_SB) is what a following smm_apply_sb_cf consumes.  Level groups: smm_group_apply_pk and friends,
 * below the group _cf entries.
 */
int smm_apply_pk(smm_operator_t op,
                 const void* x, int x_dtype, int64_t ldx,
                 void* y, int y_dtype, int64_t ldy,
                 int64_t n_batch, double remap_area_min, unsigned flags, void* stream,
                 const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);
int smm_apply_sb_pk(smm_operator_t op,
                    const void* x, int x_dtype, int64_t ldx,
                    void* y, int y_dtype, int64_t ldy,
                    int64_t n_batch, double remap_area_min, unsigned flags, void* stream,
                    const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);
int smm_apply_host_pk(smm_operator_t op,
                      const void* x_host, int x_dtype, int64_t ldx,
                      void* y_host, int y_dtype, int64_t ldy,
                      int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows,
                      const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);

/*
 * smm_apply / smm_apply_host for GRIB simple-packed fields shipped RAW (smm_grib_row_t above): x holds the packed bit
 * streams of n_batch fields -- typically the file's bytes as they are -- and rows[b] says where batch row b starts in
 * it and how it decodes; rows need not lie in buffer order, may have different widths and may overlap.  2 B per cell
 * at 16 bits (1.5 B at 12) cross PCIe and HBM instead of 4, and no host decode runs.  The kernel is the row-per-lane
 * SELL-64 kernel with the bit extraction and the decode in its gather (two instantiations, without and with the f64
 * division: the one without runs when every row of the call has ddiv == 1.0; their bits are identical).
 *   smm_apply_grib       x device bytes, 4-byte aligned, the allocation covering x_bytes rounded up to 4 (the kernel
 *                        reads whole 32-bit words, never past that).  rows is a HOST array (pageable or page-locked): it is copied on `stream`
 *                        into a device table the operator owns (grown on demand) and may be reused on return.  Calls on
 *                        one operator share that table: they take turns, and are ordered against each other only on
 *                        one stream -- concurrent calls on different streams need one operator handle each.
 *   smm_apply_host_grib  x_host host bytes (no alignment needed), Y host (n_batch, ldy).  Chunks of consecutive rows flow
 *                        through the pipeline of smm_apply_host: each row's ceil(n_src * nbits / 8) data bytes are copied
 *                        into the pinned staging back to back at 4-byte-aligned starts (pinned x_host too: the rows of a
 *                        chunk need not be adjacent in a file), the chunk's table rides in front of them.  A chunk is
 *                        sized by bytes, not rows (rows may differ in width): staged X plus rows * n_dst * 8 of Y against
 *                        ~256 MiB and an eighth of the free device memory (a chunk's X and Y exist twice on the
 *                        device: a quarter in all); chunk_rows > 0 fixes the rows per chunk.
 *                        SMM_HOST_STAT_H2D_BYTES counts the staged bytes with their <= 3 B pads and the tables.
 * y_dtype must be SMM_F64 (else SMM_ERR_UNSUPPORTED).  SMM_APPLY_MASKED and SMM_APPLY_NO_FILL work as for float fields,
 * SMM_APPLY_KERNEL_SELL is accepted (it is the kernel that runs); SMM_APPLY_SKIPNA (its form of these entries is the _na
 * pair below), SMM_APPLY_KERNEL_TILE and the batch-fastest / host-pack flags are SMM_ERR_UNSUPPORTED.  SMM_ERR_INVALID, before any device is touched: flag bits
 * outside the set, null pointers, a negative n_batch, ldy < n_dst, a misaligned x (device entry) or y, nbits outside
 * 0..32, reserved != 0, a bscale that is not a normal power of two, a ddiv that is not finite or <= 0, a non-finite ref,
 * a row whose [byte_off, byte_off + ceil(n_src * nbits / 8)) leaves [0, x_bytes).  The rules are checked before the
 * operator handle is looked at (a NULL handle is SMM_ERR_INVALID, as everywhere).
 */
int smm_apply_grib(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows /* host */,
                   void* y, int y_dtype, int64_t ldy, int64_t n_batch,
                   double remap_area_min, unsigned flags, void* stream);
int smm_apply_host_grib(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                        void* y_host, int y_dtype, int64_t ldy, int64_t n_batch,
                        double remap_area_min, unsigned flags, int64_t chunk_rows);

/*
 * The two entries above for fields with a bitmap (ocean and land-surface variables, regional and masked grids):
 * `bitmaps` is a HOST array of n_batch records parallel to `rows` (smm_grib_bitmap_t above), or NULL -- then the call
 * is the entry above in every respect.  Rows with and without a bitmap may be mixed, and several rows may name one
 * bitmap_off (GRIB-2's "same bitmap as the previous field").  A cell whose bitmap bit is 0 becomes a float32 NaN, a
 * cell whose bit is 1 the decode of packed value number rank(c); after that nothing differs (the fill to float32(1e20)
 * unless SMM_APPLY_NO_FILL, promotion to f64, the plain epilogue): the results are bit-identical to smm_apply with
 * SMM_F32 X on the field a host decode gives, NaN where the bitmap is 0.
 * How: ahead of the gather, on the same stream, two small kernels turn each bitmapped row's bitmap into a device
 * table of one 8-byte entry per 32 cells -- the 32 bitmap bits and the count of set bits before them (a popcount
 * per (row, segment of 32768 cells), then a scan inside every segment) -- 0.25 B per cell; the gather loads one entry
 * per link, takes a popcount and a bit test and reads the stream at the rank instead of the cell.  Bits at or beyond
 * n_src in the bitmap's last byte influence nothing.
 *   smm_apply_grib_bm       as smm_apply_grib.  The tables live in a buffer the operator owns (grown on demand, only
 *                           bitmapped rows take space), as the row table does: the same rule holds -- calls on one
 *                           operator take turns and are ordered against each other only on ONE stream; concurrent
 *                           calls on different streams need one operator handle each.
 *   smm_apply_host_grib_bm  as smm_apply_host_grib.  With bitmaps a chunk stages its row table, then its bitmap records
 *                           (16 B per row), then per row its ceil(n_values * nbits / 8) data bytes and, for a bitmapped
 *                           row, its ceil(n_src / 8) bitmap bytes (a row that shares another row's bitmap stages its
 *                           own copy), every piece at the next 4-byte-aligned offset, all in one H2D copy: per row
 *                           40 + 16 + align4(data) + (bitmapped ? align4(ceil(n_src / 8)) : 0) bytes in
 *                           SMM_HOST_STAT_H2D_BYTES.  The rank tables are device-only, one buffer per pipeline slot,
 *                           and count against the chunk's byte budget with the staged bytes.
 * SMM_ERR_INVALID in addition to the refusals above, before any launch: n_values > n_src; a bitmap whose
 * ceil(n_src / 8) bytes leave [0, x_bytes); a row whose ceil(n_values * nbits / 8) data bytes leave it (for a bitmapped
 * row this takes the place of the n_src-based check).  n_values is trusted for sizes only: every kernel load stays
 * clamped to the buffer's last word, so a lying n_values yields wrong numbers and never a read outside the allocation.
 */
int smm_apply_grib_bm(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows /* host */,
                      const smm_grib_bitmap_t* bitmaps /* host, or NULL */, void* y, int y_dtype, int64_t ldy,
                      int64_t n_batch, double remap_area_min, unsigned flags, void* stream);
int smm_apply_host_grib_bm(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t ldy,
                           int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows);

/*
 * The SMM_APPLY_SKIPNA form of the two _bm entries above, with their argument lists (`bitmaps` may be NULL): the bit is
 * implied and may be passed.  The gather hands every value to the sum raw -- no 1e20 fill; a cell whose bitmap bit is 0
 * is the float32 NaN, a value whose rule overflows float32 is the infinity the decode gives -- and the kernel applies
 * the SMM_APPLY_SKIPNA rule above (num / den / tot per destination row, the area test on frac_d * r).  The result: the
 * bits of smm_apply with SMM_APPLY_SKIPNA | SMM_APPLY_KERNEL_SELL on the float32 field a host decode gives, NaN where
 * the bitmap is 0.  Staging, chunks, rank tables and the splits of oversized grids are those of the twins.
 * Refusals, in this order: flag bits outside the set, and SMM_APPLY_NO_FILL (the SKIPNA rule above): SMM_ERR_INVALID;
 * SMM_APPLY_KERNEL_TILE and the batch-fastest / host-pack flags, then y_dtype != SMM_F64: SMM_ERR_UNSUPPORTED; after
 * that everything the twins refuse, as they refuse it (remap_area_min > 0 without dst_frac and SMM_APPLY_MASKED without
 * dst_imask are SMM_ERR_INVALID, as for smm_apply with SMM_APPLY_SKIPNA).
 */
int smm_apply_grib_na(smm_operator_t op, const void* x, int64_t x_bytes, const smm_grib_row_t* rows /* host */,
                      const smm_grib_bitmap_t* bitmaps /* host, or NULL */, void* y, int y_dtype, int64_t ldy,
                      int64_t n_batch, double remap_area_min, unsigned flags, void* stream);
int smm_apply_host_grib_na(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps, void* y_host, int y_dtype, int64_t ldy,
                           int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows);

/*
 * Results in GRIB simple packing (smm_grib_encode_t above): 16 or 12 bits per cell, a reference value and a binary scale
 * per row and a bitmap where cells are missing cross PCIe instead of 8 B per cell, in a form the _bm entries above take
 * back as they are.  The packing cannot sit in the apply kernels' stores (a row's rule depends on the row's own minimum
 * and maximum): four steps run on the float64 Y before it leaves the device -- a range pass that also writes the bitmap
 * (one workgroup per row and segment of 32768 cells), a rule pass (one wave per row), the rank tables of the bitmaps
 * just written (the build of smm_apply_grib_bm), and a pack pass with one thread per 32-bit word of a row's stream.
 * The layout is known before any launch: row b owns a slot of align4(ceil(n_dst / 8)) bitmap bytes followed by
 * align4(ceil(n_dst * nbits_b / 8)) stream bytes, slots back to back in row order.  The bitmap is MSB first with zero
 * pad bits; the stream holds the present cells in cell order, big-endian, and every byte of it that the values do not
 * reach is zero: every byte of every slot is written.  rows_out[b] = {byte offset of the stream, ref, bscale, ddiv,
 * stored width (nbits, or 0 for a constant or empty row), 0}; bitmaps_out[b] = {byte offset of the bitmap, n_values},
 * the offset SMM_GRIB_NO_BITMAP when n_values == n_dst.
 *   smm_grib_out_layout     host only: byte_off[b] (may be NULL) = where row b's slot starts, *total_bytes = all slots.
 *   smm_grib_pack           packs any float64 device result (n_batch, ldy) on `device` into `out` (device, 4-byte
 *                           aligned, out_bytes >= the layout's total).  enc, rows_out and bitmaps_out are HOST arrays of
 *                           n_batch records; the stream is synchronised before the call returns (the records come
 *                           back to the host arrays).  Scratch is allocated and freed inside the call.
 *   smm_apply_host_grib_pk  smm_apply_host_grib_bm (bitmaps may be NULL; SMM_APPLY_SKIPNA in flags: smm_apply_host_grib_na)
 *                           with the result packed: each chunk's float64 Y stays on the device and is packed on the
 *                           chunk's stream into a buffer that holds the chunk's row and bitmap records followed by its
 *                           slots.  A pageable out_host receives one D2H copy per chunk through the pinned slot
 *                           buffer; a page-locked out_host receives the slots directly, the records (56 B per row) in
 *                           a copy of their own.  SMM_HOST_STAT_D2H_BYTES counts the slots and the records;
 *                           SMM_HOST_STAT_H2D_BYTES also counts 48 B per row of pack tables staged behind the chunk's X.
 *                           The chunk plan budgets the packed buffer and the scratch beside the device-only Y.
 *   smm_group_apply_host_grib_pk  smm_group_apply_host_grib (below; SMM_APPLY_SKIPNA in flags:
 *                           smm_group_apply_host_grib_na) with the result packed the same way.  enc, rows_out and
 *                           bitmaps_out are HOST arrays of n_outer * n_lev * n_inner records in record order (o, l, i);
 *                           row b owns slot b of smm_grib_out_layout(D, enc, n_rows).  There is no `transpose`: no Y
 *                           array is delivered.  A chunk is a block of whole outer indices; the grouped gather writes
 *                           its Y on the device in record order, (rows of the chunk, D), and the four pack steps run
 *                           behind it on the chunk's stream over all of the chunk's rows.  Pack tables, result copies,
 *                           the two SMM_HOST_STAT byte counts and the chunk plan's budget are those of
 *                           smm_apply_host_grib_pk, with never less than one outer index per chunk.
 * SMM_ERR_INVALID, before any device is touched: nbits outside 1..32, a ddiv that is not finite or <= 0, reserved != 0,
 * out_bytes below the layout, a misaligned out (device entry) or y, ldy < n_dst, n_dst >= 2^31, null pointers, a negative
 * count; for the host entry everything smm_apply_host_grib_bm / _na refuses, as they refuse it (SMM_APPLY_KERNEL_TILE
 * included).  The group entry refuses the result side first -- null enc, rows_out or bitmaps_out and a bad encode rule
 * whatever the handle, out_bytes below the layout and a null out_host once the group gives n_dst -- then everything
 * smm_group_apply_host_grib / _na refuses, in their order and with their codes.
 */
int smm_grib_out_layout(int64_t n_dst, const smm_grib_encode_t* enc, int64_t n_batch, uint64_t* byte_off,
                        uint64_t* total_bytes);
int smm_grib_pack(int device, const void* y, int64_t ldy, int64_t n_dst, int64_t n_batch,
                  const smm_grib_encode_t* enc /* host */, void* out, int64_t out_bytes,
                  smm_grib_row_t* rows_out /* host */, smm_grib_bitmap_t* bitmaps_out /* host */, void* stream);
int smm_apply_host_grib_pk(smm_operator_t op, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                           const smm_grib_bitmap_t* bitmaps /* or NULL */, const smm_grib_encode_t* enc,
                           void* out_host, int64_t out_bytes, smm_grib_row_t* rows_out, smm_grib_bitmap_t* bitmaps_out,
                           int64_t n_batch, double remap_area_min, unsigned flags, int64_t chunk_rows);
int smm_group_apply_host_grib_pk(smm_group_t g, const void* x_host, int64_t x_bytes, const smm_grib_row_t* rows,
                                 const smm_grib_bitmap_t* bitmaps /* or NULL */, const smm_grib_encode_t* enc,
                                 void* out_host, int64_t out_bytes, smm_grib_row_t* rows_out,
                                 smm_grib_bitmap_t* bitmaps_out, int64_t n_outer, int64_t n_lev, int64_t n_inner,
                                 const int32_t* level_index, const uint8_t* masked_levels, double remap_area_min,
                                 unsigned flags, int64_t chunk_outer);

/*
 * CCSDS-packed GRIB-2 fields (smm_grib_aec_t above) on the raw road: one device step turns the rows' adaptive-
 * entropy-coded streams into the simple-packed streams smm_apply_grib_bm / _na take -- the mirror of smm_grib_pack.
 * Row b's integers are stored with the row's own width nbits, big-endian, at a 4-byte-aligned offset of `out`, rows back
 * to back in row order, every byte of every slot written (a slot is ceil(n_values * nbits / 8) bytes rounded up to 4).
 * Three kernels: one wave per row parses the stream block after block (all lanes take part in a block: the wave finds
 * the ends of its fundamental sequences by popcounts and a scan) into 4 bytes per sample of scratch; one lane per
 * reference sample interval inverts the preprocessor, tiles of the scratch passing through LDS; one thread per 32-bit
 * word packs the stream.  The decoder and its two rules are the text of smmregrid_amd/csrc/smm_grib_aec.hpp.
 *   smm_grib_aec_layout       host only: byte_off[b] (may be NULL) = where row b's stream starts in `out`,
 *                             *total_bytes = all of them.
 *   smm_grib_aec_unpack       x: device bytes, 4-byte aligned, the allocation covering x_bytes rounded up to 4; recs and
 *                             rows_in: HOST arrays of n_batch records; out: device, 4-byte aligned, out_bytes >= the
 *                             layout's total.  rows_out[b] (HOST) = rows_in[b] with byte_off the row's place in `out`.
 *                             A row with nbits == 0 passes through untouched.  Scratch is allocated and freed inside
 *                             the call; the stream is synchronised before it returns.  A row whose stream does not end
 *                             ok makes the call return SMM_ERR_INVALID, smm_last_error naming the first such row.
 *   smm_grib_aec_decode_host  one row decoded on the host, no device: values[n_values] receives the integers,
 *                             histogram (SMM_GRIB_AEC_OPTIONS counters, or NULL) is ADDED to, *status is how the stream
 *                             ended (SMM_GRIB_AEC_*).  x_host needs no alignment.  A malformed stream costs wrong
 *                             numbers and a status, never a read outside [0, x_bytes).
 * SMM_ERR_INVALID, before any device is touched: null pointers, a negative count, nbits outside 0..32, a block size
 * outside {8, 16, 32, 64}, rsi outside 1..4096, a refused flag, reserved != 0, n_values >= 2^31, a stream that leaves
 * [0, x_bytes), rows_in[b].nbits != recs[b].nbits, out_bytes below the layout, a misaligned x or out.
 */
int smm_grib_aec_layout(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes);
int smm_grib_aec_unpack(int device, const void* x, int64_t x_bytes, const smm_grib_aec_t* recs /* host */,
                        const smm_grib_row_t* rows_in /* host */, int64_t n_batch, void* out, int64_t out_bytes,
                        smm_grib_row_t* rows_out /* host */, void* stream);
int smm_grib_aec_decode_host(const void* x_host, int64_t x_bytes, const smm_grib_aec_t* rec, uint32_t* values,
                             uint64_t* histogram, int* status);

/*
 * The way back: simple-packed streams on the device coded as CCSDS streams (template 5.42), behind the four passes of
 * smm_grib_pack or on any rows an smm_grib_row_t table describes.  THE RULE OF THIS ENCODER is the text of
 * smmregrid_amd/csrc/smm_grib_aec.hpp: the option with the fewest bits per block, the split parameter searched
 * exhaustively, zero blocks joined into runs within a 64-block segment.  It is fully deterministic -- the host entry and
 * the kernels give the same bytes -- and it is not libaec's choice of bits: a valid CCSDS 121.0-B stream that
 * smm_grib_aec_decode_host, smm_grib_aec_unpack and libaec decode.  recs are the parameters WANTED per row: n_values
 * and nbits as the row has them, block_size, rsi and flags to code with (what smm_grib_aec_unpack takes, no more);
 * byte_off and byte_len are not read.
 *   smm_grib_aec_pack_bound   host only: the worst case per row, ceil(n_values / block_size) blocks of
 *                             id length + block_size * nbits bits, rounded up to bytes and then to 4 (derived: no block
 *                             is coded longer than uncompressed); byte_off[b] (may be NULL) = the sum before row b,
 *                             *total_bytes = the sum.
 *   smm_grib_aec_pack         x: device bytes, 4-byte aligned, the allocation covering x_bytes rounded up to 4;
 *                             rows_in[b].byte_off: where row b's n_values integers of nbits bits begin in x; rows_in,
 *                             recs and recs_out: HOST arrays of n_batch records; out: device, 4-byte aligned,
 *                             out_bytes >= the bound.  recs_out[b] = recs[b] with byte_off and byte_len the row's
 *                             stream in out: rows lie back to back in row order, each at a 4-byte-aligned offset, and
 *                             every byte from a row's start to the aligned end of its stream is written;
 *                             *used_bytes = the aligned end of the last row, bytes of out beyond it are unspecified.
 *                             A row with nbits == 0 gets byte_len 0 and block_size 0 (the mark of a field without a
 *                             coded stream).  Six kernels (cost per block, runs and offsets per segment, per row, over
 *                             the rows, shared words zeroed, emit through LDS); nothing returns to the host between
 *                             them.  Scratch (8 B per block, 12 B per segment) is allocated and freed inside the call;
 *                             the stream is synchronised before it returns.
 *   smm_grib_aec_encode_host  one row coded on the host, no device: values[n_values] (n_values == rec->n_values, each
 *                             within nbits bits) into out[0, out_cap), *byte_len its bytes; histogram
 *                             (SMM_GRIB_AEC_OPTIONS counters, or NULL) is ADDED to.  out needs no alignment; out_cap
 *                             must reach the bound.
 * SMM_ERR_INVALID, before any device is touched: everything smm_grib_aec_unpack refuses about a record (its place in x
 * apart), rows_in[b].nbits != recs[b].nbits, a row's integers leaving [0, x_bytes), out_bytes / out_cap below the bound,
 * a misaligned x or out, null pointers, negative counts, a value wider than nbits (host entry).
 */
int smm_grib_aec_pack_bound(const smm_grib_aec_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes);
int smm_grib_aec_pack(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in /* host */,
                      const smm_grib_aec_t* recs /* host */, int64_t n_batch, void* out, int64_t out_bytes,
                      smm_grib_aec_t* recs_out /* host */, uint64_t* used_bytes, void* stream);
int smm_grib_aec_encode_host(const uint32_t* values, int64_t n_values, const smm_grib_aec_t* rec, void* out,
                             int64_t out_cap, uint64_t* byte_len, uint64_t* histogram);

/*
 * Complex-packed GRIB-2 fields (templates 5.2 / 5.3, smm_grib_cpx_t above) on the raw road: one device step turns the
 * rows' group-coded streams into the simple-packed streams smm_apply_grib_bm / _na take, as smm_grib_aec_unpack does for
 * CCSDS.  Nothing in the format is serial beyond a prefix sum: the groups' widths and lengths are fixed-width tables, a
 * scan gives every group its value and bit offset, every value is an independent bit extraction, and spatial
 * differencing is undone by one or two prefix sums over the row.  The rule is the text of
 * smmregrid_amd/csrc/smm_grib_cpx.hpp; the kernels are described in smm_grib_cpx.hip.
 *   smm_grib_cpx_layout       host only: a coded row's slot is n_values * 4 bytes (the width of its integers is only known
 *                             after the decode: the slot is a bound), a row marked SMM_GRIB_CPX_SIMPLE has none; slots lie
 *                             back to back in row order, each 4-byte aligned.  byte_off[b] (may be NULL) = where row b's
 *                             slot starts in `out`, *total_bytes = all of them.
 *   smm_grib_cpx_unpack       x: device bytes, 4-byte aligned, the allocation covering x_bytes rounded up to 4; recs and
 *                             rows_in: HOST arrays of n_batch records; out: device, 4-byte aligned, out_bytes >= the
 *                             layout's total.  Row b's integers are stored big-endian from its slot's start with the
 *                             row's own minimal width w_b = the bit length of its largest X (0 when every X is 0: a
 *                             constant field); every byte of ceil(n_values * w_b / 8) rounded up to 4 is written, the
 *                             rest of the slot is unspecified.  rows_out[b] (HOST) = rows_in[b] with byte_off the slot
 *                             and nbits = w_b (rows_in[b].nbits is not read).  A marked row passes through untouched.
 *                             Scratch (8 B per value, 16 B per group) is allocated and freed inside the call; the stream
 *                             is synchronised before it returns.  A row whose status is not ok makes the call return
 *                             SMM_ERR_INVALID, smm_last_error naming the first such row.
 *   smm_grib_cpx_decode_host  one row decoded on the host, no device: values[n_values] receives the integers, *status is
 *                             how the row ended (SMM_GRIB_CPX_*).  x_host needs no alignment.  A malformed stream costs
 *                             wrong numbers and a status, never a read outside [0, x_bytes).
 * SMM_ERR_INVALID, before any device is touched: null pointers, a negative count, order outside 0..2 (the mark apart),
 * n_oct outside 1..4 when order > 0, nbits, width_bits or length_bits outside 0..32, width_ref or length_inc above 255,
 * n_groups == 0 with n_values > 0, 0 < n_values <= order, n_values >= 2^31, reserved != 0, a stream that leaves
 * [0, x_bytes), out_bytes below the layout, a misaligned x or out.
 */
int smm_grib_cpx_layout(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes);
int smm_grib_cpx_unpack(int device, const void* x, int64_t x_bytes, const smm_grib_cpx_t* recs /* host */,
                        const smm_grib_row_t* rows_in /* host */, int64_t n_batch, void* out, int64_t out_bytes,
                        smm_grib_row_t* rows_out /* host */, void* stream);
int smm_grib_cpx_decode_host(const void* x_host, int64_t x_bytes, const smm_grib_cpx_t* rec, uint32_t* values, int* status);

/*
 * The three entries above for rows with MISSING VALUES INSIDE THE GROUPS (section 5's octet 23, missing value management
 * 1 or 2: what wgrib2 writes for undefined points instead of a section-6 bitmap; the rule is the text of
 * smmregrid_amd/csrc/smm_grib_cpx.hpp).  smm_grib_cpx_t stays as it is: the octet travels in `mvm`, a HOST array of
 * n_batch values 0, 1 or 2 parallel to recs, or NULL for all zero -- then each entry is the one above in every respect.
 * The device step turns "codes inside the groups" into "a bitmap plus the compacted integers", the form
 * smm_apply_grib_bm / _na take: both kinds of missing become a 0 bit, hence a float32 NaN; the substitute values of
 * octets 24 - 31 are not read.
 *   smm_grib_cpx_layout_mv       a coded row with mvm != 0 gets its slot of n_values * 4 bytes and, behind it, a bitmap
 *                                slot of ceil(n_values / 8) bytes rounded up to 4.  bitmap_off[b] (may be NULL) = where
 *                                that slot starts in `out`, SMM_GRIB_NO_BITMAP for a row without one.
 *   smm_grib_cpx_unpack_mv       bitmaps_out: a HOST array of n_batch records.  A row with mvm != 0: its slot receives
 *                                its P present integers big-endian at the row's own minimal width w_b, every byte of
 *                                ceil(P * w_b / 8) rounded up to 4 written; its bitmap slot receives n_values bits, MSB
 *                                first, zero-padded, every byte of the slot written; bitmaps_out[b] = {the bitmap slot's
 *                                offset in out, P}; rows_out[b].nbits = w_b.  A row with mvm == 0 and a row marked
 *                                SMM_GRIB_CPX_SIMPLE get {SMM_GRIB_NO_BITMAP, n_values} and the bytes of
 *                                smm_grib_cpx_unpack.  Scratch: 8 B per value and 16 B per group as above, and for a row
 *                                with mvm != 0 another 8 B per value and 4 B per 256 values (its integers pass through a
 *                                second array on their way to their ranks).
 *   smm_grib_cpx_decode_host_mv  mvm: one value, or NULL.  present[n_values] receives a flag per coded position,
 *                                *n_present = P, values[n_values] the P compacted integers (zero behind them).  A row
 *                                that does not end ok leaves zeros everywhere.
 * SMM_ERR_INVALID before any device is touched, beside what the entries above refuse: an mvm value above 2 (the row is
 * named), a null bitmaps_out, out_bytes below this layout.
 */
int smm_grib_cpx_layout_mv(const smm_grib_cpx_t* recs, const uint8_t* mvm, int64_t n_batch, uint64_t* byte_off,
                           uint64_t* bitmap_off, uint64_t* total_bytes);
int smm_grib_cpx_unpack_mv(int device, const void* x, int64_t x_bytes, const smm_grib_cpx_t* recs /* host */,
                           const uint8_t* mvm /* host, or NULL */, const smm_grib_row_t* rows_in /* host */, int64_t n_batch,
                           void* out, int64_t out_bytes, smm_grib_row_t* rows_out /* host */,
                           smm_grib_bitmap_t* bitmaps_out /* host */, void* stream);
int smm_grib_cpx_decode_host_mv(const void* x_host, int64_t x_bytes, const smm_grib_cpx_t* rec, const uint8_t* mvm,
                                uint32_t* values, uint8_t* present, uint64_t* n_present, int* status);

/*
 * The way back: simple-packed streams on the device coded as complex-packed streams (templates 5.2 / 5.3), behind the
 * four passes of smm_grib_pack or on any rows an smm_grib_row_t table describes.  THE RULE OF THIS ENCODER is the text of
 * smmregrid_amd/csrc/smm_grib_cpx.hpp: spatial differencing of the wanted order unless a descriptor or a difference would
 * not fit (then order 0), groups of one fixed length, every table at its minimal width.  It is fully deterministic -- the
 * host entry and the kernels give the same bytes -- and it is the project's own choice of groups, not g2c's: a valid
 * stream that smm_grib_cpx_decode_host and smm_grib_cpx_unpack decode.  recs are the parameters WANTED per row: n_values
 * and nbits (the width of the row's integers, 0..32) as the row has them, order (0, 1 or 2) and length_ref = the group
 * length L (8, 16, 32 or 64) to code with; reserved must be 0, nothing else is read.
 *   smm_grib_cpx_pack_bound   host only: the worst case per row, rounded up to 4 -- with m = min(32, nbits + order) and
 *                             NG = ceil(n_values / L): (order + 1) * 4 octets of descriptors (none at order 0), NG
 *                             references of m bits, NG widths of 6 bits, n_values values of m bits, each part rounded up
 *                             to an octet (derived next to pack_bound_bytes in smm_grib_cpx.hpp); a row of no values or
 *                             of width 0 needs none.  byte_off[b] (may be NULL) = the sum before row b, *total_bytes = the
 *                             sum.
 *   smm_grib_cpx_pack         x: device bytes, 4-byte aligned, the allocation covering x_bytes rounded up to 4;
 *                             rows_in[b].byte_off: where row b's n_values integers of nbits bits begin in x; rows_in,
 *                             recs and recs_out: HOST arrays of n_batch records; out: device, 4-byte aligned,
 *                             out_bytes >= the bound.  recs_out[b] is the full record of the stream written (the
 *                             effective order, n_oct, NG, the three table widths, the group lengths, byte_off and
 *                             byte_len in out): rows lie back to back in row order, each at a 4-byte-aligned offset, and
 *                             every byte from a row's start to the aligned end of its stream is written;
 *                             *used_bytes = the aligned end of the last row, bytes of out beyond it are unspecified.
 *                             A row with nbits == 0 is not coded: its record is marked SMM_GRIB_CPX_SIMPLE with byte_len
 *                             0.  Seven kernels (differences and their extremes per row, the order per row, references
 *                             and widths per group, offsets per row, over the rows, shared words zeroed, emit through
 *                             LDS); nothing returns to the host between them.  Scratch (8 B per group, 12 B per 1024
 *                             values) is allocated and freed inside the call; the stream is synchronised before it
 *                             returns.
 *   smm_grib_cpx_encode_host  one row coded on the host, no device: values[n_values] (n_values == rec->n_values, each
 *                             within nbits bits) into out[0, out_cap), *byte_len its bytes, *rec_out its record with
 *                             byte_off 0.  out needs no alignment; out_cap must reach the bound.
 * SMM_ERR_INVALID, before any device is touched: null pointers, negative counts, order outside 0..2, length_ref outside
 * {8, 16, 32, 64}, nbits outside 0..32 or different from rows_in[b].nbits, n_values >= 2^31, reserved != 0, a row's
 * integers leaving [0, x_bytes), out_bytes / out_cap below the bound, a misaligned x or out, a value wider than nbits
 * (host entry).
 */
int smm_grib_cpx_pack_bound(const smm_grib_cpx_t* recs, int64_t n_batch, uint64_t* byte_off, uint64_t* total_bytes);
int smm_grib_cpx_pack(int device, const void* x, int64_t x_bytes, const smm_grib_row_t* rows_in /* host */,
                      const smm_grib_cpx_t* recs /* host */, int64_t n_batch, void* out, int64_t out_bytes,
                      smm_grib_cpx_t* recs_out /* host */, uint64_t* used_bytes, void* stream);
int smm_grib_cpx_encode_host(const uint32_t* values, int64_t n_values, const smm_grib_cpx_t* rec, void* out,
                             int64_t out_cap, uint64_t* byte_len, smm_grib_cpx_t* rec_out);

/*
 * Masked-level apply (regrid.py:387-418 in one launch).  The kept dims of the
 * field are viewed as (n_outer, n_lev, n_inner) around the mask dimension;
 * data level l uses group member level_index[l] (host int32[n_lev], result of
 * the nearest-level match regrid.py:390).  Element offsets:
 *   x row (o,l,i) at  o*xs_outer + l*xs_lev + i*xs_inner
 *   y row (o,l,i) at  o*ys_outer + l*ys_lev + i*ys_inner
 * so both the concat order and the transpose (regrid.py:420-427) are strides.
 * With SMM_APPLY_MASKED, masked_levels (host uint8[n_ops], nullable = all)
 * says per group member whether its dst_imask is applied (regrid.py:405).
 */
int smm_group_apply(smm_group_t g,
                    const void* x, int x_dtype,
                    int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                    void* y, int y_dtype,
                    int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                    int64_t n_outer, int64_t n_lev, int64_t n_inner,
                    const int32_t* level_index, const uint8_t* masked_levels,
                    double remap_area_min, unsigned flags, void* stream);

/*
 * Masked-level apply for a field kept batch-fastest per level: data level l is an (S, ldx >= n_batch)
 * slab at x + l * xs_lev (the n_batch values of a source cell contiguous), its results go to
 * y + l * ys_lev + b * ys_batch + d.  Y as regrid3d lays it out with transpose (B, L, D):
 * ys_lev = D, ys_batch = L * D; without (L, B, D): ys_lev = B * D, ys_batch = D.  With SMM_APPLY_SB_Y_SB
 * the result stays batch-fastest per level, Y (L, D, ys_batch >= B): ys_lev = D * ys_batch.  Same level_index /
 * masked_levels semantics and the same bits as smm_group_apply.  All data levels run in ONE kernel launch (the
 * levels' CSR pointers travel in the kernel arguments; groups of more than 88 data levels take several launches),
 * ordered on `stream` and capturable into a hipGraph after one warm-up call, which uploads the members' CSR copies
 * (smm_group_prepare_sb does that ahead of time).  BASELINE config 3 kept batch-fastest: 14.4 ms with one launch per
 * level, 9.5 ms grouped.
 */
int smm_group_prepare_sb(smm_group_t g);
int smm_group_apply_sb(smm_group_t g,
                       const void* x, int x_dtype, int64_t xs_lev, int64_t ldx,
                       void* y, int y_dtype, int64_t ys_lev, int64_t ys_batch,
                       int64_t n_batch, int64_t n_lev,
                       const int32_t* level_index, const uint8_t* masked_levels,
                       double remap_area_min, unsigned flags, void* stream);

/*
 * Host-buffer variant (the fields Regridder.regrid3d receives): X host C-contiguous
 * (n_outer, n_lev, n_inner, S); Y host (n_outer, n_inner, n_lev, D) when transpose != 0
 * (regrid.py:420-427) else (n_lev, n_outer, n_inner, D) (regrid.py:410).  Chunks flow through the same
 * double-buffered pipeline as smm_apply_host.  Synchronous.  When the selected levels use at most four fifths of their
 * source cells in total (masked ocean levels thin out with depth) and the batch has >= 8 entries, only the used
 * cells travel over PCIe, packed batch-fastest per level: a chunk is a block of the outer axis with every level when
 * the batch has >= 32 entries and 32 of all levels fit the staging budget, else a few consecutive data levels x a block
 * of the outer axis
 * (BASELINE config 3, 106 GB of X in host memory: 37 GB over PCIe, 0.90 s against 2.04 s for whole rows; same bits).
 * SMM_APPLY_HOST_NO_PACK, a forced kernel flag or a caller's chunk_outer keep whole rows / blocks of the outer axis.
 */
int smm_group_apply_host(smm_group_t g,
                         const void* x_host, int x_dtype, void* y_host, int y_dtype,
                         int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                         const int32_t* level_index, const uint8_t* masked_levels,
                         double remap_area_min, unsigned flags, int64_t chunk_outer);

/*
 * The three group entries above for CF-packed fields (SMM_I16 / SMM_U16 X, raw 2-byte elements, decoded inside the
 * kernels), with the contract of smm_apply_cf / smm_apply_sb_cf / smm_apply_host_cf: y_dtype must be SMM_F64
 * (else SMM_ERR_UNSUPPORTED); cf == NULL with a float x_dtype is the plain entry; cf == NULL with an integer x_dtype,
 * cf != NULL with a float one, a fill value outside the raw type, or SMM_APPLY_NO_FILL with n_fill > 0 are
 * SMM_ERR_INVALID.  One decode rule per call: a variable has one set of packing attributes, it applies to every level.
 * The plain group entries refuse the integer codes with SMM_ERR_UNSUPPORTED.  The whole call is validated before
 * the first launch.  level_index / masked_levels, MASKED, SKIPNA, SB_Y_SB, HOST_NO_PACK and KERNEL_SELL work as for
 * float fields, with the bits of decoding on the host and calling the plain entry.
 *   smm_group_apply_cf      native layout, strides in elements of the raw type.  Runs the SELL kernel whatever the
 *                           group's tile plan (smm_group_launch_info says so for SMM_I16 / SMM_U16);
 *                           SMM_APPLY_KERNEL_TILE is SMM_ERR_UNSUPPORTED.
 *   smm_group_apply_sb_cf   per-level (S, ldx) slabs of raw elements, xs_lev in raw elements; all data levels in one
 *                           launch of the grouped batch-fastest kernel as for float fields (the decode rule travels
 *                           in the kernel arguments beside the 88 levels' pointers).  SMM_APPLY_SB_PACKED is refused.
 *   smm_group_apply_host_cf host X (n_outer, n_lev, n_inner, S) of raw elements: staged, packed level-major or per
 *                           outer block and shipped as 2-byte elements (SMM_HOST_STAT_H2D_BYTES counts 2 B per cell).
 *                           The slabs of a packed chunk lie back to back without padding: the kernel's loads need
 *                           element alignment only.
 */
int smm_group_apply_cf(smm_group_t g,
                       const void* x, int x_dtype,
                       int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                       void* y, int y_dtype,
                       int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                       int64_t n_outer, int64_t n_lev, int64_t n_inner,
                       const int32_t* level_index, const uint8_t* masked_levels,
                       double remap_area_min, unsigned flags, void* stream,
                       const smm_cf_decode_t* cf);
int smm_group_apply_sb_cf(smm_group_t g,
                          const void* x, int x_dtype, int64_t xs_lev, int64_t ldx,
                          void* y, int y_dtype, int64_t ys_lev, int64_t ys_batch,
                          int64_t n_batch, int64_t n_lev,
                          const int32_t* level_index, const uint8_t* masked_levels,
                          double remap_area_min, unsigned flags, void* stream,
                          const smm_cf_decode_t* cf);
int smm_group_apply_host_cf(smm_group_t g,
                            const void* x_host, int x_dtype, void* y_host, int y_dtype,
                            int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                            const int32_t* level_index, const uint8_t* masked_levels,
                            double remap_area_min, unsigned flags, int64_t chunk_outer,
                            const smm_cf_decode_t* cf);

/*
 * smm_group_apply / smm_group_apply_host for GRIB simple-packed fields shipped RAW, with or without bitmaps: the masked
 * levels of ocean variables, whose bitmapped streams hold the present cells only.  rows (and bitmaps, or NULL: no row has
 * one, as in smm_apply_grib_bm) are HOST arrays of n_outer * n_lev * n_inner records; batch row (o, l, i) is record
 * (o * n_lev + l) * n_inner + i, data level l uses group member level_index[l].  Every row keeps the semantics of
 * smm_apply_grib_bm -- any width 0..32 and byte alignment, rows in any buffer order and overlapping, rows with and
 * without a bitmap mixed, several rows naming one bitmap_off, a cell whose bitmap bit is 0 a float32 NaN -- and the
 * results are bit-identical to smm_group_apply / smm_group_apply_host with SMM_F32 X on the field a host decode gives.
 * One kernel launch covers all levels (the grouped form of the GRIB gather: grid = destination blocks x batch tiles x
 * levels, the BT batch rows of a thread are rows (o, i) of one level); ahead of it, on the same stream, one build of the
 * rank tables runs over all rows of the call or chunk.  A grid beyond the launch limit is cut over the outer and inner
 * range and, for a single row, over the levels.
 *   smm_group_apply_grib       x device bytes as in smm_apply_grib; Y rows at o*ys_outer + l*ys_lev + i*ys_inner
 *                              (elements, 64-bit) as in smm_group_apply.  The device row table, the bitmap records and the
 *                              rank tables live in buffers the GROUP owns (grown on demand, under a mutex of their own),
 *                              as an operator holds them for smm_apply_grib_bm: calls on one group take turns and are
 *                              ordered against each other only on ONE stream; concurrent calls on different streams
 *                              need one group handle each.
 *   smm_group_apply_host_grib  x_host host bytes; Y host (n_outer, n_inner, n_lev, D) when transpose != 0, else
 *                              (n_lev, n_outer, n_inner, D), pinned or pageable, as smm_group_apply_host.  A chunk is a
 *                              block of consecutive outer indices with all n_lev * n_inner of their rows (consecutive
 *                              records), staged as smm_apply_host_grib_bm stages a chunk and sized by bytes the same
 *                              way -- staged bytes, rank tables and rows * n_dst * 8 of Y against ~256 MiB and an eighth
 *                              of the free device memory -- but never less than one outer index; chunk_outer > 0 fixes
 *                              the outer indices per chunk.  SMM_HOST_STAT_H2D_BYTES counts per row
 *                              40 + (bitmaps ? 16 : 0) + align4(data) + (bitmapped ? align4(ceil(n_src / 8)) : 0).
 * Refusals, before any device is touched, in the order and with the codes of smm_apply_grib_bm: flag bits outside the
 * set; SMM_APPLY_SKIPNA, SMM_APPLY_KERNEL_TILE and the batch-fastest / host-pack flags, and y_dtype != SMM_F64:
 * SMM_ERR_UNSUPPORTED; null pointers, negative counts, a misaligned x (device entry) or y, a bad rule: SMM_ERR_INVALID.
 * Then, SMM_ERR_INVALID all: a NULL group, a level_index entry outside the group, a row or bitmap that leaves
 * [0, x_bytes) for the group's n_src, a used member without the dst_imask / dst_frac the call asks for.
 */
int smm_group_apply_grib(smm_group_t g, const void* x, int64_t x_bytes,
                         const smm_grib_row_t* rows /* host */, const smm_grib_bitmap_t* bitmaps /* host, or NULL */,
                         void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                         int64_t n_outer, int64_t n_lev, int64_t n_inner,
                         const int32_t* level_index, const uint8_t* masked_levels,
                         double remap_area_min, unsigned flags, void* stream);
int smm_group_apply_host_grib(smm_group_t g, const void* x_host, int64_t x_bytes,
                              const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                              void* y_host, int y_dtype,
                              int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                              const int32_t* level_index, const uint8_t* masked_levels,
                              double remap_area_min, unsigned flags, int64_t chunk_outer);

/*
 * The SMM_APPLY_SKIPNA form of the two group entries above, with their argument lists (`bitmaps` may be NULL), as
 * smm_apply_grib_na is the form of smm_apply_grib_bm: the bit is implied and may be passed, every level renormalises
 * over its valid source values with its own member, mask switch and dst_frac, and the result has the bits of
 * smm_group_apply / smm_group_apply_host with SMM_APPLY_SKIPNA | SMM_APPLY_KERNEL_SELL on the float32 field a host
 * decode gives, NaN where the bitmap is 0.  Refusals in the order of smm_apply_grib_na, then those of the twins.
 */
int smm_group_apply_grib_na(smm_group_t g, const void* x, int64_t x_bytes,
                            const smm_grib_row_t* rows /* host */, const smm_grib_bitmap_t* bitmaps /* host, or NULL */,
                            void* y, int y_dtype, int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                            int64_t n_outer, int64_t n_lev, int64_t n_inner,
                            const int32_t* level_index, const uint8_t* masked_levels,
                            double remap_area_min, unsigned flags, void* stream);
int smm_group_apply_host_grib_na(smm_group_t g, const void* x_host, int64_t x_bytes,
                                 const smm_grib_row_t* rows, const smm_grib_bitmap_t* bitmaps,
                                 void* y_host, int y_dtype,
                                 int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                                 const int32_t* level_index, const uint8_t* masked_levels,
                                 double remap_area_min, unsigned flags, int64_t chunk_outer);

/*
 * The three group _cf entries with a CF-packed RESULT, with the contract of smm_apply_pk / smm_apply_sb_pk /
 * smm_apply_host_pk: enc != NULL stores Y as raw 2-byte integers, encoded inside the kernels' stores by *enc; y_dtype
 * must then be SMM_I16 / SMM_U16, y 2-byte aligned, and every Y stride (ys_outer / ys_lev / ys_inner, ys_lev / ys_batch)
 * counts 2-byte elements.  enc == NULL is the _cf entry unchanged.  X is float (cf == NULL) or packed with Y's own raw
 * type (a packed X of the other raw type: SMM_ERR_UNSUPPORTED).  SMM_ERR_INVALID, before any device is touched: enc !=
 * NULL with a float y_dtype, an integer y_dtype without enc, a fill the raw type cannot hold, a zero or non-finite
 * scale, a non-finite offset, reserved != 0.  SMM_APPLY_KERNEL_TILE with enc is SMM_ERR_UNSUPPORTED (the LDS tile kernel
 * is not built for packed results); SMM_APPLY_SB_PACKED stays refused for groups.  One encode rule per call, for every
 * level: a variable has one set of packing attributes.  The whole call is validated before the first launch.
 * level_index / masked_levels, MASKED, SKIPNA, SB_Y_SB, HOST_NO_PACK, KERNEL_SELL and the split of oversized grids
 * behave as for float Y, with the bits of encoding the float64 result of the _cf entry on the host.
 *   smm_group_apply_pk      runs the SELL kernel whatever the group's tile plan.
 *   smm_group_apply_sb_pk   all data levels in one launch of the grouped batch-fastest kernel (the encode rule travels
 *                           in the kernel arguments behind the decode rule); tiles of 64 destination rows, or 16 under the
 *                           tuning knob SMM_TUNE_SB_PACKED_Y_ROWS (as in smm_apply_sb_pk).  A batch-fastest packed result (SB_Y_SB,
 *                           Y (L, D, ys_batch) raw) is what a following smm_apply_sb_cf / smm_group_apply_sb_cf consumes.
 *   smm_group_apply_host_pk Y host (n_outer, n_inner, n_lev, D) or (n_lev, n_outer, n_inner, D) of raw elements: chunks
 *                           are sized, staged, copied back and copied out as 2-byte cells in every form of the pipeline
 *                           (SMM_HOST_STAT_D2H_BYTES counts 2 B per cell) -- a quarter of the float64 result over PCIe.
 */
int smm_group_apply_pk(smm_group_t g,
                       const void* x, int x_dtype,
                       int64_t xs_outer, int64_t xs_lev, int64_t xs_inner,
                       void* y, int y_dtype,
                       int64_t ys_outer, int64_t ys_lev, int64_t ys_inner,
                       int64_t n_outer, int64_t n_lev, int64_t n_inner,
                       const int32_t* level_index, const uint8_t* masked_levels,
                       double remap_area_min, unsigned flags, void* stream,
                       const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);
int smm_group_apply_sb_pk(smm_group_t g,
                          const void* x, int x_dtype, int64_t xs_lev, int64_t ldx,
                          void* y, int y_dtype, int64_t ys_lev, int64_t ys_batch,
                          int64_t n_batch, int64_t n_lev,
                          const int32_t* level_index, const uint8_t* masked_levels,
                          double remap_area_min, unsigned flags, void* stream,
                          const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);
int smm_group_apply_host_pk(smm_group_t g,
                            const void* x_host, int x_dtype, void* y_host, int y_dtype,
                            int64_t n_outer, int64_t n_lev, int64_t n_inner, int transpose,
                            const int32_t* level_index, const uint8_t* masked_levels,
                            double remap_area_min, unsigned flags, int64_t chunk_outer,
                            const smm_cf_decode_t* cf, const smm_cf_encode_t* enc);

/* ------------------------------------------- weight columns and source gradients (opt-in, beyond the reference)
 *
 * Bicubic weights (`cdo genbic`, num_wgts = 4) and second-order conservative weights (SCRIP-style, num_wgts = 3)
 * carry more than the value weight in a row of remap_matrix: weights of the source field's gradients.  The reference
 * applies column 0 alone (weights.py:33) and so does every entry above.  The entries below apply every column:
 *
 *     y[d] = epilogue( sum over the links of d:  w0 * fill(f[s]) + w1 * g1[s] + ... + w(K-1) * g(K-1)[s] )
 *
 * with g1 .. g(K-1) gradients of each batch row, computed on the device from the row itself.
 *
 * The gradient rule (stated in numpy by smmregrid_amd.gradients.GradientRule, which also makes the tables).  The source
 * is a regular lon/lat grid of nx * ny cells, nx fastest; f is widened to float64 first.  A neighbour is ABSENT when it
 * lies outside the grid (j beyond the first or last row; i beyond the ends unless `periodic`, which wraps) or its value
 * is not finite; src_grid_imask is not consulted.  With i+ / i- the east / west and j+ / j- the next / previous row:
 *     g_i [j,i] = ((f[j,i+] - f[j,i-]) * si[c * nx + i]) * ci[j]
 *     g_j [j,i] =  (f[j+,i] - f[j-,i]) * sj[c * ny + j]
 *     g_ij[j,i] = ((g_j[j,i+] - g_j[j,i-]) * si[c * nx + i]) * ci[j]      presence still judged on f
 * an absent side is replaced by the cell itself; c = 0 with both sides present, 1 with the + side only, 2 with the -
 * side only.  With both sides absent, or f[j,i] itself not finite, the gradient is exactly +0.0.  The tables are made
 * on the host in float64 (1 / spacing, 1 / cos lat, signs): the device multiplies, it never divides, and keeps every
 * multiply and subtract apart (no FMA).  A non-finite cell still enters the sum through column 0 as ever (the 1e20
 * fill, then > 1e19 -> NaN), so the NaN footprint of a result is that of the column-0 result.  This is SCRIP's
 * masked-neighbour convention as recalled, not pinned against a CDO run.
 */
enum { SMM_GRAD_I = 0, SMM_GRAD_J = 1, SMM_GRAD_IJ = 2 };   /* plane kinds */
typedef struct smm_grad_plan* smm_grad_plan_t;              /* the tables of one source grid, resident in HBM */

/* smm_operator_create_opt for links with n_cols weights each, 1..4: w is double[nnz * n_cols], rows as in remap_matrix.
 * The sort by (dst, src), the tie-break and the sequential duplicate summing are applied to every column with the same
 * permutation; SMM_CREATE_PRUNE_ZEROS drops a link only when all its columns are zero.  Column 0 of such an operator is
 * exactly the operator smm_operator_create_opt builds from column 0, and every other entry works on it unchanged; the
 * extra columns are kept as SELL slot planes beside it (padded slots +0.0) for smm_apply_cols. */
int smm_operator_create_cols(int64_t n_src, int64_t n_dst, int64_t nnz, const int32_t* src_addr_1based,
                             const int32_t* dst_addr_1based, const double* w, int n_cols, unsigned options,
                             int device, smm_operator_t* out);
int smm_operator_cols(smm_operator_t op, int* n_cols);
/* every column of the canonical CSR for parity tests: val double[nnz * n_cols], link p's weights at val + p * n_cols, the
 * links in the order of smm_operator_export_csr */
int smm_operator_export_cols(smm_operator_t op, double* val);

/* The gradient tables of one source grid: plane_kind int[n_planes] (SMM_GRAD_*) in the order of the weight columns
 * 1.., si double[3 * nx], sj double[3 * ny], ci double[ny] (host arrays, copied).  SMM_ERR_INVALID, before any device is
 * touched: nx or ny < 1, nx * ny beyond int32, n_planes outside 1..3, a null table, an unknown plane kind, an IJ plane
 * without a J plane. */
int smm_grad_plan_create(int64_t nx, int64_t ny, int periodic, int n_planes, const int* plane_kind, const double* si,
                         const double* sj, const double* ci, int device, smm_grad_plan_t* out);
int smm_grad_plan_destroy(smm_grad_plan_t plan);
/* The planes of n_batch rows: x device (n_batch, ldx >= nx * ny) of x_dtype SMM_F32 / SMM_F64 (anything else:
 * SMM_ERR_UNSUPPORTED); g device double, plane p of row b at g + b * ld_row + p * ld_plane (ld_plane >= nx * ny,
 * ld_row >= (n_planes - 1) * ld_plane + nx * ny).  One stencil kernel: lanes run along i, a workgroup walks a band of
 * rows and keeps the three source rows it needs in LDS, so f is read once (plus two halo rows per band) and every plane
 * is written once.  Stream-ordered; allocates nothing. */
int smm_gradients(smm_grad_plan_t plan, const void* x, int x_dtype, int64_t ldx, double* g, int64_t ld_plane,
                  int64_t ld_row, int64_t n_batch, void* stream);

/* The K-column apply: op from smm_operator_create_cols with K = n_cols >= 2, plan with K - 1 planes on a grid of
 * nx * ny == n_src cells.  x, ldx, y, ldy, n_batch, remap_area_min and stream as for smm_apply.  `scratch` is device
 * memory for the planes, 8-byte aligned: the call computes the planes of as many batch rows as fit in scratch_bytes,
 * gathers them, and goes on until all rows are done; it allocates nothing and refuses (SMM_ERR_INVALID) only when not
 * even one row's planes -- (K - 1) * n_src * 8 bytes -- fit.  smm_apply_cols_scratch reports the bytes that hold all
 * n_batch rows at once.
 * The gather is the row-per-lane SELL-64 kernel reading one column index and K weights per slot; links in ascending
 * source index, per link the columns 0 .. K-1 in order, separate multiply and add into one accumulator per batch row.
 * The result is bit for bit what smm_apply gives with SMM_APPLY_KERNEL_SELL on the "stacked" operator -- K * n_src
 * source cells, link (d, s, k) at source index s * K + k -- and the stacked float64 field X[b, s * K + k], k = 0 holding
 * f filled with its own dtype's 1e20 and widened, k >= 1 plane k.  SMM_APPLY_MASKED and SMM_APPLY_NO_FILL work as for
 * smm_apply (unfilled, a non-finite f enters through the links of its own rows alone, as on the stacked operator);
 * SMM_APPLY_KERNEL_SELL is accepted (it is the kernel that runs).  A launch grid the rounds were not planned to fit is
 * SMM_ERR_INVALID, never launched.
 * Built: SMM_F32 and SMM_F64 fields to SMM_F64 results in the native (B, S) layout.  SMM_ERR_UNSUPPORTED, checked
 * before the handles are looked at: SMM_APPLY_SKIPNA, SMM_APPLY_KERNEL_TILE, the batch-fastest and host-pack flags,
 * packed / half x_dtype (GRIB fields have no entry of this kind), any y_dtype but SMM_F64.  Level groups have no
 * such entry. */
int smm_apply_cols(smm_operator_t op, smm_grad_plan_t plan, const void* x, int x_dtype, int64_t ldx, void* y,
                   int y_dtype, int64_t ldy, int64_t n_batch, double remap_area_min, unsigned flags, void* scratch,
                   size_t scratch_bytes, void* stream);
int smm_apply_cols_scratch(smm_operator_t op, int64_t n_batch, size_t* bytes);

/* ------------------------------------------- categorical fields (opt-in, beyond the reference)
 *
 * Every entry above is a weighted sum of source values.  That is wrong for a field of class codes -- land cover, soil
 * and vegetation type, masks, precipitation type: classes 3 and 7 do not average to 5.  smm_apply_mode stores, per
 * destination cell, the class that covers the largest summed share of it ("largest area fraction").  This is CDO's
 * remaplaf as recalled; it is not pinned against a cdo run.  The rule depends on the values, so no weights file
 * expresses it: weights made with method "laf" hold one link per target cell, to the single source cell of largest
 * overlap -- a static approximation.  Meant for conservative weights; on one-link rows it is the identity on the link.
 *
 * The rule (stated in numpy by smmregrid_amd.categorical.ModeRule), for destination row d, batch row b and the links k
 * of the canonical CSR in ascending source order, w_k the weight of column 0:
 *   missing  For SMM_F32 / SMM_F64, x[b, col_k] is missing when it is not finite; for SMM_I16 / SMM_U16 when it equals
 *            one of the first n_fill entries of fill[2], compared on the raw integer.  A missing link takes part in no
 *            class.
 *   classes  Two links are of one class when their values compare equal with == (so -0.0 and +0.0 are one class); a
 *            class is represented by the value of its first link.  share(c) is the sum of w_k over the links of class
 *            c: float64, from +0.0, in ascending link order, one add per link -- the bits of smm_apply on the float64
 *            indicator field x == c (w * 1.0 is w, w * 0.0 is +-0, and a sum that starts at +0.0 is never -0.0).
 *   row sums tot = the sum of w_k over all links of the row, val = the same over the links that are not missing, both
 *            in that order from +0.0: a row without a missing link has val bit-equal to tot.
 *   winner   The class of the largest share, which must be > 0.0.  Bit-equal shares: the class whose first link comes
 *            first wins (walk the first links in order, replace the best on a strictly greater share only).
 *   dead     A row is dead when it is masked (SMM_APPLY_MASKED and dst_imask[d] == 0), when no class has a share > 0
 *            (no links, all missing, all weights <= 0), or when remap_area_min > 0 and
 *            frac_d * (val / tot) < remap_area_min, frac_d = dst_frac[d].  remap_area_min > 0 without dst_frac, and
 *            MASKED without dst_imask, are refused as smm_apply with SMM_APPLY_SKIPNA refuses them.
 *   result   y[b, d], of the field's own type, holds the winner's representative value bit for bit; a dead row NaN
 *            (floats) or fill_out (integers).  share[b, d] (optional, float64) holds the winner's share as summed
 *            above, not divided by anything; a dead row +0.0.
 * There is no 1e20 fill, no > 1e19 test and no SMM_APPLY_NO_FILL; the rule works for any weights.
 */
typedef struct smm_mode_rule_t {
  int32_t n_fill;     /* 0..2: how many entries of fill are missing values */
  int32_t fill[2];    /* raw integers of the field's type */
  int32_t fill_out;   /* what a dead row stores */
  int32_t reserved;   /* 0 */
} smm_mode_rule_t;

/* x device (n_batch, ldx >= n_src) of x_dtype SMM_F32 / SMM_F64 / SMM_I16 / SMM_U16; y device (n_batch, ldy >= n_dst)
 * of the same type; share device double (n_batch, ld_share >= n_dst) or NULL; rule NULL for float fields, required for
 * integer ones.  Native (B, S) layout, stream-ordered, allocates nothing.  An operator from smm_operator_create_cols
 * works through its column 0.
 * The kernel walks the operator's SELL-64 tables, one destination row per lane: a slice's values are gathered once into
 * LDS and the class scan -- O(links * distinct classes) per row -- runs from there; a slice with more slots than the
 * LDS holds (smm_mode_launch_info) gathers from x again inside the scan, which is right for any length and slow.
 * flags: SMM_APPLY_MASKED; SMM_APPLY_KERNEL_SELL is accepted (it is the kernel that runs); unknown bits are
 * SMM_ERR_INVALID.  SMM_ERR_UNSUPPORTED, checked before the handles are looked at: SMM_APPLY_SKIPNA, SMM_APPLY_NO_FILL,
 * SMM_APPLY_KERNEL_TILE, the batch-fastest and host-pack flags, SMM_F16 / SMM_BF16 and any other x_dtype.
 * SMM_ERR_INVALID, before any device is touched: a rule with a float field or an integer field without one, n_fill
 * outside 0..2, a fill or fill_out the raw type cannot hold, reserved != 0, ldx < n_src, ldy < n_dst, ld_share < n_dst,
 * misaligned pointers, a negative n_batch.  Level groups, batch-fastest fields and host buffers have no such entry. */
int smm_apply_mode(smm_operator_t op, const void* x, int x_dtype, int64_t ldx, void* y, int64_t ldy, double* share,
                   int64_t ld_share, int64_t n_batch, double remap_area_min, unsigned flags, const smm_mode_rule_t* rule,
                   void* stream);
/* How smm_apply_mode would run op for fields of x_dtype (nothing is launched; every out pointer may be NULL): capacity =
 * the most slots of a slice the LDS form takes (it depends on x_dtype alone: op may then be NULL); lds_slots = the slots
 * per wave a launch asks for, min(capacity, the operator's longest row), and lds_bytes what that is per workgroup;
 * n_lds_slices / n_global_slices = the slices that take each form. */
int smm_mode_launch_info(smm_operator_t op, int x_dtype, int* capacity, int* lds_slots, int64_t* lds_bytes,
                         int64_t* n_lds_slices, int64_t* n_global_slices);

/* Test hook of the two host pipelines' error path: chunk number `chunk` (0-based) of every following
 * smm_apply_host / smm_group_apply_host call fails with SMM_ERR_HIP before its copies are queued;
 * chunk < 0 (the initial state) switches it off.  Process-wide; for tests only. */
int smm_debug_fail_at_chunk(int64_t chunk);
/* Test hook of the staging pool behind the host pipelines (one persistent set of worker threads per process, started
 * on first need): no_threads != 0 = behave as if no worker thread could be started (the calling thread then does the
 * staging alone: same bits); throw_in_task >= 0 = the staging task started after that many others throws
 * std::bad_alloc, which the pipeline must turn into SMM_ERR_ALLOC after draining the copies in flight; -1 = off.
 * Process-wide; for tests only. */
int smm_debug_staging_faults(int no_threads, int64_t throw_in_task);

/* Where the host pipelines (smm_apply_host / smm_group_apply_host) spent their time, summed over the calls of this
 * process since the last reset: out[i] for i < n receives entry i of the list below (ms unless said otherwise).
 * STAGE_IN = pack / copy into the pinned staging (calling thread + the staging pool), COPY_OUT = pinned staging ->
 * the caller's Y, WAIT = the calling thread blocked on a chunk's stream; H2D / KERNEL / D2H = per chunk from HIP
 * events on the chunk's stream, summed (the two streams overlap, so the sums may exceed TOTAL, the wall time of the
 * calls).  reset != 0 zeroes the sums afterwards.  For benchmarks and tests. */
enum {
  SMM_HOST_STAT_CALLS = 0, /* count */
  SMM_HOST_STAT_CHUNKS,    /* count */
  SMM_HOST_STAT_STAGE_IN_MS,
  SMM_HOST_STAT_H2D_MS,
  SMM_HOST_STAT_KERNEL_MS,
  SMM_HOST_STAT_D2H_MS,
  SMM_HOST_STAT_COPY_OUT_MS,
  SMM_HOST_STAT_WAIT_MS,
  SMM_HOST_STAT_TOTAL_MS,
  SMM_HOST_STAT_THREADS,   /* staging threads in force at the last call (count) */
  SMM_HOST_STAT_H2D_BYTES, /* bytes queued host -> device (X as shipped: packed or whole rows, 2 B per cell of a packed field) */
  SMM_HOST_STAT_D2H_BYTES, /* bytes queued device -> host (Y) */
  SMM_HOST_STAT_COUNT
};
int smm_debug_host_stats(double* out, int n, int reset);

/* Launch grids are 1-D: a batch whose grid would exceed 2^31 - 1 workgroups is cut into parts that are
 * launched one after the other on the same stream (smm_apply / smm_group_apply: halves of the outer batch
 * range, then of the inner one; smm_apply_sb: runs of whole 128-entry batch tiles).  This test hook lowers
 * that limit so that small inputs reach the split path; 0 restores the default.  Process-wide; for tests only. */
int smm_debug_set_grid_limit(int64_t max_blocks);

/* Tuning knobs of tests, tools and benchmarks -- NOT part of the apply flags, product callers never set them.
 * Every knob only changes how a launch is shaped (which kernel form, how many rows per workgroup, which stream);
 * the results are bit-identical for every value.  value 0 restores the library's own choice; *previous (may be
 * NULL) receives the former value.  Process-wide; set them while no apply call is in flight. */
enum {
  SMM_TUNE_SELL_BATCH_ROWS = 0, /* row-per-lane kernel: batch rows per thread (2, 4, 8)                         */
  SMM_TUNE_TILE_WALK,           /* tile kernel: batch rows walked by one workgroup                             */
  SMM_TUNE_TILE_STAGING,        /* tile kernel: 1 = source tiles staged through registers, 2 = by LDS-DMA      */
  SMM_TUNE_TILE_ROWS_PER_STEP,  /* tile kernel, small tiles: batch rows staged per step (1, 2, 4)              */
  SMM_TUNE_TILE_X_LOADS,        /* tile kernel: 1 = non-temporal, 2 = cached loads of X                        */
  SMM_TUNE_TILE_SPLIT_ROWS,     /* tile kernel, part-of-a-slice blocks: 1 = rows are not split over lane groups */
  SMM_TUNE_TILE_LINKS,          /* single-wave tile kernel: 1 = links streamed per batch row, not kept in registers */
  SMM_TUNE_XCD_RUN,             /* tile + batch-fastest kernels: consecutive blocks per XCD (-1 = dispatcher order) */
  SMM_TUNE_SB_STRIP,            /* batch-fastest kernel: destination tiles per strip (-1 = whole-grid order)   */
  SMM_TUNE_SB_LOADS,            /* batch-fastest kernel: loads per batch of the link walk (4, 8)               */
  SMM_TUNE_SB_LEVEL_LAUNCHES,   /* smm_group_apply_sb: 1 = one launch per data level instead of one grouped launch */
  SMM_TUNE_SB_LDS_PAD,          /* batch-fastest kernels: extra LDS bytes per wave, capping the waves per CU    */
  SMM_TUNE_HOST_PACK_STORES,    /* host pipelines: 1 = the pack writes its staging block with plain (not non-temporal) stores */
  SMM_TUNE_HOST_CHUNK_KB,       /* smm_group_apply_host: > 0 forces level-major packed chunks with this staging budget in KiB (default: 256 MiB, only when a block of the outer axis with all levels does not fit) */
  SMM_TUNE_SB_PACKED_Y_ROWS,    /* batch-fastest kernel, packed Y (_pk entries): destination rows per tile, 16 or 64 */
  SMM_TUNE_COUNT
};
int smm_debug_set_tuning(int knob, int value, int* previous);

/* Host threads of operator creation (the sort / duplicate sum replacing weights.py:25-44, the SELL layout and
 * the tile plans are built on several cores) and of the host pipelines' staging copies (one persistent worker
 * pool per process): n > 0 fixes the count, 0 (the initial state) = automatic -- the CPUs the process may really
 * use (scheduler affinity capped by the cgroup CPU quota), at most 16, creations running at the same moment
 * sharing them.  Results do not depend on the count.  *previous (may be NULL) receives the former setting.
 * Process-wide. */
int smm_set_host_threads(int n, int* previous);

/* ------------------------------------------------- multi-GPU exchange (RCCL over xGMI) */

/*
 * One process per GPU; batch rows are sharded over the ranks with no collective on the data
 * path; these calls move the Y shards afterwards.  Rank 0 obtains an id with
 * smm_comm_unique_id, distributes its SMM_COMM_ID_BYTES bytes to the other ranks by any
 * host channel, then every rank (after smm_set_device) calls smm_comm_create.  librccl is
 * bound at run time; SMM_ERR_UNSUPPORTED if it cannot be loaded.
 *   gather   : root's recv_dev holds n_ranks * count elements, rank r's shard at r * count
 *   allgather: every rank's recv_dev holds n_ranks * count elements
 * Both are asynchronous on `stream`.
 */
#define SMM_COMM_ID_BYTES 128
typedef struct smm_comm* smm_comm_t;
int smm_comm_unique_id(void* id_out);
int smm_comm_create(const void* id, int n_ranks, int rank, smm_comm_t* out);
int smm_comm_destroy(smm_comm_t c);
int smm_comm_gather(smm_comm_t c, const void* send_dev, void* recv_dev, int64_t count, int dtype,
                    int root, void* stream);
int smm_comm_allgather(smm_comm_t c, const void* send_dev, void* recv_dev, int64_t count, int dtype,
                       void* stream);

#ifdef __cplusplus
}
#endif
#endif /* SMMREGRID_AMD_H */
