// GRIB-2 complex packing (data representation template 5.2) and complex packing with spatial differencing (5.3), what
// NCEP's g2c / wgrib2 write for GFS, GEFS, HRRR: the decoder and the encoder, each stated once.  Plain C++ that compiles
// for host and device -- the host decode (smm_grib_cpx_decode_host), the kernels of smm_grib_cpx_unpack
// (smm_grib_cpx.hip) and tests/cpp/grib_cpx_harness.cpp all read the stream through Stream::peek (smm_grib_codec.hpp's
// load_word / bits_of) and take the tables apart with the small functions below; the host encode
// (smm_grib_cpx_encode_host), the kernels of smm_grib_cpx_pack (smm_grib_cpx_pack.hip) and
// tests/cpp/grib_cpx_encode_harness.cpp share decide / z_of / coded_row / pack_bound_bytes behind decode_row.
//
// THE FORMAT.  Octets are WMO's (FM 92 GRIB edition 2), as recalled: no file written by g2c, wgrib2 or ecCodes was at
// hand to pin them.
//   section 5, template 5.2 (47 octets)
//     12-15 R (IEEE f32)   16-17 E   18-19 D (sign-magnitude)   20 nbits, the width of the group references
//     21 type of original values   22 group splitting method   23 missing value management m (0, 1 or 2: MISSING
//     VALUES INSIDE THE GROUPS below)
//     24-27, 28-31 missing value substitutes (not read)   32-35 NG, the number of groups   36 reference for group widths
//     37 bits per stored group width   38-41 reference for group lengths   42 length increment
//     43-46 true length of the last group   47 bits per stored scaled group length
//   template 5.3 (49 octets) adds   48 order of spatial differencing (1 or 2)   49 n_oct, octets per extra descriptor
//   section 7, from octet 6 (byte_off of the record; every part starts on an octet)
//     1. only 5.3: h_1 .. h_order, the first values, then g, the overall minimum of the differences; each n_oct octets,
//        sign-magnitude with the top bit as the sign
//     2. NG group references of nbits bits          3. NG stored widths of width_bits bits
//     4. NG stored scaled lengths of length_bits bits
//     5. the groups' values back to back: group g holds L_g values of w_g bits
//   groups     w_g = width_ref + stored width;  L_g = length_ref + length_inc * stored length for g < NG - 1,
//              L_(NG-1) = length_last;  z_i = ref_g(i) + stored value (0 when w_g == 0; every ref is 0 when nbits == 0)
//   integers   order 0: X_i = z_i.  order 1: X_0 = h_1, X_i = X_(i-1) + z_i + g.  order 2: X_0 = h_1, X_1 = h_2,
//              X_i = 2 X_(i-1) - X_(i-2) + z_i + g.  The stream holds n_values stored values, the `order` leading
//              placeholders included: they are read past, not used.  All of it in 64-bit two's complement with
//              wrap-around (computed as uint64): host and device agree on every input, malformed ones included
//   the field  value = (R + X * 2^E) / 10^D: smm_grib_row_t's rule with q = X
// THE SAME AS PREFIX SUMS (what the kernels compute): with a_0 = h_1, a_1 = h_2 - 2 h_1 (order 2 only) and
// a_i = z_i + g from i = order on, X is the inclusive prefix sum of a taken `order` times, modulo 2^64.
//
// MISSING VALUES INSIDE THE GROUPS (octet 23, m = 1 or 2; decode_row_mv, the _mv entries).  The wording is g2c's
// comunpack as recalled: no file written by NCEP's tools was at hand to pin it.  The row codes N = n_values positions;
// s_i is the stored value of position i, w_g and r_g the width and reference of its group.  Every comparison is made in
// 64 bits, so a code that would be negative (2^0 - 2) matches nothing.
//   w_g > 0    position i is missing iff s_i == 2^w_g - 1, or m == 2 and s_i == 2^w_g - 2; else present with
//              z = r_g + s_i.  (w_g == 1 under m == 2: both stored values are codes.  w_g == 32: the code is 0xFFFFFFFF)
//   w_g == 0   the whole group is missing iff r_g == 2^nbits - 1, or m == 2 and r_g == 2^nbits - 2; else every position
//              is present with z = r_g.  (nbits == 0: r_g = 0 = 2^0 - 1, the group is missing)
//   compaction the present values in order form c_0 .. c_(P-1); spatial differencing is undone over THAT sequence, not
//              over the positions: a_0 = h_1, a_1 = h_2 - 2 h_1 (order 2 only), a_k = c_k + g for k >= order, and X is
//              the inclusive prefix sum of a taken `order` times modulo 2^64 over k < P.  The placeholders are the first
//              `order` PRESENT values wherever they lie in the row.  P may be 0 or at most `order`: the prefix-sum form
//              gives X_0 = h_1 and X_1 = h_2 as it stands
//   the field  the cell at position i is (R + X_rank(i) * 2^E) / 10^D when present and a float32 NaN when missing, both
//              kinds of missing alike; the substitutes of octets 24-31 are not read
//   statuses   as below, over the P integers; a row with P == 0 is ok
// What the device step makes of such a row is a simple-packed row with a bitmap: N bits, MSB first, and the P integers.
//
// A ROW ENDS AS (first that applies)
//   kInvalid    NG > n_values -- a group of no values is no group; it bounds the scratch by the record
//   kExhausted  the descriptors and the three tables do not fit into byte_len
//   kInvalid    some w_g > 32, or some L_g > n_values, or the lengths do not sum to n_values
//   kExhausted  the groups' bits leave the stream
//   kInvalid    some X_i outside [0, 2^32)
// and its integers are then zero.  TWO RULES bound every loop and every read: (1) every loop runs over NG or n_values of
// the record; (2) no load goes past the 32-bit word that holds the stream's last byte (load_word clamps; a stream of no
// bytes is never loaded from).  A malformed stream costs wrong numbers and a status, never a read outside the buffer.
//
// THE RULE OF THIS ENCODER (smm_grib_cpx_encode_host: encode_row below; smm_grib_cpx_pack: the kernels of
// smm_grib_cpx_pack.hip; tests/cpp/grib_cpx_encode_harness.cpp).  A row brings n integers X of nbits_in bits -- a
// simple-packed stream --, a wanted order o of 0, 1 or 2 and a group length L of 8, 16, 32 or 64.
//   1. effective order   o falls to 0 when n <= o; when |h_1|, |h_2| or |g| exceeds 2^31 - 1 (a descriptor is
//      sign-magnitude in at most 4 octets); when some z >= 2^32.  There is no cascade from 2 to 1.  A row with
//      nbits_in <= 29 never falls back: with X < 2^29, h < 2^29, |d| <= 2 (2^29 - 1) < 2^30 at order 2 (less at order
//      1), so |g| < 2^30, and z = d - g <= max d - min d <= 4 (2^29 - 1) < 2^31
//   2. differences       order 1: d_i = X_i - X_(i-1); order 2: d_i = X_i - 2 X_(i-1) + X_(i-2); g = min d_i over i >= o;
//      z_i = d_i - g for i >= o and 0 for the o placeholders; h_1 = X_0, h_2 = X_1.  Order 0: z = X, no descriptors
//      (n_oct = 0).  n_oct is the smallest of 1..4 that holds h_1 .. h_o and g
//   3. groups            all of length L but the last: NG = ceil(n / L), length_inc = 1, length_bits = 0,
//      length_last = n - (NG - 1) L, length_ref = L when NG > 1, else n.  ref_g = min z of the group,
//      w_g = the bit length of (max z - ref_g)
//   4. table widths      each the smallest that holds its table: nbits = bit length of max ref_g, width_ref = min w_g,
//      width_bits = bit length of (max w_g - width_ref)
//   5. the stream        descriptors | NG references | NG widths | an empty lengths table | the groups' bits, each part
//      padded to an octet with zero bits
//   6. special rows      n = 0: NG = 0 and no bytes.  nbits_in = 0: the row is not coded, it passes through marked
//      SMM_GRIB_CPX_SIMPLE with byte length 0
// The rule is deterministic -- host and kernels give the same bytes -- and it is the project's own choice of groups, not
// g2c's: a valid 5.2 / 5.3 stream that decode_row above inverts.  Its bound is derived at pack_bound_bytes.
#pragma once

#include <cstdint>

#include "smm_grib_codec.hpp"

namespace smm_cpx {

enum : int { kOk = SMM_GRIB_CPX_OK, kExhausted = SMM_GRIB_CPX_EXHAUSTED, kInvalid = SMM_GRIB_CPX_INVALID };

struct Row {   // smm_grib_cpx_t without its padding
  uint64_t byte_off, byte_len;
  uint32_t n_values, n_groups;
  int32_t nbits;
  uint32_t width_ref;
  int32_t width_bits;
  uint32_t length_ref, length_inc, length_last;
  int32_t length_bits, order, n_oct;
};

SMM_GRIB_HD Row row_of(const smm_grib_cpx_t& c) {
  return Row{c.byte_off, c.byte_len, (uint32_t)c.n_values, c.n_groups, c.nbits, c.width_ref, c.width_bits,
             c.length_ref, c.length_inc, c.length_last, c.length_bits, c.order, c.n_oct};
}

// where the parts of a row's stream begin, as absolute bit positions in x
struct Sections {
  uint64_t refs_bit, widths_bit, lengths_bit, data_bit, bit_end;
  int status;
};
SMM_GRIB_HD Sections sections(const Row& r) {
  const uint64_t ng = r.n_groups;
  const uint64_t head = r.order > 0 ? (uint64_t)(r.order + 1) * (uint64_t)r.n_oct : 0;
  const uint64_t refs = (ng * (uint64_t)r.nbits + 7) / 8, widths = (ng * (uint64_t)r.width_bits + 7) / 8,
                 lengths = (ng * (uint64_t)r.length_bits + 7) / 8;
  Sections s;
  s.refs_bit = 8 * (r.byte_off + head);
  s.widths_bit = s.refs_bit + 8 * refs;
  s.lengths_bit = s.widths_bit + 8 * widths;
  s.data_bit = s.lengths_bit + 8 * lengths;
  s.bit_end = 8 * (r.byte_off + r.byte_len);
  s.status = ng > r.n_values ? kInvalid : head + refs + widths + lengths > r.byte_len ? kExhausted : kOk;
  return s;
}

// the row's bytes as a bit stream: rule (2)
struct Stream {
  const void* x;
  uint64_t last_word, end_byte;
  bool empty;
  // the n (0..32) bits at absolute bit position p
  SMM_GRIB_HD uint32_t peek(uint64_t p, int n) const {
    if (n <= 0 || empty) return 0u;
    const uint64_t w = p >> 5;
    return smm_grib::bits_of(smm_grib::load_word(x, w, last_word, end_byte), smm_grib::load_word(x, w + 1, last_word, end_byte),
                             (unsigned)(p & 31), n);
  }
};
SMM_GRIB_HD Stream stream_of(const void* x, const Row& r) {
  Stream s;
  s.x = x;
  s.end_byte = r.byte_off + r.byte_len;
  s.empty = r.byte_len == 0;
  s.last_word = s.empty ? 0 : (s.end_byte - 1) >> 2;
  return s;
}

// a sign-magnitude number of n_oct octets as a 64-bit two's complement one
SMM_GRIB_HD uint64_t sign_magnitude(uint32_t v, int n_oct) {
  const uint32_t sign = 1u << (8 * n_oct - 1);
  const uint64_t mag = v & (sign - 1u);
  return (v & sign) ? (uint64_t)0 - mag : mag;
}
// h_1, h_2 and g of a row whose sections fit (order 0: all zero; order 1: h_2 = 0)
SMM_GRIB_HD void descriptors(const Stream& s, const Row& r, uint64_t* h1, uint64_t* h2, uint64_t* gmin) {
  *h1 = *h2 = *gmin = 0;
  if (r.order <= 0) return;
  const int nb = 8 * r.n_oct;
  const uint64_t p = 8 * r.byte_off;
  *h1 = sign_magnitude(s.peek(p, nb), r.n_oct);
  if (r.order > 1) *h2 = sign_magnitude(s.peek(p + (uint64_t)nb, nb), r.n_oct);
  *gmin = sign_magnitude(s.peek(p + (uint64_t)r.order * (uint64_t)nb, nb), r.n_oct);
}
// a_i of the prefix-sum form for i < order
SMM_GRIB_HD uint64_t seed(uint32_t i, uint64_t h1, uint64_t h2) { return i == 0 ? h1 : h2 - 2 * h1; }

// width and length of group g (g < NG); both may be anything a malformed table holds
SMM_GRIB_HD void group_of(const Stream& s, const Row& r, const Sections& sec, uint32_t g, uint64_t* w, uint64_t* len) {
  *w = (uint64_t)r.width_ref + s.peek(sec.widths_bit + (uint64_t)g * (uint64_t)r.width_bits, r.width_bits);
  *len = g + 1 < r.n_groups
             ? (uint64_t)r.length_ref + (uint64_t)r.length_inc * s.peek(sec.lengths_bit + (uint64_t)g * (uint64_t)r.length_bits, r.length_bits)
             : (uint64_t)r.length_last;
}
SMM_GRIB_HD uint64_t group_ref(const Stream& s, const Row& r, const Sections& sec, uint32_t g) {
  return s.peek(sec.refs_bit + (uint64_t)g * (uint64_t)r.nbits, r.nbits);
}
// the bit length of a row's largest X: the width its integers are stored with
SMM_GRIB_HD int width_of(uint32_t xmax) { return xmax ? 32 - __builtin_clz(xmax) : 0; }

// ---- the scalar decode: one row into out[0, n_values).  Returns the row's status; not ok: out is all zero.
SMM_GRIB_HD int decode_row(const void* x, const Row& r, uint32_t* out) {
  const uint32_t n = r.n_values, ng = r.n_groups;
  if (n == 0) return kOk;
  const Sections sec = sections(r);
  const Stream s = stream_of(x, r);
  int status = sec.status;
  if (status == kOk) {
    uint64_t sum_len = 0, sum_bits = 0;
    for (uint32_t g = 0; g < ng && status == kOk; ++g) {
      uint64_t w, len;
      group_of(s, r, sec, g, &w, &len);
      if (w > 32 || len > n) status = kInvalid;
      sum_len += len;
      sum_bits += w * len;
      if (sum_len > n) status = kInvalid;
    }
    if (status == kOk && sum_len != n) status = kInvalid;
    if (status == kOk && sum_bits > sec.bit_end - sec.data_bit) status = kExhausted;
  }
  if (status == kOk) {
    uint64_t h1, h2, gmin;
    descriptors(s, r, &h1, &h2, &gmin);
    uint64_t pos = sec.data_bit, x1 = 0, x2 = 0, high = 0;
    uint32_t i = 0;
    for (uint32_t g = 0; g < ng; ++g) {
      uint64_t w, len;
      group_of(s, r, sec, g, &w, &len);
      const uint64_t ref = group_ref(s, r, sec, g);
      for (uint64_t k = 0; k < len; ++k, ++i, pos += w) {
        const uint64_t z = ref + s.peek(pos, (int)w);
        uint64_t X;
        if (r.order <= 0)
          X = z;
        else if (i == 0)
          X = h1;
        else if (r.order == 1)
          X = x1 + z + gmin;
        else if (i == 1)
          X = h2;
        else
          X = 2 * x1 - x2 + z + gmin;
        x2 = x1;
        x1 = X;
        high |= X >> 32;
        out[i] = (uint32_t)X;
      }
    }
    if (high) status = kInvalid;
  }
  if (status != kOk)
    for (uint32_t i = 0; i < n; ++i) out[i] = 0;
  return status;
}

// ---- MISSING VALUES INSIDE THE GROUPS.  Whether a position of a group of width w (0..32) and reference ref is missing
// under m (1 or 2): s is its stored value (0 when w == 0), nbits the width of the references
SMM_GRIB_HD bool is_missing(int m, uint64_t w, int nbits, uint64_t ref, uint64_t s) {
  const uint64_t v = w > 0 ? s : ref;
  const uint64_t top = ((uint64_t)1 << (w > 0 ? w : (uint64_t)nbits)) - 1;   // 2^0 - 1 = 0; top - 1 wraps to 2^64 - 1 then
  return v == top || (m == 2 && v == top - 1);
}

// the scalar decode of a row with m = 0, 1 or 2: the P present integers into out[0, P), present[i] = 1 for a position
// that has one (n_values flags), *n_present = P.  out holds n_values integers; those behind P are zero.  Returns the
// row's status; not ok: out and present are all zero and P is 0.  m == 0 is decode_row with every position present.
SMM_GRIB_HD int decode_row_mv(const void* x, const Row& r, int m, uint32_t* out, uint8_t* present, uint64_t* n_present) {
  const uint32_t n = r.n_values, ng = r.n_groups;
  *n_present = 0;
  if (m == 0) {
    const int status = decode_row(x, r, out);
    for (uint32_t i = 0; i < n; ++i) present[i] = status == kOk;
    if (status == kOk) *n_present = n;
    return status;
  }
  if (n == 0) return kOk;
  const Sections sec = sections(r);
  const Stream s = stream_of(x, r);
  int status = sec.status;
  if (status == kOk) {
    uint64_t sum_len = 0, sum_bits = 0;
    for (uint32_t g = 0; g < ng && status == kOk; ++g) {
      uint64_t w, len;
      group_of(s, r, sec, g, &w, &len);
      if (w > 32 || len > n) status = kInvalid;
      sum_len += len;
      sum_bits += w * len;
      if (sum_len > n) status = kInvalid;
    }
    if (status == kOk && sum_len != n) status = kInvalid;
    if (status == kOk && sum_bits > sec.bit_end - sec.data_bit) status = kExhausted;
  }
  uint32_t k = 0;   // present values so far
  if (status == kOk) {
    uint64_t h1, h2, gmin;
    descriptors(s, r, &h1, &h2, &gmin);
    uint64_t pos = sec.data_bit, x1 = 0, x2 = 0, high = 0;
    uint32_t i = 0;
    for (uint32_t g = 0; g < ng; ++g) {
      uint64_t w, len;
      group_of(s, r, sec, g, &w, &len);
      const uint64_t ref = group_ref(s, r, sec, g);
      for (uint64_t q = 0; q < len; ++q, ++i, pos += w) {
        const uint64_t stored = s.peek(pos, (int)w);
        present[i] = !is_missing(m, w, r.nbits, ref, stored);
        if (!present[i]) continue;
        const uint64_t z = ref + stored;
        uint64_t X;
        if (r.order <= 0)
          X = z;
        else if (k == 0)
          X = h1;
        else if (r.order == 1)
          X = x1 + z + gmin;
        else if (k == 1)
          X = h2;
        else
          X = 2 * x1 - x2 + z + gmin;
        x2 = x1;
        x1 = X;
        high |= X >> 32;
        out[k++] = (uint32_t)X;
      }
    }
    if (high) status = kInvalid;
  }
  if (status != kOk) {
    for (uint32_t i = 0; i < n; ++i) present[i] = 0;
    k = 0;
  }
  for (uint32_t i = k; i < n; ++i) out[i] = 0;
  *n_present = k;
  return status;
}

// ---- the encoder's small functions: what encode_row below and the kernels of smm_grib_cpx_pack.hip share
// what is wanted of a row: n integers of nbits_in bits, coded at `order` in groups of L values
struct Want {
  uint32_t n_values;
  int32_t nbits_in, order;
  uint32_t L;
};
// rule 1 and the descriptors' size: the effective order (0: g and n_oct are 0)
struct Decision {
  int64_t g;
  int32_t order, n_oct;
};
SMM_GRIB_HD int bit_length(uint64_t v) { return v ? 64 - __builtin_clzll(v) : 0; }
// the smallest n_oct of 1..4 whose sign-magnitude form holds a magnitude <= 2^31 - 1
SMM_GRIB_HD int octets_of(uint64_t mag) { return mag < (1u << 7) ? 1 : mag < (1u << 15) ? 2 : mag < (1u << 23) ? 3 : 4; }
// x0, x1: the row's first two integers (x1 is read at order 2 only); dmin, dmax: the extremes of d_i over i >= order
SMM_GRIB_HD Decision decide(uint32_t n, int order, uint64_t x0, uint64_t x1, int64_t dmin, int64_t dmax) {
  const Decision none{0, 0, 0};
  if (order <= 0 || n <= (uint32_t)order) return none;
  uint64_t top = dmin < 0 ? (uint64_t)0 - (uint64_t)dmin : (uint64_t)dmin;
  if (x0 > top) top = x0;
  if (order > 1 && x1 > top) top = x1;
  if (top > 0x7fffffffull || (uint64_t)(dmax - dmin) > 0xffffffffull) return none;
  return Decision{dmin, order, octets_of(top)};
}
// d_i (i >= order >= 1) of the integers q(0..n)
template <class Q>
SMM_GRIB_HD int64_t difference(Q&& q, uint32_t i, int order) {
  const int64_t a = (int64_t)q(i) - (int64_t)q(i - 1);
  return order == 1 ? a : a - ((int64_t)q(i - 1) - (int64_t)q(i - 2));
}
// z_i under a decision: in [0, 2^32)
template <class Q>
SMM_GRIB_HD uint32_t z_of(Q&& q, uint32_t i, const Decision& dec) {
  if (dec.order <= 0) return q(i);
  return i < (uint32_t)dec.order ? 0u : (uint32_t)(difference(q, i, dec.order) - dec.g);
}
SMM_GRIB_HD uint32_t sign_magnitude_of(int64_t v, int n_oct) {
  return v < 0 ? (1u << (8 * n_oct - 1)) | (uint32_t)(-v) : (uint32_t)v;
}
SMM_GRIB_HD uint32_t groups_of(uint32_t n, uint32_t L) { return (uint32_t)(((uint64_t)n + L - 1) / L); }
// rules 3 and 4 as a record: the stream of n values in groups of L with the three table widths from the extremes of the
// groups' references and widths; byte_off is 0, byte_len the stream's bytes for data_bits bits of group values
SMM_GRIB_HD Row coded_row(uint32_t n, uint32_t L, const Decision& dec, uint32_t ref_max, uint32_t w_min, uint32_t w_max,
                          uint64_t data_bits) {
  Row r{};
  r.n_values = n;
  r.n_groups = groups_of(n, L);
  if (n == 0) return r;
  r.nbits = bit_length(ref_max);
  r.width_ref = w_min;
  r.width_bits = bit_length(w_max - w_min);
  r.length_ref = r.n_groups > 1 ? L : n;
  r.length_inc = 1;
  r.length_last = n - (r.n_groups - 1) * L;
  r.order = dec.order;
  r.n_oct = dec.n_oct;
  const Sections sec = sections(r);
  r.byte_len = (sec.data_bit + data_bits + 7) / 8;
  return r;
}
SMM_GRIB_HD smm_grib_cpx_t record_of(const Row& r) {
  smm_grib_cpx_t c{};
  c.byte_off = r.byte_off, c.byte_len = r.byte_len, c.n_values = r.n_values, c.n_groups = r.n_groups, c.nbits = r.nbits;
  c.width_ref = r.width_ref, c.width_bits = r.width_bits, c.length_ref = r.length_ref, c.length_inc = r.length_inc;
  c.length_last = r.length_last, c.length_bits = r.length_bits, c.order = r.order, c.n_oct = r.n_oct;
  return c;
}
// the record of a row that is not coded (nbits_in == 0): marked simple-packed, no bytes
SMM_GRIB_HD smm_grib_cpx_t simple_record(uint64_t n_values, uint64_t byte_off) {
  smm_grib_cpx_t c{};
  c.byte_off = byte_off, c.n_values = n_values, c.order = SMM_GRIB_CPX_SIMPLE;
  return c;
}
// THE BOUND of a row's stream, rounded up to 4 bytes.  With o the wanted order and w = nbits_in: z = X < 2^w at order 0,
// z = d - g <= max d - min d <= 2 (2^w - 1) at order 1 and <= 4 (2^w - 1) at order 2, and z < 2^32 by rule 1, so every z --
// hence every group reference and every group's max z - ref -- fits in m = min(32, w + o) bits; a fall to order 0 only
// lowers that to w.  A group width is at most 32, so a stored width (w_g - width_ref <= 32) needs at most 6 bits.
//   descriptors (o + 1) * 4 octets at most (none at order 0) | NG references of <= m bits | NG widths of <= 6 bits |
//   no lengths | n values of <= m bits; each part rounded up to an octet.  A row of no values or of width 0 has no bytes.
SMM_GRIB_HD uint64_t pack_bound_bytes(uint64_t n, int nbits_in, int order, uint32_t L) {
  if (n == 0 || nbits_in == 0) return 0;
  const uint64_t m = nbits_in + order < 32 ? (uint64_t)(nbits_in + order) : 32, ng = (n + L - 1) / L;
  const uint64_t head = order > 0 ? (uint64_t)(order + 1) * 4 : 0;
  return smm_grib::align4(head + (ng * m + 7) / 8 + (ng * 6 + 7) / 8 + (n * m + 7) / 8);
}

// n (0..32) bits of v at bit position p of the zeroed bytes out[0, cap); false: they would pass cap
inline bool put_bits(uint8_t* out, uint64_t cap, uint64_t p, uint32_t v, int n) {
  if (n <= 0) return true;
  if ((p + (uint64_t)n + 7) / 8 > cap) return false;
  for (int b = n - 1; b >= 0; --b, ++p)
    if ((v >> b) & 1u) out[p >> 3] |= (uint8_t)(0x80u >> (p & 7));
  return true;
}
// ---- the scalar encode: the integers q(0..n) into the zeroed out[0, cap) by THE RULE OF THIS ENCODER; *rec is the
// record of the stream written (byte_off 0).  Returns its bytes, or UINT64_MAX when they would pass cap.  The row has
// nbits_in >= 1.  Host only: the groups' references and widths are kept in two heap arrays between the passes.
template <class Q>
uint64_t encode_row(Q&& q, const Want& want, uint8_t* out, uint64_t cap, Row* rec) {
  const uint32_t n = want.n_values, L = want.L, ng = groups_of(n, L);
  int64_t dmin = INT64_MAX, dmax = INT64_MIN;
  const int o = n > (uint32_t)want.order ? want.order : 0;
  for (uint32_t i = (uint32_t)o; o > 0 && i < n; ++i) {
    const int64_t d = difference(q, i, o);
    dmin = d < dmin ? d : dmin;
    dmax = d > dmax ? d : dmax;
  }
  const Decision dec = o > 0 ? decide(n, o, q(0), o > 1 ? q(1) : 0, dmin, dmax) : Decision{0, 0, 0};
  uint32_t* refs = new uint32_t[2 * (size_t)ng + 1];
  uint32_t* ws = refs + ng;
  uint32_t ref_max = 0, w_min = 64, w_max = 0;
  uint64_t data_bits = 0;
  for (uint32_t g = 0; g < ng; ++g) {
    const uint32_t i0 = g * L, i1 = n - i0 < L ? n : i0 + L;
    uint32_t lo = 0xffffffffu, hi = 0;
    for (uint32_t i = i0; i < i1; ++i) {
      const uint32_t z = z_of(q, i, dec);
      lo = z < lo ? z : lo;
      hi = z > hi ? z : hi;
    }
    refs[g] = lo;
    ws[g] = (uint32_t)bit_length(hi - lo);
    ref_max = lo > ref_max ? lo : ref_max;
    w_min = ws[g] < w_min ? ws[g] : w_min;
    w_max = ws[g] > w_max ? ws[g] : w_max;
    data_bits += (uint64_t)ws[g] * (i1 - i0);
  }
  *rec = coded_row(n, L, dec, ref_max, w_min, w_max, data_bits);
  const Sections sec = sections(*rec);
  bool ok = rec->byte_len <= cap;
  if (ok && dec.order > 0) {
    const int nb = 8 * dec.n_oct;
    ok = put_bits(out, cap, 0, sign_magnitude_of((int64_t)q(0), dec.n_oct), nb);
    if (dec.order > 1) ok = ok && put_bits(out, cap, (uint64_t)nb, sign_magnitude_of((int64_t)q(1), dec.n_oct), nb);
    ok = ok && put_bits(out, cap, (uint64_t)dec.order * nb, sign_magnitude_of(dec.g, dec.n_oct), nb);
  }
  uint64_t pos = sec.data_bit;
  for (uint32_t g = 0; ok && g < ng; ++g) {
    ok = put_bits(out, cap, sec.refs_bit + (uint64_t)g * (uint64_t)rec->nbits, refs[g], rec->nbits) &&
         put_bits(out, cap, sec.widths_bit + (uint64_t)g * (uint64_t)rec->width_bits, ws[g] - rec->width_ref, rec->width_bits);
    const uint32_t i0 = g * L, i1 = n - i0 < L ? n : i0 + L;
    for (uint32_t i = i0; ok && i < i1; ++i, pos += ws[g]) ok = put_bits(out, cap, pos, z_of(q, i, dec) - refs[g], (int)ws[g]);
  }
  delete[] refs;
  return ok ? rec->byte_len : UINT64_MAX;
}

}  // namespace smm_cpx
