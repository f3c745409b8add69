// GRIB-2 complex packing (data representation template 5.2) and complex packing with spatial differencing (5.3), what
// NCEP's g2c / wgrib2 write for GFS, GEFS, HRRR: the decoder, stated once.  Plain C++ that compiles for host and device
// -- the host decode (smm_grib_cpx_decode_host), the kernels of smm_grib_cpx_unpack (smm_grib_cpx.hip) and
// tests/cpp/grib_cpx_harness.cpp all read the stream through Stream::peek (smm_grib_aec.hpp's load_word / bits_of) and
// take the tables apart with the small functions below.
//
// THE FORMAT.  Octets are WMO's (FM 92 GRIB edition 2), as recalled: no file written by g2c, wgrib2 or ecCodes was at
// hand to pin them.
//   section 5, template 5.2 (47 octets)
//     12-15 R (IEEE f32)   16-17 E   18-19 D (sign-magnitude)   20 nbits, the width of the group references
//     21 type of original values   22 group splitting method   23 missing value management (only 0 is decoded)
//     24-27, 28-31 missing value substitutes   32-35 NG, the number of groups   36 reference for group widths
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
// A ROW ENDS AS (first that applies)
//   kInvalid    NG > n_values -- a group of no values is no group; it bounds the scratch by the record
//   kExhausted  the descriptors and the three tables do not fit into byte_len
//   kInvalid    some w_g > 32, or some L_g > n_values, or the lengths do not sum to n_values
//   kExhausted  the groups' bits leave the stream
//   kInvalid    some X_i outside [0, 2^32)
// and its integers are then zero.  TWO RULES bound every loop and every read: (1) every loop runs over NG or n_values of
// the record; (2) no load goes past the 32-bit word that holds the stream's last byte (load_word clamps; a stream of no
// bytes is never loaded from).  A malformed stream costs wrong numbers and a status, never a read outside the buffer.
#pragma once

#include <cstdint>

#include "smm_grib_aec.hpp"

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
    return smm_aec::bits_of(smm_aec::load_word(x, w, last_word, end_byte), smm_aec::load_word(x, w + 1, last_word, end_byte),
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

}  // namespace smm_cpx
