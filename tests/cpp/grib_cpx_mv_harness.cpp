// The complex-packing decoder for rows with missing values inside their groups (decode_row_mv of smm_grib_cpx.hpp) on the
// host under AddressSanitizer + UBSan.  The stream sits in a heap block of exactly its bytes (at offset 0 and at the odd
// offset 3), the integers and the flags in blocks of exactly n_values entries, so a read or a write past an end is a
// sanitizer report.  Per case: the stream as it is (it must give the case's integers, flags and count); truncated at
// every byte; single bytes inverted (every 7th beyond 1024 bytes).  Every run must end with one of the three statuses;
// one that does not end ok leaves zeros and a count of 0, one that ends ok a count that is the number of set flags.
//
// case file: int64 n_cases, then per case  int64 {n_values, n_groups, nbits, width_ref, width_bits, length_ref, length_inc,
// length_last, length_bits, order, n_oct, stream bytes, m, P}, the stream, P uint32 integers, n_values flags.
//
// grib_cpx_mv_harness <cases> pinned: rows with the status they must end with (tests/complex_seam_cases.py), malformed
// ones among them.  The header has one more int64, that status; a row that is not ok has P = 0 and flags of zero.  Each
// row is decoded once at each of the offsets 0..3: status, count, integers (zero behind P) and flags must be the file's.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_cpx.hpp"

static int fail(const char* what, long c, long at) {
  fprintf(stderr, "grib_cpx_mv_harness: case %ld, at %ld: %s\n", c, at, what);
  return 1;
}

struct Run {
  int status;
  uint64_t count;
};

// decodes `len` bytes of `bytes` from a heap block of exactly off + len bytes into exact blocks of n entries
static Run decode_exact(const smm_cpx::Row& proto, int m, const uint8_t* bytes, size_t len, size_t off, std::vector<uint32_t>& out,
                        std::vector<uint8_t>& flags) {
  const size_t n = proto.n_values;
  uint8_t* block = new uint8_t[off + len + (off + len == 0)];
  uint32_t* values = new uint32_t[n + (n == 0)];
  uint8_t* present = new uint8_t[n + (n == 0)];
  memset(block, 0xEE, off);
  if (len) memcpy(block + off, bytes, len);
  smm_cpx::Row r = proto;
  r.byte_off = off;
  r.byte_len = len;
  Run got{0, 0};
  got.status = smm_cpx::decode_row_mv(block, r, m, values, present, &got.count);
  out.assign(values, values + n);
  flags.assign(present, present + n);
  delete[] block;
  delete[] values;
  delete[] present;
  return got;
}

static int pinned(FILE* f, int64_t n_cases) {
  long count[3] = {0, 0, 0};
  for (int64_t c = 0; c < n_cases; ++c) {
    int64_t h[15];
    if (fread(h, 8, 15, f) != 15) return fail("short case header", c, 0);
    const size_t n = (size_t)h[0], len = (size_t)h[11], P = (size_t)h[13];
    const int m = (int)h[12], want_status = (int)h[14];
    std::vector<uint8_t> stream(len + 1), want_flags(n + 1), flags;
    std::vector<uint32_t> want(P + 1), got;
    if (len && fread(stream.data(), 1, len, f) != len) return fail("short stream", c, 0);
    if (P && fread(want.data(), 4, P, f) != P) return fail("short values", c, 0);
    if (n && fread(want_flags.data(), 1, n, f) != n) return fail("short flags", c, 0);
    if (want_status < 0 || want_status > 2 || P > n) return fail("no such status or count", c, want_status);
    smm_cpx::Row proto{0,           0,           (uint32_t)h[0], (uint32_t)h[1], (int32_t)h[2],  (uint32_t)h[3], (int32_t)h[4],
                       (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
    for (size_t off = 0; off < 4; ++off) {
      const Run r = decode_exact(proto, m, stream.data(), len, off, got, flags);
      if (r.status != want_status) return fail("the row ends with another status", c, r.status);
      if (r.count != P) return fail("the row's count differs", c, (long)r.count);
      if (P && memcmp(got.data(), want.data(), 4 * P) != 0) return fail("the row's integers differ", c, (long)off);
      for (size_t i = P; i < n; ++i)
        if (got[i]) return fail("an integer behind the count is not zero", c, (long)i);
      for (size_t i = 0; i < n; ++i)
        if ((flags[i] != 0) != (want_flags[i] != 0)) return fail("the row's flags differ", c, (long)i);
    }
    ++count[want_status];
  }
  printf("pinned %ld ok %ld exhausted %ld invalid %ld\n", (long)n_cases, count[0], count[1], count[2]);
  return 0;
}

int main(int argc, char** argv) {
  const bool pin = argc == 3 && strcmp(argv[2], "pinned") == 0;
  if (argc != 2 && !pin) return fail("usage: grib_cpx_mv_harness <cases> [pinned]", -1, 0);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fail("cannot open the case file", -1, 0);
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return fail("short case file", -1, 0);
  if (pin) {
    const int rc = pinned(f, n_cases);
    fclose(f);
    return rc;
  }
  for (int64_t c = 0; c < n_cases; ++c) {
    int64_t h[14];
    if (fread(h, 8, 14, f) != 14) return fail("short case header", c, 0);
    const size_t n = (size_t)h[0], len = (size_t)h[11], P = (size_t)h[13];
    const int m = (int)h[12];
    std::vector<uint8_t> stream(len + 1), want_flags(n + 1), flags;
    std::vector<uint32_t> want(P + 1), got;
    if (len && fread(stream.data(), 1, len, f) != len) return fail("short stream", c, 0);
    if (P && fread(want.data(), 4, P, f) != P) return fail("short values", c, 0);
    if (n && fread(want_flags.data(), 1, n, f) != n) return fail("short flags", c, 0);
    smm_cpx::Row proto{0,           0,           (uint32_t)h[0], (uint32_t)h[1], (int32_t)h[2],  (uint32_t)h[3], (int32_t)h[4],
                       (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
    long runs = 0, count[3] = {0, 0, 0};
    auto run = [&](const uint8_t* bytes, size_t l, size_t off, bool intact) -> int {
      const Run r = decode_exact(proto, m, bytes, l, off, got, flags);
      if (r.status < 0 || r.status > 2) return -1;
      size_t set = 0;
      for (size_t i = 0; i < n; ++i) set += flags[i] != 0;
      if (set != r.count || r.count > n) return -2;
      for (size_t i = r.count; i < n; ++i)
        if (got[i]) return -3;
      if (r.status != smm_cpx::kOk && r.count != 0) return -4;
      if (intact && (r.status != smm_cpx::kOk || r.count != P || memcmp(got.data(), want.data(), 4 * P) != 0 ||
                     memcmp(flags.data(), want_flags.data(), n) != 0))
        return -5;
      ++runs;
      ++count[r.status];
      return r.status;
    };
    for (size_t off : {(size_t)0, (size_t)3})
      if (run(stream.data(), len, off, true) < 0) return fail("the intact stream does not decode to its integers and flags", c, (long)off);
    const size_t step = len > 1024 ? 7 : 1;
    for (size_t cut = 0; cut < len; ++cut)
      if (run(stream.data(), cut, cut & 3, false) < 0) return fail("a truncated stream broke the contract", c, (long)cut);
    for (size_t at = 0; at < len; at += step) {
      stream[at] ^= 0xFF;
      const int st = run(stream.data(), len, 0, false);
      stream[at] ^= 0xFF;
      if (st < 0) return fail("an inverted byte broke the contract", c, (long)at);
    }
    printf("case %ld runs %ld ok %ld exhausted %ld invalid %ld\n", (long)c, runs, count[0], count[1], count[2]);
  }
  fclose(f);
  return 0;
}
