// The complex-packing decoder of smm_grib_cpx.hpp on the host under AddressSanitizer + UBSan, on input that is not what
// an encoder wrote.  The stream always sits in a heap block of exactly its bytes (at offset 0 and at the odd offset 3), so
// a read past its end is a sanitizer report; every run must end with one of the three statuses, a run that ends ok on a
// truncated stream must still give the case's integers (only pad bits were cut), and a run that does not end ok leaves
// zeros.  Per case: the stream as it is; truncated at every byte; single bytes inverted (every 7th beyond 1024 bytes);
// and five named faults whose status tests/test_grib_complex.py checks -- the last length one more and one less (the
// lengths no longer sum to n_values), a group width of 33, every group one bit wider (their bits pass the stream's end),
// the sign bit set on h_1.  Then seeded random records over random byte strings.
//
// case file: int64 n_cases, then per case  int64 {n_values, n_groups, nbits, width_ref, width_bits, length_ref, length_inc,
// length_last, length_bits, order, n_oct, stream bytes}, the stream, the expected uint32 values.
//
// grib_cpx_harness <cases> pinned: rows with the status they must end with (tests/complex_seam_cases.py), malformed ones
// among them.  The header has one more int64, that status; the values are n_values zeros when it is not ok.  Each row
// is decoded once at each of the offsets 0..3, from a block of exactly its bytes: status and integers must be the
// file's.  No truncation, no inversion -- the rows may be long.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_cpx.hpp"

static int fail(const char* what, long c, long at) {
  fprintf(stderr, "grib_cpx_harness: case %ld, at %ld: %s\n", c, at, what);
  return 1;
}

// decodes `len` bytes of `bytes` from a heap block of exactly off + len bytes
static int decode_exact(const smm_cpx::Row& proto, const uint8_t* bytes, size_t len, size_t off, std::vector<uint32_t>& out) {
  uint8_t* block = new uint8_t[off + len + (off + len == 0)];
  memset(block, 0xEE, off);
  if (len) memcpy(block + off, bytes, len);
  smm_cpx::Row r = proto;
  r.byte_off = off;
  r.byte_len = len;
  const int status = smm_cpx::decode_row(block, r, out.data());
  delete[] block;
  return status;
}

static bool all_zero(const std::vector<uint32_t>& v, size_t n) {
  for (size_t i = 0; i < n; ++i)
    if (v[i]) return false;
  return true;
}

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() {   // xorshift64*
  rng_state ^= rng_state >> 12;
  rng_state ^= rng_state << 25;
  rng_state ^= rng_state >> 27;
  return rng_state * 0x2545F4914F6CDD1Dull;
}

static int pinned(FILE* f, int64_t n_cases) {
  long count[3] = {0, 0, 0};
  for (int64_t c = 0; c < n_cases; ++c) {
    int64_t h[13];
    if (fread(h, 8, 13, f) != 13) return fail("short case header", c, 0);
    const size_t n = (size_t)h[0], len = (size_t)h[11];
    const int want_status = (int)h[12];
    std::vector<uint8_t> stream(len + 1);
    std::vector<uint32_t> want(n + 1), got(n + 1);
    if (len && fread(stream.data(), 1, len, f) != len) return fail("short stream", c, 0);
    if (n && fread(want.data(), 4, n, f) != n) return fail("short values", c, 0);
    if (want_status < 0 || want_status > 2) return fail("no such status", c, want_status);
    smm_cpx::Row proto{0,           0,           (uint32_t)h[0], (uint32_t)h[1], (int32_t)h[2],  (uint32_t)h[3], (int32_t)h[4],
                       (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
    for (size_t off = 0; off < 4; ++off) {
      got.assign(n + 1, 0xDEADBEEFu);
      const int st = decode_exact(proto, stream.data(), len, off, got);
      if (st != want_status) return fail("the row ends with another status", c, st);
      if (n && memcmp(got.data(), want.data(), 4 * n) != 0) return fail("the row's integers differ", c, (long)off);
    }
    ++count[want_status];
  }
  printf("pinned %ld ok %ld exhausted %ld invalid %ld\n", (long)n_cases, count[0], count[1], count[2]);
  return 0;
}

int main(int argc, char** argv) {
  const bool pin = argc == 3 && strcmp(argv[2], "pinned") == 0;
  if (argc != 2 && !pin) return fail("usage: grib_cpx_harness <cases> [pinned]", -1, 0);
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
    int64_t h[12];
    if (fread(h, 8, 12, f) != 12) return fail("short case header", c, 0);
    const size_t n = (size_t)h[0], len = (size_t)h[11];
    std::vector<uint8_t> stream(len + 1);
    std::vector<uint32_t> want(n + 1), got(n + 1);
    if (len && fread(stream.data(), 1, len, f) != len) return fail("short stream", c, 0);
    if (n && fread(want.data(), 4, n, f) != n) return fail("short values", c, 0);
    smm_cpx::Row proto{0,           0,           (uint32_t)h[0], (uint32_t)h[1], (int32_t)h[2],  (uint32_t)h[3], (int32_t)h[4],
                       (uint32_t)h[5], (uint32_t)h[6], (uint32_t)h[7], (int32_t)h[8], (int32_t)h[9], (int32_t)h[10]};
    long runs = 0, count[3] = {0, 0, 0};
    auto run = [&](const smm_cpx::Row& r, const uint8_t* bytes, size_t l, size_t off, bool same_when_ok) -> int {
      const int st = decode_exact(r, bytes, l, off, got);
      if (st < 0 || st > 2) return -1;
      if (st != smm_cpx::kOk && !all_zero(got, n)) return -2;
      if (st == smm_cpx::kOk && same_when_ok && memcmp(got.data(), want.data(), 4 * n) != 0) return -3;
      ++runs;
      ++count[st];
      return st;
    };
    for (size_t off : {(size_t)0, (size_t)3})
      if (run(proto, stream.data(), len, off, true) != smm_cpx::kOk) return fail("the intact stream does not decode to its integers", c, (long)off);
    const size_t step = len > 1024 ? 7 : 1;
    for (size_t cut = 0; cut < len; ++cut)
      if (run(proto, stream.data(), cut, cut & 1 ? 3 : 0, true) < 0) return fail("a truncated stream", c, (long)cut);
    for (size_t at = 0; at < len; at += step) {
      stream[at] ^= 0xFF;
      const int st = run(proto, stream.data(), len, 3, false);
      stream[at] ^= 0xFF;
      if (st < 0) return fail("a corrupted stream", c, (long)at);
    }
    // the named faults
    int named[5];
    smm_cpx::Row r = proto;
    r.length_last = proto.length_last + 1;
    named[0] = run(r, stream.data(), len, 0, false);
    r.length_last = proto.length_last - 1;
    named[1] = run(r, stream.data(), len, 3, false);
    r = proto;
    r.width_ref = 33;
    named[2] = run(r, stream.data(), len, 0, false);
    r = proto;
    r.width_ref = proto.width_ref + 1;
    named[3] = run(r, stream.data(), len, 3, false);
    named[4] = 9;   // not applicable: no h_1, or h_1 == 0 (minus zero is zero)
    if (proto.order > 0 && len > 0) {
      bool nonzero = false;
      for (int k = 0; k < proto.n_oct; ++k) nonzero = nonzero || (stream[k] & (k ? 0xFF : 0x7F));
      if (nonzero) {
        stream[0] |= 0x80;
        named[4] = run(proto, stream.data(), len, 0, false);
        stream[0] = (uint8_t)(stream[0] & 0x7F);   // (no case's h_1 is negative)
      }
    }
    for (int k = 0; k < 5; ++k)
      if (named[k] < 0) return fail("a named fault", c, k);
    printf("case %ld runs %ld ok %ld exhausted %ld invalid %ld named %d %d %d %d %d\n", (long)c, runs, count[0], count[1], count[2],
           named[0], named[1], named[2], named[3], named[4]);
  }
  fclose(f);
  // random records over random bytes: whatever they say, a status and no read outside the block
  long count[3] = {0, 0, 0};
  std::vector<uint32_t> out(600);
  std::vector<uint8_t> bytes(256);
  for (int it = 0; it < 6000; ++it) {
    const size_t len = rnd() % 200;
    for (size_t k = 0; k < len; ++k) bytes[k] = (uint8_t)rnd();
    const int order = (int)(rnd() % 3);
    const uint32_t n = (uint32_t)order + 1 + (uint32_t)(rnd() % 500);
    const bool small = it & 1;   // small tables: rows that get past the table checks more often
    smm_cpx::Row r{0, 0, n, 1 + (uint32_t)(rnd() % (small ? 4 : 600)), (int32_t)(rnd() % (small ? 5 : 33)), (uint32_t)(rnd() % (small ? 6 : 256)),
                   (int32_t)(rnd() % (small ? 3 : 33)), (uint32_t)(rnd() % (small ? n : 1000)), (uint32_t)(rnd() % (small ? 3 : 256)),
                   (uint32_t)(rnd() % (n + 2)), (int32_t)(rnd() % (small ? 3 : 33)), order, 1 + (int32_t)(rnd() % 4)};
    const int st = decode_exact(r, bytes.data(), len, it % 4, out);
    if (st < 0 || st > 2) return fail("a random record", -1, it);
    if (st != smm_cpx::kOk && !all_zero(out, n)) return fail("a failed random record left numbers", -1, it);
    ++count[st];
  }
  printf("random runs 6000 ok %ld exhausted %ld invalid %ld\n", count[0], count[1], count[2]);
  return 0;
}
