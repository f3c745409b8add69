// The CCSDS decoder of smm_grib_aec.hpp on the host under AddressSanitizer + UBSan, on streams that are not what an
// encoder wrote: every fixture truncated at every byte, and with single bytes corrupted.  The stream always sits in a heap
// block of exactly its bytes (at offset 0 and at the odd offset 3), so a read past its end is a sanitizer report; every
// run must end with one of the three statuses, and a run that ends ok on a truncated stream must still give the
// fixture's integers (only pad bits were cut).  A case may be malformed as it stands (the forced streams of
// tests/ccsds_forced_cases.py, group G): its whole stream must then end with the status the case names and leave the
// values the case holds -- the samples up to the failing block, zeros from there on.  tests/test_grib_ccsds.py writes
// the case file and runs this program.
//
// case file: int64 n_cases, then per case  int64 {n_values, nbits, block, rsi, preprocess, stream bytes, the status of
// the whole stream}, the stream, the expected uint32 values.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_aec.hpp"

static int fail(const char* what, long c, long at) {
  fprintf(stderr, "grib_aec_harness: case %ld, at %ld: %s\n", c, at, what);
  return 1;
}

// decodes `len` bytes of `bytes` from a heap block of exactly off + len bytes
static int decode_exact(const smm_aec::Row& proto, const uint8_t* bytes, size_t len, size_t off, std::vector<uint32_t>& out) {
  uint8_t* block = new uint8_t[off + len + (off + len == 0)];
  memset(block, 0xEE, off);
  if (len) memcpy(block + off, bytes, len);
  smm_aec::Row r = proto;
  r.byte_off = off;
  r.byte_len = len;
  const int status = smm_aec::decode_row(block, r, out.data(), nullptr);
  delete[] block;
  return status;
}

int main(int argc, char** argv) {
  if (argc != 2) return fail("usage: grib_aec_harness <cases>", -1, 0);
  FILE* f = fopen(argv[1], "rb");
  if (!f) return fail("cannot open the case file", -1, 0);
  int64_t n_cases = 0;
  if (fread(&n_cases, 8, 1, f) != 1) return fail("short case file", -1, 0);
  for (int64_t c = 0; c < n_cases; ++c) {
    int64_t h[7];
    if (fread(h, 8, 7, f) != 7) return fail("short case header", c, 0);
    const int expect = (int)h[6];
    std::vector<uint8_t> stream((size_t)h[5]);
    std::vector<uint32_t> want((size_t)h[0]), got((size_t)h[0] + 1);
    if (fread(stream.data(), 1, stream.size(), f) != stream.size()) return fail("short stream", c, 0);
    if (fread(want.data(), 4, want.size(), f) != want.size()) return fail("short values", c, 0);
    const smm_aec::Row row{0, 0, (uint32_t)h[0], (int)h[1], (int)h[2], (int)h[3], h[4] != 0};
    const uint32_t guard = 0xFEEDFACEu;
    long counts[3] = {0, 0, 0}, runs = 0;
    auto run = [&](const uint8_t* bytes, size_t len, size_t off, bool must_match_if_ok, long at) -> int {
      got[want.size()] = guard;
      const int st = decode_exact(row, bytes, len, off, got);
      ++runs;
      if (st < 0 || st > 2) return fail("a status outside ok / exhausted / invalid", c, at);
      if (got[want.size()] != guard) return fail("a store past n_values", c, at);
      ++counts[st];
      if (st == smm_aec::kOk && must_match_if_ok && memcmp(got.data(), want.data(), want.size() * 4) != 0)
        return fail("ended ok with other integers", c, at);
      return 0;
    };
    // whole, at both offsets: the status expected (ok for a fixture) and the values expected
    for (size_t off : {(size_t)0, (size_t)3}) {
      if (run(stream.data(), stream.size(), off, true, -1)) return 1;
      if (counts[expect] != runs) return fail("the whole stream does not end with the status expected", c, (long)off);
      if (memcmp(got.data(), want.data(), want.size() * 4) != 0) return fail("the whole stream leaves other integers", c, (long)off);
    }
    // truncated at every byte
    for (size_t len = 0; len < stream.size(); ++len)
      if (run(stream.data(), len, len & 1 ? 3 : 0, expect == smm_aec::kOk, (long)len)) return 1;
    // single bytes corrupted: every byte of a short stream, some 500 spread over a long one
    const size_t step = stream.size() / 500 + 1;
    std::vector<uint8_t> bad(stream);
    for (size_t at = 0; at < stream.size(); at += step)
      for (uint8_t flip : {(uint8_t)0xFF, (uint8_t)0x01, (uint8_t)0x80}) {
        bad[at] = stream[at] ^ flip;
        if (run(bad.data(), bad.size(), at & 1 ? 3 : 0, false, (long)at)) return 1;
        bad[at] = stream[at];
      }
    printf("case %ld runs %ld ok %ld exhausted %ld invalid %ld\n", (long)c, runs, counts[0], counts[1], counts[2]);
  }
  fclose(f);
  return 0;
}
