// The pure host pieces of smm_grib_xcode.hpp -- the arena of one scratch allocation and the cutting of a launch at the
// grid limit -- on the host under AddressSanitizer + UBSan.  No HIP: g++ sees only the part of the header above its
// __HIPCC__ guard.  Prints "ok <checks>" and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_grib_xcode.hpp"

namespace {

int checks = 0, failed = 0;
#define CHECK(cond)                                                   \
  do {                                                                \
    ++checks;                                                         \
    if (!(cond)) {                                                    \
      ++failed;                                                       \
      std::printf("line %d: %s does not hold\n", __LINE__, #cond);    \
    }                                                                 \
  } while (0)

struct alignas(8) Rec56 {
  char b[56];
};
struct alignas(32) Wide {
  char b[32];
};

void arena() {
  smm_xcode::Arena a;
  CHECK(a.bytes() == 0);
  struct Member {
    size_t off, bytes, align;
  };
  std::vector<Member> m;
  m.push_back({a.add<Rec56>(3), 3 * sizeof(Rec56), alignof(Rec56)});
  m.push_back({a.add<int32_t>(5), 5 * sizeof(int32_t), alignof(int32_t)});
  m.push_back({a.add<uint64_t>(0), 0, alignof(uint64_t)});   // an empty member takes no bytes
  m.push_back({a.add<char>(1), 1, alignof(char)});
  m.push_back({a.add<uint64_t>(7), 7 * sizeof(uint64_t), alignof(uint64_t)});
  m.push_back({a.add<Wide>(2), 2 * sizeof(Wide), alignof(Wide)});
  m.push_back({a.add<uint32_t>(9), 9 * sizeof(uint32_t), alignof(uint32_t)});
  CHECK(m[0].off == 0);
  size_t end = 0;
  for (const Member& x : m) {
    CHECK(x.off % x.align == 0);
    CHECK(x.off >= end);          // in order, no overlap
    CHECK(x.off - end < 32);      // and no more than the padding between them
    end = x.off + x.bytes;
  }
  CHECK(a.bytes() == end);
  CHECK(m[3].off == m[2].off);    // the member behind the empty one begins where it does
  // every member can be written through its typed pointer without touching its neighbours or the allocation's end
  // (ASan watches the end of the vector of bytes() bytes; operator new aligns it to 16, which these types need)
  std::vector<char> mem(a.bytes(), 0);
  uint64_t* u = smm_xcode::Arena::at<uint64_t>(mem.data(), m[4].off);
  for (int i = 0; i < 7; ++i) u[i] = ~0ull;
  std::memset(mem.data() + m[5].off, 0, m[5].bytes);
  uint32_t* w = smm_xcode::Arena::at<uint32_t>(mem.data(), m[6].off);
  for (int i = 0; i < 9; ++i) w[i] = 0u;
  CHECK(u[6] == ~0ull && (char*)(w + 9) == mem.data() + a.bytes());
}

// pieces cover [0, total) once, in order, each of 1..min(limit, 2^31 - 1) workgroups
void cut(int64_t total, int64_t limit, int64_t want_pieces) {
  const int64_t cap = limit < 1 ? 1 : limit > 0x7fffffffLL ? 0x7fffffffLL : limit;
  int64_t next = 0, pieces = 0;
  bool ok = true;
  const int rc = smm_xcode::cut_grid(total, limit, [&](int64_t b0, unsigned nb) {
    ok = ok && b0 == next && nb >= 1 && (int64_t)nb <= cap && (b0 + nb == total || (int64_t)nb == cap);
    next = b0 + nb;
    ++pieces;
    return 0;
  });
  CHECK(rc == 0);
  CHECK(ok);
  CHECK(next == (total > 0 ? total : 0));
  CHECK(pieces == want_pieces);
}

void cutter() {
  cut(0, 100, 0);
  cut(-5, 100, 0);
  cut(100, 100, 1);
  cut(101, 100, 2);
  cut(1, 100, 1);
  cut(37, 1, 37);
  cut(37, 0, 37);                      // a limit below 1 counts as 1
  cut(37, -9, 37);
  cut(280, 17, 17);
  cut(280, 7, 40);
  const int64_t big = (1ll << 32) + 12345;       // above 2^32: three launches of at most 2^31 - 1
  cut(big, 0x7fffffffLL, 3);
  cut(big, INT64_MAX, 3);              // a limit above 2^31 - 1 counts as 2^31 - 1
  cut(big, 1ll << 20, (big + (1ll << 20) - 1) >> 20);
  // the first failure ends the cutting and is returned
  int calls = 0;
  const int rc = smm_xcode::cut_grid(1000, 10, [&](int64_t, unsigned) { return ++calls == 3 ? 42 : 0; });
  CHECK(rc == 42 && calls == 3);
}

}  // namespace

int main() {
  arena();
  cutter();
  if (failed) return std::printf("%d of %d checks failed\n", failed, checks), 1;
  std::printf("ok %d\n", checks);
  return 0;
}
