// Host-only harness around csrc/smm_devmem.hpp, compiled with g++ -fsanitize=address,undefined by
// tests/test_devmem_sanitized.py and NOT linked against the HIP runtime: the seven HIP functions the header uses are
// malloc-backed stand-ins defined here.  They count the live blocks, refuse to free a block twice, and fail the k-th
// call on request (a failed hipFree / hipHostFree still gives its block back: the owners ignore that status).
// The sequences mirror how smm_device.hip uses the buffers: ensure_sb (four uploads into locals, then the moves),
// smm_operator_set_epilogue (upload two, swap, refresh the descriptor, swap back on failure) and HostPipe::ensure
// (grow a pair).  Each runs once clean to count its HIP calls N, then once per k = 1..N with call k failing: a failed
// run must leave the "handle" exactly as it was, nothing may leak, and the sticky error must be cleared.
// stdout: one line per sequence with its call count, then "DEVMEMBAD <violations>".
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

#include "../../smmregrid_amd/csrc/smm_devmem.hpp"

namespace {
std::set<void*> g_dev, g_host;   // live blocks
long g_calls = 0, g_fail_at = 0, g_bad = 0;
hipError_t g_sticky = hipSuccess;

#define CHECK(cond)                                              \
  do {                                                           \
    if (!(cond)) {                                               \
      ++g_bad;                                                   \
      printf("line %d: %s (k = %ld)\n", __LINE__, #cond, g_fail_at); \
    }                                                            \
  } while (0)

bool failing() { return ++g_calls == g_fail_at; }
hipError_t fake_alloc(std::set<void*>& live, void** ptr, size_t size) {
  if (failing()) return g_sticky = hipErrorOutOfMemory;
  CHECK(size > 0);
  *ptr = malloc(size);
  live.insert(*ptr);
  return hipSuccess;
}
hipError_t fake_free(std::set<void*>& live, void* ptr) {
  const bool fails = failing();
  if (!ptr) return hipSuccess;
  if (!live.erase(ptr)) {   // freed twice, or never allocated
    CHECK(!"free of a block that is not live");
    return hipErrorInvalidValue;
  }
  free(ptr);
  return fails ? hipErrorInvalidValue : hipSuccess;
}
}  // namespace

extern "C" {
hipError_t hipMalloc(void** ptr, size_t size) { return fake_alloc(g_dev, ptr, size); }
hipError_t hipHostMalloc(void** ptr, size_t size, unsigned int) { return fake_alloc(g_host, ptr, size); }
hipError_t hipFree(void* ptr) { return fake_free(g_dev, ptr); }
hipError_t hipHostFree(void* ptr) { return fake_free(g_host, ptr); }
hipError_t hipMemcpy(void* dst, const void* src, size_t bytes, hipMemcpyKind) {
  if (failing()) return g_sticky = hipErrorInvalidValue;
  memcpy(dst, src, bytes);
  return hipSuccess;
}
hipError_t hipGetLastError(void) {
  const hipError_t e = g_sticky;
  g_sticky = hipSuccess;
  return e;
}
const char* hipGetErrorString(hipError_t e) { return e == hipSuccess ? "no error" : "stand-in error"; }
}

namespace {
using smm::DeviceBuf;
using smm::PinnedBuf;

size_t live() { return g_dev.size() + g_host.size(); }

// run(k) performs the sequence with HIP call k failing (0: none) and checks what it left behind.  Returns the number
// of HIP calls of the clean run after having failed each of them in turn.
template <typename Run>
long every_failure(const char* name, Run&& run) {
  g_calls = g_fail_at = 0;
  run();
  const long n = g_calls;
  for (long k = 1; k <= n; ++k) {
    g_calls = 0;
    g_fail_at = k;
    run();
    CHECK(g_calls >= k);              // call k was reached
    CHECK(g_sticky == hipSuccess);    // ... and its sticky error cleared where it failed
    CHECK(live() == 0);
  }
  g_fail_at = 0;
  CHECK(live() == 0);
  printf("SEQ %s %ld\n", name, n);
  return n;
}

template <typename B>
bool empty(const B& b) { return b.get() == nullptr && b.bytes() == 0; }

// ---- one buffer: alloc, upload, moves, reset
void basics() {
  const std::vector<double> v{1.5, -2.0, 3.25}, none;
  every_failure("device_basics", [&] {
    DeviceBuf<double> a;
    CHECK(empty(a));
    if (a.alloc(5) != hipSuccess) {
      CHECK(empty(a));
      return;
    }
    CHECK(a.get() && a.bytes() == 40 && live() == 1);
    if (a.upload(v) != hipSuccess) {   // frees the 5 elements first; empty after a failed allocation or copy
      CHECK(empty(a) && live() == 0);
      return;
    }
    CHECK(a.bytes() == 24 && live() == 1 && memcmp(a.get(), v.data(), 24) == 0);
    double* const p = a.get();
    DeviceBuf<double> b(std::move(a));                     // move construction: the block changes owner
    CHECK(empty(a) && b.get() == p && b.bytes() == 24 && live() == 1);
    DeviceBuf<double> c;
    if (c.upload(none) != hipSuccess) {                    // empty vector: one element allocated, nothing copied
      CHECK(empty(c) && live() == 1);
      return;
    }
    CHECK(c.get() && c.bytes() == 8 && live() == 2);
    c = std::move(b);                                      // move assignment onto a full buffer frees its block
    CHECK(empty(b) && c.get() == p && c.bytes() == 24 && live() == 1);
    DeviceBuf<double>& same = c;
    c = std::move(same);                                   // onto itself: nothing happens
    CHECK(c.get() == p && c.bytes() == 24 && live() == 1);
    c.reset();
    CHECK(empty(c) && live() == 0);
    c.reset();                                             // twice is harmless
  });
  every_failure("pinned_basics", [&] {
    PinnedBuf a;
    CHECK(empty(a));
    if (a.alloc(64) != hipSuccess) {
      CHECK(empty(a));
      return;
    }
    CHECK(a.get() && a.bytes() == 64 && g_host.size() == 1 && g_dev.empty());
    void* const p = a.get();
    memset(p, 7, 64);
    PinnedBuf b(std::move(a));
    CHECK(empty(a) && b.get() == p && b.bytes() == 64 && live() == 1);
    PinnedBuf c;
    if (c.alloc(16) != hipSuccess) {
      CHECK(empty(c) && live() == 1);
      return;
    }
    c = std::move(b);
    CHECK(empty(b) && c.get() == p && c.bytes() == 64 && live() == 1);
    if (c.alloc(128) != hipSuccess) {                      // grow: free, then allocate; empty after a failure
      CHECK(empty(c) && live() == 0);
      return;
    }
    CHECK(c.bytes() == 128 && live() == 1);
    c.reset();
    CHECK(empty(c) && live() == 0);
  });
}

// ---- ensure_sb: four uploads into locals, moved into the handle only when all four succeeded
struct SbHandle {
  DeviceBuf<long> rowptr;
  DeviceBuf<int> col, colp;
  DeviceBuf<double> val;
  bool ready = false;
};
hipError_t ensure_sb(SbHandle& h, const std::vector<long>& rowptr, const std::vector<int>& col,
                     const std::vector<int>& colp, const std::vector<double>& val) {
  DeviceBuf<long> d_rowptr;
  DeviceBuf<int> d_col, d_colp;
  DeviceBuf<double> d_val;
  hipError_t e;
  if ((e = d_rowptr.upload(rowptr)) != hipSuccess || (e = d_col.upload(col)) != hipSuccess ||
      (e = d_colp.upload(colp)) != hipSuccess || (e = d_val.upload(val)) != hipSuccess)
    return e;
  h.rowptr = std::move(d_rowptr);
  h.col = std::move(d_col);
  h.colp = std::move(d_colp);
  h.val = std::move(d_val);
  h.ready = true;
  return hipSuccess;
}
void sb_sequence() {
  for (int with_links = 0; with_links < 2; ++with_links) {   // an operator without links uploads empty col / val
    const std::vector<long> rowptr = with_links ? std::vector<long>{0, 2, 2, 3} : std::vector<long>{0, 0};
    const std::vector<int> col = with_links ? std::vector<int>{4, 9, 1} : std::vector<int>{};
    const std::vector<int> colp = with_links ? std::vector<int>{1, 2, 0} : std::vector<int>{};
    const std::vector<double> val = with_links ? std::vector<double>{0.25, 0.75, 1.0} : std::vector<double>{};
    const long n = every_failure(with_links ? "ensure_sb" : "ensure_sb_empty", [&] {
      SbHandle h;
      const hipError_t e = ensure_sb(h, rowptr, col, colp, val);
      if (e != hipSuccess) {   // the handle holds none of the four, and the locals are gone
        CHECK(empty(h.rowptr) && empty(h.col) && empty(h.colp) && empty(h.val) && !h.ready && live() == 0);
        return;
      }
      CHECK(h.ready && live() == 4 && h.rowptr.bytes() == rowptr.size() * sizeof(long));
      CHECK(memcmp(h.rowptr.get(), rowptr.data(), h.rowptr.bytes()) == 0);
      CHECK(h.col.bytes() == (with_links ? 12u : 4u) && h.colp.get() && h.val.bytes() == (with_links ? 24u : 8u));
      if (with_links) CHECK(memcmp(h.val.get(), val.data(), 24) == 0 && memcmp(h.colp.get(), colp.data(), 12) == 0);
    });
    CHECK(n == (with_links ? 12 : 9));   // 4 x (hipMalloc + hipMemcpy, none for an empty vector) + 4 x hipFree
  }
}

// ---- set_epilogue: upload two, swap into the handle, refresh the descriptor; on failure swap back
struct Desc {
  const unsigned char* imask;
  const double* frac;
};
struct EpHandle {
  DeviceBuf<unsigned char> imask;
  DeviceBuf<double> frac;
  DeviceBuf<Desc> desc;
};
hipError_t refresh_desc(EpHandle& h) {
  const Desc d{h.imask.get(), h.frac.get()};
  if (!h.desc.get()) {
    const hipError_t e = h.desc.alloc(1);
    if (e != hipSuccess) return e;
  }
  const hipError_t e = hipMemcpy(h.desc.get(), &d, sizeof(Desc), hipMemcpyHostToDevice);
  if (e != hipSuccess) (void)hipGetLastError();   // SMM_HIP
  return e;
}
hipError_t set_epilogue(EpHandle& h, const std::vector<unsigned char>* m, const std::vector<double>* f) {
  DeviceBuf<double> frac;
  DeviceBuf<unsigned char> imask;
  hipError_t e;
  if (m && (e = imask.upload(*m)) != hipSuccess) return e;
  if (f && (e = frac.upload(*f)) != hipSuccess) return e;
  std::swap(h.imask, imask);
  std::swap(h.frac, frac);
  e = refresh_desc(h);
  if (e != hipSuccess) {
    std::swap(h.imask, imask);
    std::swap(h.frac, frac);
  }
  return e;
}
// the descriptor names the handle's vectors, and those are live blocks (or null)
void check_desc(const EpHandle& h) {
  const Desc* d = h.desc.get();
  CHECK(d && d->imask == h.imask.get() && d->frac == h.frac.get());
  CHECK(!h.imask.get() || g_dev.count(h.imask.get()));
  CHECK(!h.frac.get() || g_dev.count(h.frac.get()));
}
void epilogue_sequence() {
  const std::vector<unsigned char> m0{1, 0, 1}, m1{0, 0, 1};
  const std::vector<double> f0{0.5, 1.0, 0.0}, f1{0.1, 0.2, 0.3};
  for (int variant = 0; variant < 3; ++variant) {   // replace both, drop the mask, first vectors of a bare handle
    const char* names[] = {"set_epilogue_replace", "set_epilogue_drop_mask", "set_epilogue_first"};
    every_failure(names[variant], [&] {
      EpHandle h;
      const long k = g_fail_at;
      g_fail_at = 0;   // the state before the call under test is built without failures
      CHECK(refresh_desc(h) == hipSuccess);
      if (variant < 2) CHECK(set_epilogue(h, &m0, &f0) == hipSuccess);
      const size_t live0 = live();
      const unsigned char* const im0 = h.imask.get();
      const double* const fr0 = h.frac.get();
      check_desc(h);
      g_calls = 0;
      g_fail_at = k;
      const hipError_t e = set_epilogue(h, variant == 1 ? nullptr : &m1, &f1);
      if (e != hipSuccess) {   // exactly as before: same blocks, same contents, descriptor untouched
        CHECK(h.imask.get() == im0 && h.frac.get() == fr0 && live() == live0);
        if (variant < 2) CHECK(memcmp(h.imask.get(), m0.data(), 3) == 0 && memcmp(h.frac.get(), f0.data(), 24) == 0);
      } else {                 // the new vectors; the old ones were freed only now
        CHECK(variant == 1 ? empty(h.imask) : memcmp(h.imask.get(), m1.data(), 3) == 0);
        CHECK(memcmp(h.frac.get(), f1.data(), 24) == 0 && live() == (variant == 1 ? 2u : 3u));
      }
      check_desc(h);
    });
  }
}

// ---- HostPipe::ensure's grow rule for a pair of buffers: per buffer free then allocate; the pair's capacity (its
// smaller buffer) is zero after a failure, so the next call allocates both again
template <typename B>
hipError_t grow(B (&buf)[2], size_t need) {
  hipError_t e = hipSuccess;
  if (need <= std::min(buf[0].bytes(), buf[1].bytes())) return e;
  for (int i = 0; i < 2 && e == hipSuccess; ++i) e = buf[i].alloc(need);
  return e;
}
template <typename B>
void grow_sequence(const char* name) {
  every_failure(name, [&] {
    B buf[2];
    const long k = g_fail_at;
    g_fail_at = 0;
    CHECK(grow(buf, 32) == hipSuccess && live() == 2);
    g_calls = 0;
    g_fail_at = k;
    CHECK(grow(buf, 16) == hipSuccess && g_calls == 0);   // large enough: no HIP call
    const hipError_t e = grow(buf, 64);
    if (e != hipSuccess) {
      CHECK(std::min(buf[0].bytes(), buf[1].bytes()) == 0 && live() <= 1);
      g_fail_at = 0;
      CHECK(grow(buf, 64) == hipSuccess);                 // the next call starts over
    }
    CHECK(buf[0].bytes() == 64 && buf[1].bytes() == 64 && live() == 2);
  });
}
}  // namespace

int main() {
  basics();
  sb_sequence();
  epilogue_sequence();
  grow_sequence<DeviceBuf<char>>("grow_device_pair");
  grow_sequence<PinnedBuf>("grow_pinned_pair");
  CHECK(live() == 0);
  printf("DEVMEMBAD %ld\n", g_bad);
  return 0;
}
