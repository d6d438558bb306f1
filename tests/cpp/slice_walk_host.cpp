// slice_walk_host.cpp — the host-compilable part of lneto_amd/csrc/slice_walk.hpp
// (slice_grid, slice_bounds, frame_len, written_wanted), compiled stand-alone for
// tests/test_slice_walk_host.py: no GPU.  Built a second time with
// AddressSanitizer and UBSan; nothing but this program is loaded.
//
// For block = 256, cap in {512, 1024} and n at and around every edge of the
// grid: G = min(max(ceil(n / 256), 1), cap); the G slices are in order,
// disjoint and cover exactly [0, n); every start is a multiple of 256 (or n,
// for a slice past the end); slices past the end are empty, not inverted.
#include <cstdio>
#include "../../lneto_amd/csrc/slice_walk.hpp"

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

static void slices(uint64_t n, uint32_t block, uint32_t cap) {
  const int before = g_fail;
  const uint32_t G = lnx::slice_grid(n, block, cap);
  const uint64_t chunks = (n + block - 1) / block;
  const uint64_t want = chunks < 1 ? 1 : (chunks < cap ? chunks : cap);
  CHECK(G == want);
  uint64_t at = 0;  // the end of the slice before
  for (uint32_t g = 0; g < G; ++g) {
    uint64_t lo = ~0ull, hi = ~0ull;
    lnx::slice_bounds(n, block, g, G, lo, hi);
    CHECK(lo == at);                       // in order, disjoint, no gap
    CHECK(lo <= hi && hi <= n);            // never inverted, never past n
    CHECK(lo % block == 0 || lo == n);     // whole chunks
    CHECK((hi - lo) % block == 0 || hi == n);
    if (lo == n) CHECK(hi == n);           // past the end: empty
    at = hi;
  }
  CHECK(at == n);                          // exactly [0, n)
  printf("n %llu cap %u: G %u%s\n", (unsigned long long)n, cap, G, g_fail == before ? " ok" : "");
}

int main() {
  const uint32_t block = 256;
  const uint32_t caps[] = {512, 1024};
  for (uint32_t cap : caps) {
    const uint64_t full = (uint64_t)block * cap;
    const uint64_t ns[] = {0, 1, 255, 256, 257, full - 1, full, full + 1, 3 * full + 77, 0xFFFFFFFFull};
    for (uint64_t n : ns) slices(n, block, cap);
  }
  // frame_len: a reversed pair is an empty frame; a span above 2^31 clamps to 2^31 - 1 before the trim; a trim
  // larger than the frame leaves nothing
  CHECK(lnx::frame_len(100, 40, 0) == 0 && lnx::frame_len(100, 40, 4) == 0);
  CHECK(lnx::frame_len(40, 100, 0) == 60 && lnx::frame_len(40, 100, 4) == 56);
  CHECK(lnx::frame_len(7, 7, 0) == 0);
  CHECK(lnx::frame_len(0, 0x80000001ull, 0) == 0x7FFFFFFFu && lnx::frame_len(0, 0x80000001ull, 4) == 0x7FFFFFFBu);
  CHECK(lnx::frame_len(5, ~0ull, 4) == 0x7FFFFFFBu && lnx::frame_len(0, 0x7FFFFFFEull, 0) == 0x7FFFFFFEu);
  CHECK(lnx::frame_len(10, 13, 4) == 0 && lnx::frame_len(10, 14, 4) == 0 && lnx::frame_len(10, 15, 4) == 1);
  CHECK(lnx::frame_len(0, 1, 0xFFFFFFFFu) == 0);
  // written_wanted: the first `cap` of the total are written, all of it is wanted; a cap above 2^32 changes nothing
  const struct { uint32_t total; uint64_t cap; uint32_t written; } ww[] = {
      {0, 0, 0}, {7, 0, 0}, {7, 6, 6}, {7, 7, 7}, {7, 8, 7}, {0xFFFFFFFFu, 0xFFFFFFFEull, 0xFFFFFFFEu},
      {0xFFFFFFFFu, 0x100000000ull, 0xFFFFFFFFu}, {5, ~0ull, 5}};
  for (const auto& c : ww) {
    uint32_t d_n[4] = {0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u, 0xA5A5A5A5u};
    lnx::written_wanted(d_n + 1, c.total, c.cap);
    CHECK(d_n[0] == 0xA5A5A5A5u && d_n[1] == c.written && d_n[2] == c.total && d_n[3] == 0xA5A5A5A5u);
  }
  printf(g_fail ? "FAILED %d\n" : "frame_len: ok\n", g_fail);
  return g_fail ? 1 : 0;
}
