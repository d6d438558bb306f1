// lnx_crc32_search at the limits of min_off: every int64 value above len - 4
// gives -1 and reads nothing (the header's promise; Go itself panics there), and
// every value at or below it gives the first hit at or after max(min_off, 0).
// A program of its own, linked with cpu_path.cpp alone (no HIP), so that it can
// be built with -fsanitize=address,undefined and run directly
// (tests/test_search_octets.py).  Each capture is a heap block of exactly its
// length, so a read past it is a report.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <vector>

#include "lneto_amd.h"

static int failures = 0;

static uint64_t rng_state = 0x7365617263ull;
static uint64_t next64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// bit-serial CRC-32/ISO-HDLC: nothing shared with the library
static uint32_t crc_ref(const uint8_t* p, size_t n) {
  uint32_t c = 0xFFFFFFFFu;
  for (size_t i = 0; i < n; ++i) {
    c ^= p[i];
    for (int b = 0; b < 8; ++b) c = (c >> 1) ^ (c & 1u ? 0xEDB88320u : 0u);
  }
  return ~c;
}

// the definition, with no sum of min_off: -1 when min_off > n - 4
static int64_t search_ref(const uint8_t* p, size_t n, int64_t m) {
  if (m < 0) m = 0;
  if (n < 4 || (uint64_t)m > n - 4) return -1;
  for (size_t off = (size_t)m; off + 4 <= n; ++off) {
    const uint32_t got = (uint32_t)p[off] | (uint32_t)p[off + 1] << 8 | (uint32_t)p[off + 2] << 16 |
                         (uint32_t)p[off + 3] << 24;
    if (crc_ref(p, off) == got) return (int64_t)off;
  }
  return -1;
}

// a capture of n bytes; cut >= 0 places LE32(CRC32(capture[:cut])) at cut
static std::unique_ptr<uint8_t[]> capture(size_t n, int cut) {
  std::unique_ptr<uint8_t[]> p(new uint8_t[n]);
  for (size_t i = 0; i < n; ++i) p[i] = (uint8_t)next64();
  if (cut >= 0) {
    const uint32_t c = crc_ref(p.get(), (size_t)cut);
    for (int k = 0; k < 4; ++k) p[(size_t)cut + k] = (uint8_t)(c >> (8 * k));
  }
  return p;
}

int main() {
  struct Case { size_t n; int cut; };
  const Case cases[] = {{0, -1}, {3, -1}, {4, -1}, {4, 0}, {7, -1}, {7, 0}, {7, 3},
                        {200, -1}, {200, 0}, {200, 100}, {200, 195}, {200, 196}};
  int hits = 0, misses = 0, cut_off_by_min = 0;
  for (const Case& cs : cases) {
    const auto p = capture(cs.n, cs.cut);
    const int64_t n = (int64_t)cs.n;
    const int64_t mins[] = {INT64_MIN, -1, 0, n - 4, n - 3, (int64_t)1 << 31, (int64_t)1 << 32,
                            INT64_MAX - 4, INT64_MAX - 3, INT64_MAX,
                            cs.cut >= 0 ? cs.cut : 1, cs.cut >= 0 ? cs.cut + 1 : 2};
    for (int64_t m : mins) {
      const int64_t want = search_ref(p.get(), cs.n, m), got = lnx_crc32_search(p.get(), cs.n, m);
      if (m > n - 4 && want != -1) {
        std::printf("FAIL the reference itself: n=%zu min_off=%lld\n", cs.n, (long long)m);
        ++failures;
      }
      if (got != want) {
        std::printf("FAIL n=%zu cut=%d min_off=%lld: got %lld, want %lld\n", cs.n, cs.cut, (long long)m,
                    (long long)got, (long long)want);
        ++failures;
      }
      if (want >= 0) ++hits; else ++misses;
      if (cs.cut >= 0 && m > cs.cut && want == -1) ++cut_off_by_min;
    }
  }
  // the classes are there: hits, -1, and a hit that min_off alone excludes
  if (hits < 10 || misses < 60 || cut_off_by_min < 30) {
    std::printf("FAIL classes: hits=%d misses=%d cut_off_by_min=%d\n", hits, misses, cut_off_by_min);
    ++failures;
  }
  if (failures) return 1;
  std::printf("ok %d hits %d misses\n", hits, misses);
  return 0;
}
