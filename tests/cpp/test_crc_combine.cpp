// lnx_crc32_combine and ethernet::CRC32Combine against CRCs taken over the
// bytes themselves.  A program of its own, linked with cpu_path.cpp alone (no
// HIP), so that it can be built with -fsanitize=address,undefined and run
// directly (tests/test_crc_chain.py).
#include <cstdio>
#include <cstring>
#include <vector>

#include "lneto_amd.hpp"

static int failures = 0;
#define EXPECT(cond, ...)                             \
  do {                                                \
    if (!(cond)) {                                    \
      std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
      std::printf(__VA_ARGS__);                       \
      std::printf("\n");                              \
      ++failures;                                     \
    }                                                 \
  } while (0)

static uint64_t rng_state = 0x6C6E65746Full;
static uint64_t next64() {  // splitmix64
  uint64_t z = (rng_state += 0x9E3779B97F4A7C15ull);
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

int main() {
  const size_t lens[] = {0, 1, 2, 3, 4, 5, 59, 60, 64, 1500, 9000, 70000};
  for (size_t lb : lens) {
    for (size_t la : {size_t(0), size_t(1), size_t(61), size_t(2048)}) {
      std::vector<uint8_t> ab(la + lb);
      for (auto& x : ab) x = uint8_t(next64());
      const lneto::Bytes all(ab), a = all.sub(0, la), b = all.sub(la, la + lb);
      EXPECT(ethernet::CRC32Combine(ethernet::CRC32(a), ethernet::CRC32(b), lb) == ethernet::CRC32(all),
             "concatenation %zu + %zu", la, lb);
      const uint32_t seed = uint32_t(next64());
      EXPECT(lnx_crc32_combine(seed, ethernet::CRC32(b), lb) == ethernet::CRC32Update(seed, b.p, b.n),
             "seed over %zu bytes", lb);
    }
  }
  // a frame in five pieces, some empty, folded left to right and right to left
  {
    std::vector<uint8_t> f(9000);
    for (auto& x : f) x = uint8_t(next64());
    const size_t cut[] = {0, 2048, 2048, 4096, 8192, 9000};
    uint32_t left = 0xDEADBEEFu;
    for (int k = 0; k < 5; ++k)
      left = lnx_crc32_combine(left, lnx_crc32(f.data() + cut[k], cut[k + 1] - cut[k]), cut[k + 1] - cut[k]);
    EXPECT(left == lnx_crc32_update(0xDEADBEEFu, f.data(), f.size()), "left fold");
    uint32_t right = 0;
    uint64_t rl = 0;
    for (int k = 4; k >= 0; --k) {
      right = lnx_crc32_combine(lnx_crc32(f.data() + cut[k], cut[k + 1] - cut[k]), right, rl);
      rl += cut[k + 1] - cut[k];
    }
    EXPECT(lnx_crc32_combine(0xDEADBEEFu, right, rl) == left, "right fold");
  }
  // lengths no buffer holds: x has order 2^32 - 1, so k and k + (2^32 - 1) * j advance alike (8 is a unit mod it)
  for (int i = 0; i < 64; ++i) {
    const uint32_t a = uint32_t(next64()), b = uint32_t(next64());
    const uint64_t k = next64() >> 34, j = next64() >> 35;
    EXPECT(lnx_crc32_combine(a, b, k) == lnx_crc32_combine(a, b, k + 0xFFFFFFFFull * j), "order of x, k = %llu",
           (unsigned long long)k);
  }
  EXPECT(lnx_crc32_combine(0x12345678u, 0, 0) == 0x12345678u, "identity");
  EXPECT(lnx_crc32_combine(0, 0x9ABCDEF0u, ~0ull) == 0x9ABCDEF0u, "zero left operand");
  if (failures == 0) std::printf("ok\n");
  return failures ? 1 : 0;
}
