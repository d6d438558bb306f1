// lnx_sum_partial and lnx_sum16_chain in a program of their own, compiled
// together with lneto_amd/csrc/sum_chain_host.cpp under ASan + UBSan
// (tests/test_sum_chain.py).  The expected values come from a restatement of
// lneto's crc.go:17-59 over the concatenated bytes; every buffer is a heap
// allocation of exactly its length, so a read past a piece is caught.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>
#include "lneto_amd.h"

static uint32_t rng_state = 0x2545F491u;
static uint32_t rnd() {  // xorshift32
  rng_state ^= rng_state << 13;
  rng_state ^= rng_state >> 17;
  rng_state ^= rng_state << 5;
  return rng_state;
}

// crc.go:23-28, 52-58 without the last fold: big-endian words, an odd last byte << 8
static uint32_t ref_raw(uint32_t sum, const std::vector<uint8_t>& b) {
  size_t i = 0;
  for (; i + 1 < b.size(); i += 2) sum += (uint32_t)((b[i] << 8) | b[i + 1]);
  if (i < b.size()) sum += (uint32_t)b[i] << 8;
  return sum;
}
static uint16_t ref_sum16(uint32_t sum) {  // crc.go:17-21
  sum = (sum & 0xffffu) + (sum >> 16);
  return (uint16_t)~(uint16_t)(sum + (sum >> 16));
}

static int failures = 0;
#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      std::printf("FAIL line %d: %s\n", __LINE__, #c);          \
      ++failures;                                               \
    }                                                           \
  } while (0)

static void run(uint32_t seed, const std::vector<size_t>& lens, int fill) {
  std::vector<uint8_t*> heap;
  std::vector<const uint8_t*> ptr;
  std::vector<uint8_t> all;
  for (size_t n : lens) {
    uint8_t* p = n ? new uint8_t[n] : nullptr;  // an empty segment's pointer is never read
    for (size_t i = 0; i < n; ++i) p[i] = fill >= 0 ? (uint8_t)fill : (uint8_t)rnd();
    all.insert(all.end(), p, p + n);
    heap.push_back(p);
    ptr.push_back(p);
  }
  const uint32_t raw = ref_raw(seed, all);
  CHECK(lnx_sum16_chain(seed, ptr.data(), lens.data(), lens.size()) == ref_sum16(raw));
  // the same frame piece by piece, the phase taken from the bytes so far
  uint32_t s = seed;
  size_t pos = 0;
  for (size_t k = 0; k < lens.size(); ++k) {
    s = lnx_sum_partial(s, ptr[k], lens[k], (int)(pos & 1));
    pos += lens[k];
  }
  CHECK(s == raw);
  CHECK(lnx_sum_partial(seed, all.data(), all.size(), 0) == raw);
  // odd phase: the frame behind one more byte
  std::vector<uint8_t> shifted(1, 0x5A);
  shifted.insert(shifted.end(), all.begin(), all.end());
  CHECK(lnx_sum_partial(ref_raw(seed, std::vector<uint8_t>(1, 0x5A)), all.data(), all.size(), 1) == ref_raw(seed, shifted));
  for (uint8_t* p : heap) delete[] p;
}

int main() {
  static const size_t kLens[] = {0, 1, 2, 3, 5, 64, 127, 129};
  for (int it = 0; it < 3000; ++it) {
    const uint32_t seed = it % 3 == 0 ? 0u : (it % 3 == 1 ? 0xFFFFFFFFu : rnd());
    std::vector<size_t> lens(rnd() % 9);
    for (size_t& n : lens) n = kLens[rnd() % 8];
    run(seed, lens, -1);
  }
  run(0x12345678u, {}, -1);  // m == 0: sum16 of the seed
  CHECK(lnx_sum16_chain(0x12345678u, nullptr, nullptr, 0) == ref_sum16(0x12345678u));
  run(7u, {0, 0, 0}, -1);
  // the wrap: 140004 bytes of 0xFF from 0xFFFFFFF0 pass 2^32 twice
  {
    std::vector<uint8_t> a(70001, 0xFF), b(3, 0xFF), c(70000, 0xFF);
    const uint8_t* seg[3] = {a.data(), b.data(), c.data()};
    const size_t len[3] = {a.size(), b.size(), c.size()};
    uint32_t s = lnx_sum_partial(0xFFFFFFF0u, seg[0], len[0], 0);
    s = lnx_sum_partial(s, seg[1], len[1], 1);
    s = lnx_sum_partial(s, seg[2], len[2], 0);
    CHECK(s == 0x1170EE7Eu);
    CHECK(lnx_sum16_chain(0xFFFFFFF0u, seg, len, 3) == 17);
  }
  run(0xFFFFFFF0u, {70001, 3, 70000}, 0xFF);
  if (failures) return 1;
  std::printf("ok\n");
  return 0;
}
