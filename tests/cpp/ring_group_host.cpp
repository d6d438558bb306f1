// ring_group_host.cpp — the host side of the receive ring's grouping
// (lneto_amd/csrc/deliver_host.cpp: lnxd::merge_groups, lnxd::group_records),
// compiled stand-alone for tests/test_ring_group_host.py: no GPU.  Built a second
// time with AddressSanitizer and UBSan (with -DNO_LIBRARY: nothing but this
// program is loaded), every array in a heap block of exactly its size.
//
// merge: a call of n frames with random buckets is cut into internal batches;
// each batch's order / count are made by a stable sort of its own frames (what
// the grouping launches give), merged, and compared with a stable sort of the
// whole call.  group_records: the same from the records.  Without NO_LIBRARY
// the program also links the library and checks the argument refusals of the
// three ring entries and the batch entry that need no device.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <numeric>
#include <vector>
#include "../../lneto_amd/csrc/deliver_host.cpp"

static int g_fail = 0;
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      printf("FAIL %s:%d: %s\n", __FILE__, __LINE__, #c);     \
      ++g_fail;                                               \
    }                                                         \
  } while (0)

static uint32_t g_rng = 12345;
static uint32_t rnd() { return g_rng = g_rng * 1664525u + 1013904223u; }

constexpr uint32_t kB = lnxd::kGroupBuckets;

// stable sort of frames [0, n) by bucket: the order and the bucket sizes
static void reference(const std::vector<uint32_t>& bucket, std::vector<uint32_t>& order, std::vector<uint32_t>& count) {
  order.resize(bucket.size());
  std::iota(order.begin(), order.end(), 0u);
  std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return bucket[a] < bucket[b]; });
  count.assign(kB, 0);
  for (uint32_t b : bucket) count[b] += 1;
}

// bucket of a record as the kernels key it
static lnx_rx_delivery record_of(uint32_t bucket) {
  lnx_rx_delivery d;
  std::memset(&d, 0, sizeof d);
  d.handler = bucket == LNX_H_COUNT ? (uint16_t)LNX_H_NONE : (uint16_t)bucket;
  d.verdict = bucket == LNX_H_COUNT ? 2 : 0;
  return d;
}

static void run_case(const char* name, const std::vector<uint32_t>& bucket, const std::vector<uint32_t>& sizes) {
  const uint32_t n = (uint32_t)bucket.size();
  std::vector<uint32_t> first, bn, want_order, want_count;
  uint32_t at = 0;
  for (uint32_t s : sizes) first.push_back(at), bn.push_back(s), at += s;
  CHECK(at == n);
  reference(bucket, want_order, want_count);
  // the batches' own groups, exact-size blocks
  std::vector<uint32_t> border(n), bcount((size_t)sizes.size() * kB);
  for (size_t b = 0; b < sizes.size(); ++b) {
    std::vector<uint32_t> part(bucket.begin() + first[b], bucket.begin() + first[b] + bn[b]), o, c;
    reference(part, o, c);
    std::copy(o.begin(), o.end(), border.begin() + first[b]);
    std::copy(c.begin(), c.end(), bcount.begin() + b * kB);
  }
  std::vector<uint32_t> order(n, 0xEEEEEEEEu), count(kB, 0xEEEEEEEEu);
  lnxd::merge_groups(border.data(), bcount.data(), first.data(), bn.data(), (uint32_t)sizes.size(), order.data(),
                     count.data());
  CHECK(order == want_order);
  CHECK(count == want_count);
  // the host path: a counting sort of the records
  std::vector<lnx_rx_delivery> rec(n);
  for (uint32_t i = 0; i < n; ++i) rec[i] = record_of(bucket[i]);
  std::vector<uint32_t> order2(n, 0xEEEEEEEEu), count2(kB, 0xEEEEEEEEu);
  lnxd::group_records(rec.data(), n, order2.data(), count2.data());
  CHECK(order2 == want_order);
  CHECK(count2 == want_count);
  printf("%s: n=%u batches=%zu %s\n", name, n, sizes.size(), g_fail ? "FAIL" : "ok");
}

#ifndef NO_LIBRARY
static void refusals() {
  lnx_rx_delivery rec[4];
  uint32_t order[4], count[LNX_H_COUNT + 1];
  uint8_t ok[4], v[4];
  lnx_rx_ports big;
  std::memset(&big, 0, sizeof big);
  big.n_tcp = 257;
  // no ring
  CHECK(lnx_rx_ring_set_ports(nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_ring_ingress_deliver(nullptr, 0, 4, 0, 0, ok, v, rec, order, count) == LNX_EINVAL);
  CHECK(lnx_ingress_packets_deliver(nullptr, nullptr, nullptr, 4, 0, 0, ok, v, rec, order, count) == LNX_EINVAL);
  // the outputs' rules come before anything else
  lnx_rx_ring* fake = reinterpret_cast<lnx_rx_ring*>(rec);  // (never dereferenced: refused first)
  CHECK(lnx_rx_ring_ingress_deliver(fake, 0, 4, 0, 0, ok, v, nullptr, order, count) == LNX_EINVAL);
  CHECK(lnx_rx_ring_ingress_deliver(fake, 0, 4, 0, 0, ok, v, rec, order, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_ring_ingress_deliver(fake, 0, 4, 0, 0, ok, v, rec, nullptr, count) == LNX_EINVAL);
  CHECK(lnx_ingress_packets_deliver(fake, nullptr, nullptr, 4, 0, 0, ok, v, nullptr, order, count) == LNX_EINVAL);
  CHECK(lnx_ingress_packets_deliver(fake, nullptr, nullptr, 4, 0, 0, ok, v, rec, order, nullptr) == LNX_EINVAL);
  CHECK(lnx_ingress_packets_deliver(fake, nullptr, nullptr, 4, 0, 0, ok, v, rec, nullptr, count) == LNX_EINVAL);
  CHECK(lnx_rx_ring_set_ports(fake, &big) == LNX_EINVAL);
  // the batch entry: refused before any device call
  alignas(16) lnx_rx_delivery drec[4];
  const uint8_t bytes[64] = {0};
  const uint64_t off[5] = {0, 16, 32, 48, 64};
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, nullptr, ok, v, nullptr, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, nullptr, ok, v, drec, order, nullptr, order, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, nullptr, ok, v, drec, nullptr, count, order, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 1ull << 32, 0, nullptr, nullptr, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 8, nullptr, nullptr, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, &big, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  lnx_rx_filter bad;
  std::memset(&bad, 0, sizeof bad);
  bad.n_ethertypes = 9;
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, &bad, nullptr, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(nullptr, off, 4, 0, nullptr, nullptr, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, nullptr, nullptr, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 4, 0, nullptr, nullptr, ok, v, drec, order, count, nullptr, nullptr) == LNX_EINVAL);
  CHECK(lnx_rx_verify_deliver_batch(bytes, off, 0, 0, nullptr, nullptr, ok, v, drec, nullptr, nullptr, nullptr, nullptr) == LNX_OK);
  printf("refusals: %s\n", g_fail ? "FAIL" : "ok");
}
#endif

int main() {
  auto random_buckets = [](uint32_t n, uint32_t spread) {
    std::vector<uint32_t> b(n);
    for (auto& x : b) {
      const uint32_t r = rnd() >> 8;
      x = r % 5 == 0 ? (uint32_t)LNX_H_COUNT : r % spread;
    }
    return b;
  };
  // 1, 2 and 7 batches (a short last one, as the ring cuts them)
  run_case("one batch", random_buckets(64, LNX_H_COUNT), {64});
  run_case("two batches", random_buckets(64 + 17, 40), {64, 17});
  run_case("seven batches", random_buckets(6 * 64 + 17, 12), {64, 64, 64, 64, 64, 64, 17});
  run_case("seven uneven batches", random_buckets(300, LNX_H_COUNT), {1, 99, 2, 64, 64, 69, 1});
  // empty batches, first, last and in between; an empty call
  run_case("empty batches", random_buckets(130, 9), {0, 64, 0, 0, 64, 2, 0});
  run_case("empty call", {}, {});
  run_case("empty call of empty batches", {}, {0, 0});
  // every frame in one bucket: the first, the last handler id, the frames not delivered
  for (uint32_t h : {0u, (uint32_t)LNX_H_COUNT - 1u, (uint32_t)LNX_H_COUNT})
    run_case("one bucket", std::vector<uint32_t>(200, h), {64, 64, 64, 8});
  // every bucket hit once, in a scrambled arrival order
  {
    std::vector<uint32_t> b(kB);
    std::iota(b.begin(), b.end(), 0u);
    for (uint32_t i = kB - 1; i > 0; --i) std::swap(b[i], b[(rnd() >> 8) % (i + 1)]);
    run_case("every bucket once", b, {64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, 64, kB - 16 * 64});
  }
#ifndef NO_LIBRARY
  refusals();
#endif
  return g_fail ? 1 : 0;
}
