// deliver_host.cpp — lnx_rx_deliver: the delivery record of ONE frame on the
// host, from the rules the kernel applies (deliver_plan.hpp).  Plain C++17 with
// no HIP in it: the library builds it, and tests/cpp/deliver_plan_host.cpp
// builds it again with g++ under AddressSanitizer and UBSan.  Also the host
// side of the receive ring's grouping (deliver_group.hpp):
// the merge of the internal batches' groups into the call's, and the host
// path's counting sort (tests/cpp/ring_group_host.cpp).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "deliver_group.hpp"
#include "deliver_plan.hpp"

namespace lnxd {

void merge_groups(const uint32_t* batch_order, const uint32_t* batch_count, const uint32_t* first, const uint32_t* n,
                  uint32_t nbatches, uint32_t* order, uint32_t* count) {
  // the buckets' sizes over the call, then their bases in `order`
  std::vector<uint64_t> base(kGroupBuckets + 1u, 0);
  for (uint32_t h = 0; h < kGroupBuckets; ++h) count[h] = 0;
  for (uint32_t b = 0; b < nbatches; ++b)
    for (uint32_t h = 0; h < kGroupBuckets; ++h) count[h] += batch_count[(size_t)b * kGroupBuckets + h];
  for (uint32_t h = 0; h < kGroupBuckets; ++h) base[h + 1] = base[h] + count[h];
  // the batches in arrival order: each bucket's run goes behind the earlier batches' runs
  for (uint32_t b = 0; b < nbatches; ++b) {
    const uint32_t* bo = batch_order + first[b];
    const uint32_t* bc = batch_count + (size_t)b * kGroupBuckets;
    uint64_t at = 0;  // the run's place in the batch's order
    for (uint32_t h = 0; h < kGroupBuckets && at < n[b]; ++h) {
      // (a count that overruns the batch cannot come from the grouping launches: cut, never read past the batch)
      const uint64_t c = bc[h] < n[b] - at ? bc[h] : n[b] - at;
      for (uint64_t i = 0; i < c; ++i) order[base[h] + i] = bo[at + i] + first[b];
      base[h] += c;
      at += c;
    }
  }
}

void group_records(const lnx_rx_delivery* rec, uint64_t n, uint32_t* order, uint32_t* count) {
  auto bucket = [&](uint64_t i) -> uint32_t { return rec[i].handler < LNX_H_COUNT ? rec[i].handler : LNX_H_COUNT; };
  std::vector<uint64_t> base(kGroupBuckets + 1u, 0);
  for (uint32_t h = 0; h < kGroupBuckets; ++h) count[h] = 0;
  for (uint64_t i = 0; i < n; ++i) count[bucket(i)] += 1;
  for (uint32_t h = 0; h < kGroupBuckets; ++h) base[h + 1] = base[h] + count[h];
  for (uint64_t i = 0; i < n; ++i) order[base[bucket(i)]++] = (uint32_t)i;
}

}  // namespace lnxd

extern "C" int lnx_rx_deliver(const uint8_t* frame, size_t len, const lnx_rx_filter* filter, const lnx_rx_ports* ports,
                              int fcs_ok, uint8_t verdict_in, lnx_rx_delivery* out) {
  lnx::RxFilter filt;
  if (!out || (len > 0 && !frame) || !lnx::rx_filter_of(filter, &filt)) return LNX_EINVAL;
  if (ports && (ports->n_tcp > lnxd::kPortsMax || ports->n_udp > lnxd::kPortsMax)) return LNX_EINVAL;
  const uint32_t L = len < 0x7FFFFFFFu ? (uint32_t)len : 0x7FFFFFFFu;
  auto byt = [&](uint32_t o) -> uint32_t { return frame[o]; };
  auto be16 = [&](uint32_t o) -> uint32_t { return ((uint32_t)frame[o] << 8) | frame[o + 1]; };
  lnxd::DlvPlan r = lnxd::dlv_parse(L, verdict_in, fcs_ok < 0 ? -1 : (fcs_ok != 0), filt, be16, byt);
  int32_t k = -1;
  if (r.lookup != 0) {
    if (!ports) {
      k = (int32_t)lnxd::kPortsMax;
    } else {  // nodeByPort: the first match
      const uint16_t* tab = r.lookup == 6 ? ports->tcp : ports->udp;
      const uint32_t cnt = r.lookup == 6 ? ports->n_tcp : ports->n_udp;
      for (uint32_t i = 0; i < cnt && k < 0; ++i)
        if (tab[i] == r.dst_port) k = (int32_t)i;
    }
  }
  lnxd::dlv_finish(r, k);
  uint32_t w[4];
  lnxd::dlv_pack(r, w);
  static_assert(sizeof(lnx_rx_delivery) == 16, "include/lneto_amd.h");
  lnx_rx_delivery d;
  d.ip_end = w[0];
  d.handler = (uint16_t)w[1], d.l4_off = (uint16_t)(w[1] >> 16);
  d.src_port = (uint16_t)w[2], d.dst_port = (uint16_t)(w[2] >> 16);
  d.verdict = (uint8_t)w[3], d.flags = (uint8_t)(w[3] >> 8), d.zero = 0;
  *out = d;
  return LNX_OK;
}
