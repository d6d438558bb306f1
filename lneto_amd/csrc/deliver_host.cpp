// deliver_host.cpp — lnx_rx_deliver: the delivery record of ONE frame on the
// host, from the rules the kernel applies (deliver_plan.hpp).  Plain C++17 with
// no HIP in it: the library builds it, and tests/cpp/deliver_plan_host.cpp
// builds it again with g++ under AddressSanitizer and UBSan.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "deliver_plan.hpp"

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
