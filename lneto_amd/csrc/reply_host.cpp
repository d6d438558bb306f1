// reply_host.cpp — the RST replies of reply_plan.hpp one at a time on the host:
// lnx_ip4_id_chain, lnx_rx_rst_entry and lnx_tcp_rst_frame, the per-frame
// reference of the batch entries (reply_kernel.hip).  Plain C++17 with no HIP in
// it: the library builds it, and tests/cpp/reply_plan_host.cpp builds it again
// with g++ under AddressSanitizer and UBSan, together with table_images.cpp,
// whose RST image gives the FCS here as it does in the kernel.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "reply_plan.hpp"
#include "table_images.hpp"
#include "table_layout.hpp"

extern "C" void lnx_ip4_id_chain(uint8_t ip4_first, uint16_t ip_id, uint64_t n, uint16_t* out) {
  uint32_t id = ip_id;
  for (uint64_t k = 0; out && k < n; ++k) out[k] = (uint16_t)(id = lnxr::ip4_id_next(id, ip4_first));
}

extern "C" int lnx_rx_rst_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_tcp_rst* out) {
  if (!rec || !out || (len > 0 && !frame)) return LNX_EINVAL;
  const uint32_t L = len < 0x7FFFFFFFu ? (uint32_t)len : 0x7FFFFFFFu;
  auto byt = [&](uint32_t o) -> uint32_t { return frame[o]; };
  auto be32 = [&](uint32_t o) -> uint32_t {
    return ((uint32_t)frame[o] << 24) | ((uint32_t)frame[o + 1] << 16) | ((uint32_t)frame[o + 2] << 8) | frame[o + 3];
  };
  if (!lnxr::rst_queues(L, rec->flags, rec->l4_off, byt)) return 0;
  const lnxr::RstEntry e = lnxr::rst_entry_of(rec->l4_off, rec->src_port, rec->dst_port, be32);
  static_assert(sizeof(lnx_tcp_rst) == 20, "include/lneto_amd.h");
  lnx_tcp_rst r;
  for (uint32_t i = 0; i < 4; ++i) r.remote_addr[i] = (uint8_t)(e.addr >> (24 - 8 * i));
  r.remote_port = (uint16_t)e.remote_port, r.local_port = (uint16_t)e.local_port;
  r.seq = e.seq, r.ack = e.ack;
  r.flags = (uint16_t)e.flags, r.zero = 0;
  *out = r;
  return 1;
}

extern "C" int lnx_tcp_rst_frame(const lnx_rst_cfg* cfg, const lnx_tcp_rst* entry, uint16_t ip_id, uint8_t out[64],
                                 uint32_t* len) {
  if (!cfg || !entry || !out || !len || (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  static const std::vector<uint32_t> image = lnx::build_rst_image();
  const lnxr::RstCfg c = lnxr::rst_cfg_of(*cfg);
  lnxr::RstEntry e;
  e.addr = ((uint32_t)entry->remote_addr[0] << 24) | ((uint32_t)entry->remote_addr[1] << 16) |
           ((uint32_t)entry->remote_addr[2] << 8) | entry->remote_addr[3];
  e.remote_port = entry->remote_port, e.local_port = entry->local_port;
  e.seq = entry->seq, e.ack = entry->ack, e.flags = entry->flags;
  const uint32_t ip_sum = lnxr::rst_ip_sum(c, e, ip_id), tcp_sum = lnxr::rst_tcp_sum(c, e);
  auto tab = [&](uint32_t p, uint32_t i, uint32_t v) -> uint32_t { return image[lnx::rst_nib(p, i, v)]; };
  uint32_t reg = 0;
  for (uint32_t p = 0; p < lnxr::kRstWords; ++p) {
    uint32_t w = 0;
    if (p < lnx::kRstLanes) {
      w = lnxr::rst_word(p, lnxr::rst_fixed_word(p, c), e, ip_id, ip_sum, tcp_sum);
      reg ^= lnxr::rst_fcs_part(p, w, tab);
    } else if (c.fcs) {
      w = ~reg;
    }
    for (uint32_t b = 0; b < 4; ++b) out[4 * p + b] = (uint8_t)(w >> (8 * b));  // little-endian dwords
  }
  *len = c.fcs ? 64u : lnxr::kRstPadded;
  return LNX_OK;
}
