// reply_host.cpp — the RST replies of reply_plan.hpp one at a time on the host:
// lnx_ip4_id_chain, lnx_rx_rst_entry and lnx_tcp_rst_frame, the per-frame
// reference of the batch entries (reply_kernel.hip).  Plain C++17 with no HIP in
// it: the library builds it, and tests/cpp/reply_plan_host.cpp builds it again
// with g++ under AddressSanitizer and UBSan, together with table_images.cpp,
// whose RST image gives the FCS here as it does in the kernel (slot_frame.hpp).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "host_path.hpp"
#include "reply_plan.hpp"

extern "C" void lnx_ip4_id_chain(uint8_t ip4_first, uint16_t ip_id, uint64_t n, uint16_t* out) {
  uint32_t id = ip_id;
  for (uint64_t k = 0; out && k < n; ++k) out[k] = (uint16_t)(id = lnxr::ip4_id_next(id, ip4_first));
}

extern "C" int lnx_rx_rst_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_tcp_rst* out) {
  if (!rec || !out || (len > 0 && !frame)) return LNX_EINVAL;
  const lnx::HostFrame fr(frame, len);
  if (!lnxr::rst_queues(fr.L, rec->flags, rec->l4_off, fr.byt())) return 0;
  const lnxr::RstEntry e = lnxr::rst_entry_of(rec->l4_off, rec->src_port, rec->dst_port, fr.be32());
  static_assert(sizeof(lnx_tcp_rst) == 20, "include/lneto_amd.h");
  lnx_tcp_rst r;
  lnx::put_addr_be(e.addr, r.remote_addr);
  r.remote_port = (uint16_t)e.remote_port, r.local_port = (uint16_t)e.local_port;
  r.seq = e.seq, r.ack = e.ack;
  r.flags = (uint16_t)e.flags, r.zero = 0;
  *out = r;
  return 1;
}

extern "C" int lnx_tcp_rst_frame(const lnx_rst_cfg* cfg, const lnx_tcp_rst* entry, uint16_t ip_id, uint8_t out[64],
                                 uint32_t* len) {
  if (!cfg || !entry || !out || !len || (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  const lnxr::RstCfg c = lnxr::rst_cfg_of(*cfg);
  lnxr::RstEntry e;
  e.addr = lnx::addr_be(entry->remote_addr);
  e.remote_port = entry->remote_port, e.local_port = entry->local_port;
  e.seq = entry->seq, e.ack = entry->ack, e.flags = entry->flags;
  const uint32_t ip_sum = lnxr::rst_ip_sum(c, e, ip_id), tcp_sum = lnxr::rst_tcp_sum(c, e);
  *len = lnx::slot_frame(c.fcs, out, [&](uint32_t p) -> uint32_t {
    return lnxr::rst_word(p, lnxr::rst_fixed_word(p, c), e, ip_id, ip_sum, tcp_sum);
  });
  return LNX_OK;
}
