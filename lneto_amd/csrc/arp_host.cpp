// arp_host.cpp — the ARP rules of arp_plan.hpp one frame at a time on the host:
// lnx_rx_arp_entry and lnx_arp_frame, the per-frame reference of the batch
// entries (arp_kernel.hip).  Plain C++17 with no HIP in it: the library builds
// it, and tests/cpp/arp_plan_host.cpp builds it again with g++ under
// AddressSanitizer and UBSan, together with table_images.cpp, whose RST image
// gives the FCS here as it does in the kernel (slot_frame.hpp).
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "arp_plan.hpp"
#include "host_path.hpp"

namespace {

void put_entry(const lnxa::ArpEntry& e, lnx_arp_entry* out) {
  static_assert(sizeof(lnx_arp_entry) == 12 && sizeof(lnx_arp_seen) == 16, "include/lneto_amd.h");
  lnx_arp_entry r;
  for (uint32_t i = 0; i < 4; ++i) r.hw[i] = (uint8_t)(e.d0 >> (8 * i)), r.ip[i] = (uint8_t)(e.d2 >> (8 * i));
  r.hw[4] = (uint8_t)e.d1, r.hw[5] = (uint8_t)(e.d1 >> 8);
  r.zero = 0;
  *out = r;
}

lnxa::ArpEntry get_entry(const lnx_arp_entry& in) {
  lnxa::ArpEntry e;
  for (uint32_t i = 0; i < 4; ++i) e.d0 |= (uint32_t)in.hw[i] << (8 * i), e.d2 |= (uint32_t)in.ip[i] << (8 * i);
  e.d1 = in.hw[4] | ((uint32_t)in.hw[5] << 8);
  return e;
}

}  // namespace

extern "C" int lnx_rx_arp_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, const lnx_rst_cfg* cfg,
                                lnx_arp_entry* out, uint8_t* verdict) {
  if (!rec || !out || !cfg || (len > 0 && !frame)) return LNX_EINVAL;
  const lnx::HostFrame fr(frame, len);
  if (verdict) *verdict = 0;
  if (!lnxa::arp_reaches(fr.L, rec->verdict, rec->handler, fr.be16())) return 0;
  uint32_t v = 0;
  const uint32_t kind = lnxa::arp_demux(fr.L, lnxa::arp_cfg_of(*cfg), fr.byt(), v);
  if (verdict) *verdict = (uint8_t)v;
  if (kind == lnxa::kArpNone) return 0;
  put_entry(lnxa::arp_entry_of(fr.byt()), out);
  return (int)kind;
}

extern "C" int lnx_arp_frame(const lnx_rst_cfg* cfg, uint16_t op, const lnx_arp_entry* e, uint8_t out[64], uint32_t* len) {
  if (!cfg || !e || !out || !len || !lnxa::arp_op_ok(op) || (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  const lnxa::ArpCfg c = lnxa::arp_cfg_of(*cfg);
  const lnxa::ArpEntry en = get_entry(*e);
  *len = lnx::slot_frame(c.fcs, out, [&](uint32_t p) -> uint32_t { return lnxa::arp_word(p, lnxa::arp_fixed_word(p, c), en, op); });
  return LNX_OK;
}
