// arp_host.cpp — the ARP rules of arp_plan.hpp one frame at a time on the host:
// lnx_rx_arp_entry and lnx_arp_frame, the per-frame reference of the batch
// entries (arp_kernel.hip).  Plain C++17 with no HIP in it: the library builds
// it, and tests/cpp/arp_plan_host.cpp builds it again with g++ under
// AddressSanitizer and UBSan, together with table_images.cpp, whose RST image
// gives the FCS here as it does in the kernel.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include <vector>
#include "arp_plan.hpp"
#include "table_images.hpp"
#include "table_layout.hpp"

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
  const uint32_t L = len < 0x7FFFFFFFu ? (uint32_t)len : 0x7FFFFFFFu;
  auto byt = [&](uint32_t o) -> uint32_t { return frame[o]; };
  auto be16 = [&](uint32_t o) -> uint32_t { return ((uint32_t)frame[o] << 8) | frame[o + 1]; };
  if (verdict) *verdict = 0;
  if (!lnxa::arp_reaches(L, rec->verdict, rec->handler, be16)) return 0;
  uint32_t v = 0;
  const uint32_t kind = lnxa::arp_demux(L, lnxa::arp_cfg_of(*cfg), byt, v);
  if (verdict) *verdict = (uint8_t)v;
  if (kind == lnxa::kArpNone) return 0;
  put_entry(lnxa::arp_entry_of(byt), out);
  return (int)kind;
}

extern "C" int lnx_arp_frame(const lnx_rst_cfg* cfg, uint16_t op, const lnx_arp_entry* e, uint8_t out[64], uint32_t* len) {
  if (!cfg || !e || !out || !len || !lnxa::arp_op_ok(op) || (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  static const std::vector<uint32_t> image = lnx::build_rst_image();
  const lnxa::ArpCfg c = lnxa::arp_cfg_of(*cfg);
  const lnxa::ArpEntry en = get_entry(*e);
  auto tab = [&](uint32_t p, uint32_t i, uint32_t v) -> uint32_t { return image[lnx::rst_nib(p, i, v)]; };
  uint32_t reg = 0;
  for (uint32_t p = 0; p < lnxa::kArpWords; ++p) {
    uint32_t w = 0;
    if (p < lnx::kRstLanes) {
      w = lnxa::arp_word(p, lnxa::arp_fixed_word(p, c), en, op);
      reg ^= lnxr::rst_fcs_part(p, w, tab);
    } else if (c.fcs) {
      w = ~reg;
    }
    for (uint32_t b = 0; b < 4; ++b) out[4 * p + b] = (uint8_t)(w >> (8 * b));  // little-endian dwords
  }
  *len = c.fcs ? 64u : lnxa::kArpPadded;
  return LNX_OK;
}
