// echo_host.cpp — the echo replies of echo_plan.hpp one at a time on the host:
// lnx_rx_echo_entry and lnx_icmp_echo_reply_frame, the per-frame reference of
// the batch entry (echo_kernel.hip).  Plain C++17 with no HIP in it: the library
// builds it, and tests/cpp/echo_plan_host.cpp builds it again with g++ under
// AddressSanitizer and UBSan.
#include <cstddef>
#include <cstdint>
#include <cstring>
#include "echo_plan.hpp"
#include "host_path.hpp"

namespace lnx {

int host_echo_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_icmp_echo* out) {
  if (!rec || !out || (len > 0 && !frame)) return LNX_EINVAL;
  const HostFrame fr(frame, len);
  if (!lnxe::echo_queues(fr.L, rec->verdict, rec->handler, rec->l4_off, rec->ip_end, fr.byt())) return 0;
  const lnxe::EchoEntry e = lnxe::echo_entry_of(rec->l4_off, rec->ip_end, fr.be16(), fr.be32());
  static_assert(sizeof(lnx_icmp_echo) == 16, "include/lneto_amd.h");
  lnx_icmp_echo r;
  put_addr_be(e.addr, r.remote_addr);
  r.id = (uint16_t)e.id, r.seq = (uint16_t)e.seq;
  r.data_off = e.data_off, r.data_len = e.data_len;
  *out = r;
  return 1;
}

// 6: the library's ErrShortBuffer, as lnx_fcs_append gives it
int host_echo_reply_frame(const lnx_rst_cfg* cfg, const lnx_icmp_echo* e, const uint8_t* data, uint16_t ip_id, uint8_t* out,
                          uint32_t out_cap, uint32_t* len) {
  if (!cfg || !e || !out || !len || (cfg->flags & ~(uint32_t)LNX_TX_FCS)) return LNX_EINVAL;
  const uint32_t d = e->data_len;
  if (d == 0 || d > lnxe::kEchoMaxData || !data) return LNX_EINVAL;  // no entry carries such data (echo_plan.hpp rule 2)
  const lnxe::RstCfg c = lnxr::rst_cfg_of(*cfg);
  const uint32_t padded = lnxe::echo_padded(d), total = lnxe::echo_len(d, c.fcs);
  if (out_cap < total) return 6;
  const uint32_t addr = addr_be(e->remote_addr);
  uint32_t be_sum = (uint32_t)e->id + e->seq;  // type 0, code 0 and the zeroed checksum field add nothing
  for (uint32_t k = 0; k + 1 < d; k += 2) be_sum += ((uint32_t)data[k] << 8) | data[k + 1];
  if (d & 1u) be_sum += (uint32_t)data[d - 1] << 8;
  const uint32_t ip_sum = lnxe::echo_ip_sum(c, addr, d, ip_id), icmp_sum = lnxe::echo_icmp_sum(be_sum);
  for (uint32_t k = 0; k < 20; ++k) {
    const uint32_t f = lnxe::echo_fixed_field(k, c) | lnxe::echo_var_field(k, addr, e->id, d, ip_id, ip_sum, icmp_sum);
    out[2 * k] = (uint8_t)(f >> 8), out[2 * k + 1] = (uint8_t)f;
  }
  out[40] = (uint8_t)(e->seq >> 8), out[41] = (uint8_t)e->seq;
  memcpy(out + lnxe::kEchoHdr, data, d);
  if (lnxe::kEchoHdr + d < padded) memset(out + lnxe::kEchoHdr + d, 0, padded - lnxe::kEchoHdr - d);
  if (c.fcs) {
    uint32_t reg = 0xFFFFFFFFu;
    for (uint32_t k = 0; k < padded; ++k) reg = lnxe::echo_crc_byte(reg, out[k]);
    const uint32_t fcs = ~reg;
    for (uint32_t b = 0; b < 4; ++b) out[padded + b] = (uint8_t)(fcs >> (8 * b));
  }
  *len = total;
  return LNX_OK;
}

}  // namespace lnx

extern "C" int lnx_rx_echo_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_icmp_echo* out) {
  return lnx::host_echo_entry(frame, len, rec, out);
}

extern "C" int lnx_icmp_echo_reply_frame(const lnx_rst_cfg* cfg, const lnx_icmp_echo* e, const uint8_t* data, uint16_t ip_id,
                                         uint8_t* out, uint32_t out_cap, uint32_t* len) {
  return lnx::host_echo_reply_frame(cfg, e, data, ip_id, out, out_cap, len);
}
