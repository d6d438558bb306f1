// host_path.hpp — host_path.cpp's per-frame host forms, for the packet
// entries of rx_ring.hip (batches below the ring's host threshold) and the
// per-frame C entries.  No HIP here.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rx_filter.hpp"

namespace lnx {

// four address bytes as a big-endian number, and back
inline uint32_t addr_be(const uint8_t a[4]) { return ((uint32_t)a[0] << 24) | ((uint32_t)a[1] << 16) | ((uint32_t)a[2] << 8) | a[3]; }
inline void put_addr_be(uint32_t v, uint8_t a[4]) {
  for (uint32_t i = 0; i < 4; ++i) a[i] = (uint8_t)(v >> (24 - 8 * i));
}

// One frame of the caller's for the plan headers (reply_plan.hpp, echo_plan.hpp,
// arp_plan.hpp): L, and the accessors they take.  The accessors check nothing:
// a plan calls one only once its range is known to lie below L.
struct HostFrame {
  const uint8_t* f;
  uint32_t L;  // len, as far as the plans' 32-bit offsets reach
  HostFrame(const uint8_t* frame, size_t len) : f(frame), L(len < 0x7FFFFFFFu ? (uint32_t)len : 0x7FFFFFFFu) {}
  auto byt() const {
    return [f = f](uint32_t o) -> uint32_t { return f[o]; };
  }
  auto be16() const {
    return [f = f](uint32_t o) -> uint32_t { return ((uint32_t)f[o] << 8) | f[o + 1]; };
  }
  auto be32() const {
    return [f = f](uint32_t o) -> uint32_t { return addr_be(f + o); };
  }
};

uint8_t host_verdict(const uint8_t* fr, size_t L, uint32_t flags, const RxFilter& f);
uint8_t host_pcap(const uint8_t* fr, size_t L);
uint8_t host_tx_checksum(uint8_t* f, size_t L);
uint8_t host_fcs_append(uint8_t* f, uint32_t* len, uint32_t capacity);
uint8_t host_fcs_ok(const uint8_t* f, size_t L);
// echo_host.cpp: lnx_rx_echo_entry and lnx_icmp_echo_reply_frame (echo_plan.hpp)
int host_echo_entry(const uint8_t* frame, size_t len, const lnx_rx_delivery* rec, lnx_icmp_echo* out);
int host_echo_reply_frame(const lnx_rst_cfg* cfg, const lnx_icmp_echo* e, const uint8_t* data, uint16_t ip_id, uint8_t* out,
                          uint32_t out_cap, uint32_t* len);

}  // namespace lnx
