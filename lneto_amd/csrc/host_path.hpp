// host_path.hpp — host_path.cpp's per-frame host forms, for the packet
// entries of rx_ring.hip (batches below the ring's host threshold) and the
// per-frame C entries.  No HIP here.
#pragma once
#include <cstddef>
#include <cstdint>
#include "rx_filter.hpp"

namespace lnx {

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
