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

}  // namespace lnx
