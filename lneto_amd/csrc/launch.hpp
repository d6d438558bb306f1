// launch.hpp — every function one csrc file defines and another calls: the
// kernels' host launchers (called from api.cpp and rx_ring.hip) and api.cpp's
// device context for rx_ring.hip.  The defining file includes this header
// too, so a signature that drifts from its declaration does not compile.
// Default arguments live here only.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>
#include "../../include/lneto_amd.h"
#include "rx_filter.hpp"

// crc32_combine_kernel.hip: the running-crc forms
namespace lnxc {
hipError_t launch_combine_pairs(const uint32_t* a, const uint32_t* b, const uint64_t* len, uint64_t n, uint32_t* out,
                                int num_cus, hipStream_t stream);
hipError_t launch_seed_pairs(const uint32_t* seed, const uint64_t* off, uint64_t n, uint32_t* crc, int num_cus,
                             hipStream_t stream);
hipError_t launch_chain_fold(const uint32_t* seg_crc, const uint32_t* len, uint64_t nseg, const uint64_t* first,
                             uint64_t nframes, const uint32_t* seed, void* out, bool verify, int num_cus,
                             hipStream_t stream);
}  // namespace lnxc

// sum16_chain_kernel.hip: the running internet checksums
namespace lnxs {
hipError_t launch_sum_bytes(const uint8_t* bytes, const uint64_t* off, const uint32_t* len, const uint32_t* seed,
                            const uint8_t* phase, uint64_t n, uint32_t* out, bool planes, int num_cus,
                            hipStream_t stream);
hipError_t launch_sum_fold(const uint32_t* eo, const uint32_t* len, uint64_t nseg, const uint64_t* first,
                           uint64_t nframes, const uint32_t* seed, uint16_t* out16, uint32_t* sum32, int num_cus,
                           hipStream_t stream);
}  // namespace lnxs

// deliver_kernel.hip: receive delivery
namespace lnxd {
uint64_t deliver_ws_bytes(uint64_t n);
hipError_t launch_deliver(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx::RxFilter& filt,
                          const lnx_rx_ports* ports, const uint8_t* fcs_ok, const uint8_t* verdict, lnx_rx_delivery* rec,
                          uint32_t* order, uint32_t* count, void* ws, hipStream_t stream);
uint16_t* deliver_keys(void* ws, uint64_t n);
hipError_t launch_deliver_group(uint64_t n, uint32_t* order, uint32_t* count, void* ws, hipStream_t stream);
// rx_verify_kernel.hip: the receive check that writes the delivery records too
hipError_t launch_rx_verify_deliver(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t flags, bool fcs,
                                    uint8_t* ok, uint8_t* verdict, const uint32_t* seg_len,
                                    const lnx::RxFilter* filter, const lnx_rx_ports* ports, lnx_rx_delivery* rec,
                                    uint16_t* keys, const uint32_t* image, int num_cus, hipStream_t stream,
                                    bool host = false);
}  // namespace lnxd

// reply_kernel.hip: RST replies for SYNs to closed ports
namespace lnxr {
uint64_t rst_ws_bytes(uint64_t n);
hipError_t launch_rst_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, const uint16_t* ip_id, uint64_t cap, uint8_t* reply, uint32_t* src,
                            uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream);
hipError_t launch_rst_frames(const lnx_rst_cfg& cfg, const lnx_tcp_rst* entry, uint64_t n, const uint16_t* ip_id,
                             uint8_t* reply, const uint32_t* image, hipStream_t stream);
}  // namespace lnxr

// echo_kernel.hip: echo replies for ICMPv4 echo requests
namespace lnxe {
uint64_t echo_ws_bytes(uint64_t n);
hipError_t launch_echo_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                             const lnx_rst_cfg& cfg, const uint16_t* ip_id, uint64_t cap, uint64_t cap_blocks, uint8_t* reply,
                             uint64_t* start, uint32_t* len, uint32_t* src, uint32_t* d_n, void* ws, const uint32_t* image,
                             hipStream_t stream);
}  // namespace lnxe

// arp_kernel.hip: ARP replies and learn records
namespace lnxa {
uint64_t arp_ws_bytes(uint64_t n);
hipError_t launch_arp_reply(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t trim, const lnx_rx_delivery* rec,
                            const lnx_rst_cfg& cfg, uint64_t cap, uint64_t cap_seen, uint8_t* reply, uint32_t* src,
                            lnx_arp_seen* seen, uint32_t* d_n, void* ws, const uint32_t* image, hipStream_t stream);
hipError_t launch_arp_frames(const lnx_rst_cfg& cfg, const lnx_arp_entry* entry, const uint16_t* op, uint64_t n, uint8_t* reply,
                             const uint32_t* image, hipStream_t stream);
}  // namespace lnxa

namespace lnx {

// api.cpp: the current device's images and CU count, and the thread's lnx_last_error
int device_resources(const void** image, int* num_cus, const void** stage_image, const void** rx_image);
int hip_error(hipError_t e, const char* what);

// crc32_kernel.hip
hipError_t launch_crc32_frames(const uint8_t* bytes, const uint64_t* off, uint64_t n, void* out, bool verify,
                               const void* images, int num_cus, hipStream_t stream, uint32_t policy,
                               uint32_t* stage_flag, uint32_t epoch);
hipError_t launch_crc32_segments(const uint8_t* bytes, const uint64_t* start, const uint32_t* len, uint64_t n,
                                 void* out, const void* images, int num_cus, hipStream_t stream);
hipError_t launch_fcs_verify_segments(const uint8_t* bytes, const uint64_t* start, const uint32_t* len, uint64_t n,
                                      uint8_t* ok, const void* images, int num_cus, hipStream_t stream);
hipError_t launch_fcs_append(uint8_t* bytes, const uint64_t* start, uint32_t* len, uint64_t n, uint32_t capacity,
                             uint8_t* status, const void* images, int num_cus, hipStream_t stream, int var = 0);
// stage_kernel.hip
hipError_t launch_crc32_stage(const uint8_t* bytes, const uint64_t* off, uint64_t n, void* out, bool verify,
                              uint32_t policy, const void* image, uint32_t* scratch, int num_cus, hipStream_t stream,
                              const uint32_t* stage_flag, uint32_t epoch);
// rx_verify_kernel.hip
hipError_t launch_rx_verify(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t flags, bool fcs,
                            uint8_t* ok, uint8_t* verdict, const uint32_t* seg_len, const RxFilter* filter,
                            const uint32_t* image, int num_cus, hipStream_t stream, bool host = false,
                            const uint32_t* gate = nullptr, uint32_t epoch = 0);
hipError_t launch_tx_finish(uint8_t* bytes, const uint64_t* start, uint32_t* len, uint64_t n, uint32_t capacity,
                            uint32_t flags, uint8_t* st_ck, uint8_t* st_ap, const uint32_t* image, int num_cus,
                            hipStream_t stream, bool host, const uint32_t* gate = nullptr, uint32_t epoch = 0);
// ingress_kernel.hip
hipError_t launch_ingress_verify(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint32_t flags,
                                 uint8_t* verdict, int num_cus, hipStream_t stream, const uint32_t* seg_len,
                                 uint32_t trim, const RxFilter* filter, uint32_t* gate = nullptr, uint32_t epoch = 0,
                                 uint64_t short_mean = 0);
hipError_t launch_tx_checksum(uint8_t* bytes, const uint64_t* start, const uint32_t* len, uint64_t n,
                              uint8_t* status, int num_cus, hipStream_t stream, uint32_t* gate = nullptr,
                              uint32_t epoch = 0, uint64_t short_mean = 0);
// pcap_kernel.hip, search_kernel.hip, sum16_kernel.hip
hipError_t launch_pcap_verify(const uint8_t* bytes, const uint64_t* off, uint64_t n, uint8_t* status, int num_cus,
                              hipStream_t stream);
hipError_t launch_crc32_search(const uint8_t* bytes, const uint64_t* off, const int64_t* min_off, uint64_t n,
                               const uint32_t* tables, int64_t* result, int num_cus, hipStream_t stream);
hipError_t launch_sum16_segments(const uint8_t* bytes, const uint64_t* off, const uint32_t* len,
                                 const uint32_t* seed, uint64_t n, uint16_t* out, int num_cus,
                                 hipStream_t stream, int var = 0);

#ifdef LNX_RESEARCH
// research/stage_research.hip
namespace rs {
hipError_t launch_crc32_stage_research(const uint8_t* bytes, const uint64_t* off, uint64_t n, void* out, bool verify,
                                       int fold, int waves, const void* image, int num_cus, hipStream_t stream,
                                       bool big_blocks = false);
// lnx__crc32_variant's staged ids (all in stage_research.hip, the round-4
// kernel; the product staged kernel with its round-5 dispatch is
// lnx_crc32_batch_ex(LNX_BATCH_SHORT_FRAMES)).  id: the CRC form; id + 1 is
// its FCS verify form when `verify` is set.
struct StageVariant {
  int id, fold, waves;
  bool big_blocks, verify;
};
inline constexpr StageVariant kStageVariants[] = {
    {300, 2, 8, false, true},    // the staged lane streams (stage_kernel.hip), slicing-by-2 fold
    {302, 4, 8, false, true},    // the 16-column Z_4 fold
    {304, 2, 10, false, true},   // 300 with 10 waves per workgroup instead of 8 (retired)
    {306, 4, 10, false, true},   // 302 with 10 waves (retired)
    {308, 4, 8, true, true},     // 302 with 766-frame blocks
    {310, 8, 8, false, true},    // the slicing-by-8 fold
    {312, 9, 8, false, true},    // the slicing-by-8 fold with the boundary correction deferred
    {314, 10, 8, false, true},   // the slicing-by-8 fold with the boundary word patched per half
    {316, 11, 8, false, true},   // 314 with each half folded as two chains of four units
    {318, 12, 8, false, true},   // 314 with 190-frame blocks
    {320, 13, 8, false, true},   // 314 with 254-frame blocks
    {322, 14, 8, false, true},   // 314 with the next block's offsets loaded ahead
    {324, 15, 8, false, true},   // 314 with 510-frame blocks
    {326, 16, 8, false, true},   // 314 with 6 waves
    // timing only (wrong results; round 5)
    {328, 17, 8, false, false},  // 314 without the transpose writes
    {330, 18, 8, false, false},  // 314 with a two-op stand-in for the lookups
    {332, 19, 8, false, false},  // 314 without the ending frames' capture and Z_c
    {334, 20, 8, false, false},  // 314 without the carries
    {340, 21, 8, false, false},  // the ring's loads alone
    {342, 22, 8, false, false},  // loads + the LDS transpose
};
constexpr const StageVariant* stage_variant(int id) {
  for (const StageVariant& v : kStageVariants)
    if (id == v.id || (v.verify && id == v.id + 1)) return &v;
  return nullptr;
}
}
// crc32_kernel.hip
hipError_t launch_crc32_variant(int var, const uint8_t* bytes, const uint64_t* off, uint64_t n, void* out,
                                const void* images, int num_cus, hipStream_t stream, uint64_t* timeline);
uint64_t crc32_launch_waves(uint64_t n, int num_cus);
hipError_t launch_fcs_scatter(uint8_t* bytes, const uint64_t* start, uint32_t* len, const uint32_t* crc, uint64_t n,
                              uint32_t capacity, uint8_t* status, int num_cus, hipStream_t stream);
#endif

}  // namespace lnx
