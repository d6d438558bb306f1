// deliver_plan.hpp — the step of lneto's receive path that follows the
// checksum-stage verdict (frame_plan.hpp): which handler a frame is handed to.
// Once, for the kernel that decides it per frame (deliver_kernel.hip), the
// per-frame host function (deliver_host.cpp: lnx_rx_deliver) and the CPU test
// program that runs the same code under sanitizers
// (tests/cpp/deliver_plan_host.cpp).
//
// Plain C++17 in the style of frame_plan.hpp: no intrinsics, no thread indices
// and no memory access of its own.  The caller supplies the frame's fields
// through callables,
//   be16(o)  the big-endian 16-bit field at frame offset o
//   byt(o)   the byte at frame offset o
// and looks the destination port up in its own copy of the port table between
// dlv_parse and dlv_finish.  An accessor is called only once o + size <= L is
// known, whatever the incoming verdict claims: memory safety rests on L alone.
//
// The rules, in the reference's order:
//  1. an FCS result of 0 ends the frame: ErrBadCRC (3), flag kDlvFcs;
//  2. a non-zero receive verdict is passed through, not delivered;
//  3. an EtherType other than IPv4 / IPv6 goes to the StackEthernet handler
//     registered for it (handlers.demuxByProto, internet/stack-ethernet.go:158-161,
//     internet/definitions.go:98-106,128-139: first match): kHEth + its index
//     in the filter's EtherTypes, kHEth + 8 for the accept-all filter;
//  4. IPv4 (demux4, internet/stack-ip4.go:135-170): the handler of the protocol
//     is called with frame[14 : 14 + total length] and offset 4 IHL; IPv6
//     (demux6, internet/stack-ip6.go:107-138) with frame[14 : 54 + payload
//     length] and offset 40.  A protocol other than TCP / UDP: kHIp4 / kHIp6 +
//     protocol;
//  5. TCP / UDP: that handler is StackPorts.Demux (internet/stack-ports.go:64-84)
//     with dstPortOff 2 (ResetTCP / ResetUDP, :25-31).  P = the bytes from the
//     transport header to the end of the IP packet.
//       P < 4: io.ErrShortBuffer (:65-67), the library's 6;
//       else the port at +2 is looked up by handlers.demuxByPort -> nodeByPort
//       (internet/definitions.go:108-116,141-152): the first node with that
//       local port, kHTcp / kHUdp + its index; none: ErrPacketDrop (2), and for
//       TCP with P >= 14 a SYN without RST / ACK (flags = be16(+12) & 0x1ff)
//       queues a RST (:70-82) unless internal.GetIPAddr fails, which it does
//       only for a version nibble other than 4 or 6 (internal/ip.go:9-27;
//       demux6 never looks at the nibble): flag kDlvRst;
//  6. a field a rule needs that lies at or past L, or an IP packet that ends
//     past L (the slice the reference hands down would not exist), can only
//     come from a verdict that does not belong to these bytes: ErrTruncatedFrame
//     (18), every other field of the record 0.
#pragma once
#include <cstdint>
#include "rx_filter.hpp"
#include "wave_util.hpp"

namespace lnxd {

using lnx::RxFilter;

constexpr uint32_t kHEth = LNX_H_ETH, kHIp4 = LNX_H_IP4, kHIp6 = LNX_H_IP6, kHTcp = LNX_H_TCP, kHUdp = LNX_H_UDP,
                   kHCount = LNX_H_COUNT, kHNone = LNX_H_NONE;
static_assert(kHEth + 9 <= kHIp4 && kHIp4 + 256 == kHIp6 && kHIp6 + 256 == kHTcp && kHTcp + 257 <= kHUdp &&
              kHUdp + 257 == kHCount, "handler ids: disjoint ranges");
constexpr uint32_t kDlvRst = LNX_DLV_RST, kDlvIp6 = LNX_DLV_IP6, kDlvFcs = LNX_DLV_FCS;
// lneto errors.go:6-28; 6 is the number the library uses for io.ErrShortBuffer (lnx_fcs_append)
constexpr uint32_t kDropped = 2, kBadCRC = 3, kShortBuffer = 6, kTruncated = 18;
constexpr uint32_t kPortsMax = 256;

// the port tables as a kernel argument (on = 0: no tables, every port has a handler)
struct DlvPorts {
  uint32_t on, n_tcp, n_udp;
  uint16_t tcp[kPortsMax], udp[kPortsMax];
};
// ports NULL: no tables
inline DlvPorts dlv_ports_of(const lnx_rx_ports* ports) {
  DlvPorts pt{};
  if (ports) {
    pt.on = 1, pt.n_tcp = ports->n_tcp, pt.n_udp = ports->n_udp;
    for (uint32_t i = 0; i < kPortsMax; ++i) pt.tcp[i] = ports->tcp[i], pt.udp[i] = ports->udp[i];
  }
  return pt;
}

struct DlvPlan {
  uint32_t ip_end = 0, handler = kHNone, l4_off = 0, src_port = 0, dst_port = 0, verdict = 0, flags = 0;
  uint32_t lookup = 0;  // 6 / 17: dst_port is to be looked up in the TCP / UDP table (dlv_finish); 0: decided
  uint32_t rst = 0;     // kDlvRst when a miss of that lookup queues a RST
};

// fcs < 0: no FCS result.  L: the frame's bytes without its FCS.
template <class Be16, class Byte>
LNX_HD DlvPlan dlv_parse(uint32_t L, uint32_t v_in, int32_t fcs, const RxFilter& filt, Be16 be16, Byte byt) {
  DlvPlan r;
  if (fcs == 0) {  // rule 1
    r.verdict = kBadCRC, r.flags = kDlvFcs;
    return r;
  }
  if (v_in != 0) {  // rule 2
    r.verdict = v_in;
    return r;
  }
  DlvPlan cut;  // rule 6
  cut.verdict = kTruncated;
  if (L < 14) return cut;
  const uint32_t et = be16(12);
  if (et != 0x0800 && et != 0x86DD) {  // rule 3
    if (!filt.on) {
      r.handler = kHEth + 8;
      return r;
    }
    uint32_t slot = 8;
#pragma unroll
    for (int i = 7; i >= 0; --i) slot = (i < (int)filt.n_et && filt.et[i] == et) ? (uint32_t)i : slot;
    if (slot == 8) r.verdict = kDropped;  // no handler: a zero verdict the filter would not have given
    else r.handler = kHEth + slot;
    return r;
  }
  uint32_t proto;
  if (et == 0x0800) {  // rule 4
    if (L < 24) return cut;  // version / IHL at 14, total length at 16, protocol at 23
    r.l4_off = 14 + 4 * (byt(14) & 15u);
    r.ip_end = 14 + be16(16);
    proto = byt(23);
  } else {
    if (L < 21) return cut;  // payload length at 18, next header at 20
    r.l4_off = 54;
    r.ip_end = 54 + be16(18);
    proto = byt(20);
    r.flags = kDlvIp6;
  }
  if (r.ip_end > L) return cut;
  if (proto != 6 && proto != 17) {
    r.handler = (et == 0x0800 ? kHIp4 : kHIp6) + proto;
    return r;
  }
  // rule 5
  const int32_t P = (int32_t)r.ip_end - (int32_t)r.l4_off;
  if (P < 4) {
    r.verdict = kShortBuffer;
    return r;
  }
  // l4_off + 4 <= ip_end <= L
  r.src_port = be16(r.l4_off);
  r.dst_port = be16(r.l4_off + 2);
  r.lookup = proto;
  if (proto == 6 && P >= 14) {  // l4_off + 14 <= ip_end <= L; byte 14 < 24 <= L
    const uint32_t fl = be16(r.l4_off + 12) & 0x1FFu, ver = byt(14) >> 4;
    if ((fl & 0x02u) != 0 && (fl & 0x14u) == 0 && (ver == 4 || ver == 6)) r.rst = kDlvRst;
  }
  return r;
}

// k: the index of the first table entry equal to dst_port, -1 for none, 256
// without a table (every port has a handler).  Ignored unless r.lookup.
LNX_HD void dlv_finish(DlvPlan& r, int32_t k) {
  if (r.lookup == 0) return;
  if (k >= 0) {
    r.handler = (r.lookup == 6 ? kHTcp : kHUdp) + (uint32_t)k;
  } else {
    r.verdict = kDropped;
    r.flags |= r.rst;
  }
}

// lnx_rx_delivery as four little-endian words
LNX_HD void dlv_pack(const DlvPlan& r, uint32_t (&w)[4]) {
  w[0] = r.ip_end;
  w[1] = (r.handler & 0xFFFFu) | (r.l4_off << 16);
  w[2] = r.src_port | (r.dst_port << 16);
  w[3] = (r.verdict & 0xFFu) | (r.flags << 8);
}

// the grouping's bucket: the handler id, kHCount for a frame not delivered
LNX_HD uint32_t dlv_bucket(const DlvPlan& r) { return r.handler == kHNone ? kHCount : r.handler; }

}  // namespace lnxd
