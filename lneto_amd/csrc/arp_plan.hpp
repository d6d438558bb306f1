// arp_plan.hpp — what arp.Handler (IPv4 over Ethernet: HardwareType 1,
// ProtocolType 0x0800, a 6-byte HardwareAddr, a 4-byte ProtocolAddr, registered
// on StackEthernet at frame offset 0) does with a frame, and the frame it sends
// back.  Once, for the kernels (arp_kernel.hip), the per-frame host functions
// (arp_host.cpp: lnx_rx_arp_entry, lnx_arp_frame) and the CPU test program that
// runs the same code under sanitizers (tests/cpp/arp_plan_host.cpp).
//
// Plain C++17 in the style of reply_plan.hpp: no intrinsics, no thread indices
// and no memory access of its own.  The caller supplies the frame's fields
// through callables,
//   byt(o)   the byte at frame offset o
//   be16(o)  the big-endian 16-bit field at frame offset o
// and an accessor is called only once o + size <= L is known, whatever the
// record claims: the records are the caller's memory and may be stale, so
// memory safety rests on L (the frame's bytes without its FCS) alone.
//
// Which frame reaches the handler: the delivery record has
// verdict 0 and a handler id LNX_H_ETH .. LNX_H_ETH + 8, L >= 14 and
// be16(12) == 0x0806.  Rule 3 of deliver_plan.hpp maps the EtherType to that
// handler, so under a zero verdict the four together mean the ARP handler is
// the one called; a VLAN-tagged frame (0x8100) goes to another handler.
//
// Handler.Demux on b = frame[14:L], P = L - 14 (arp/handler.go:160-203); the
// verdict numbers are errors.go's:
//  1. P < 28: ErrTruncatedFrame, 18 (NewFrame, arp/frame.go:17-22);
//  2. hlen = b[4], ilen = b[5], minLen = 8 + 2 (hlen + ilen); P < minLen: 18
//     (errShortARP), else minLen > 255: ErrPacketDrop, 2 (errLargeSizes)
//     (ValidateSize, arp/frame.go:137-146; handler.go:166-169), before any type check;
//  3. be16(b[0]) != 1 or hlen != 6: ErrMismatch, 10 (handler.go:170-173);
//  4. be16(b[2]) != 0x0800 or ilen != 4: 10 (handler.go:174-177);
//  5. op = be16(b[6]) (handler.go:178-201):
//     op 1: b[24:28] is not our address: verdict 0, nothing happens (:180-183);
//           else the frame queues a reply entry {hw = b[8:14], ip = b[14:18]},
//           the sender (:184-186).  Nothing about the sender is filtered;
//     op 2: the frame yields a learn record {hw = b[8:14], ip = b[14:18]}
//           (:189).  cache.Lookup on it (:190) is host state and stays there;
//           the target fields are not looked at;
//     else: errARPUnsupported, 9 (:199-200).
//
// The frame an entry becomes: Handler.Encapsulate (handler.go:126-158),
// entry.put (cache.go:32-71) and StackEthernet.Encapsulate
// (internet/stack-ethernet.go:170-217).  All 60 bytes are the reference's:
//   0-5    the entry's hw: StackEthernet first writes the gateway MAC
//          (stack-ethernet.go:184), then trySetEthernetDst overwrites it with the
//          ARP body's target hardware address (handler.go:153-155, 215-219),
//          which put has just set to the entry's hw (cache.go:65-66)
//   6-11   our MAC (stack-ethernet.go:197)      12-13  0x0806 (:198)
//   14-21  00 01 08 00 06 04 00 02 (cache.go:40-41, 61)
//   22-27, 28-31  our MAC, our address (cache.go:62-64)
//   32-37, 38-41  the entry's hw, the entry's ip (cache.go:65-67)
//   42-59  the padding to 60 bytes (stack-ethernet.go:203-207)
// and, with a CRC (stack-ethernet.go:211-215), LE32(CRC32(the 60 bytes)) at
// 60..63; without, the slot's last dword is 0 and the frame is 60 bytes long.
// A query (StartQuery, handler.go:112-124, op 1) differs in two places: the
// destination is ff:ff:ff:ff:ff:ff (handler.go:150-152) and bytes 20-21 are
// 00 01; the entry's hw (which StartQuery leaves zero) goes to 32-37 as it is.
//
// ASSUMPTION: our MAC stands for both the Ethernet source and the ARP sender.
// The reference takes the first from StackEthernet and the second from
// HandlerConfig.HardwareAddr, two settings that a working stack keeps equal.
//
// NOT restated: the cache's size, eviction and ageing (acquireNext), one frame
// per Encapsulate call, cache.Lookup on a learn record and the resolve
// callback.  The batch form answers every queueing frame and emits every learn
// record, in arrival order, up to the caller's capacities, and reports what it
// left out.
#pragma once
#include <cstdint>
#include "../../include/lneto_amd.h"
#include "slot_frame.hpp"
#include "wave_util.hpp"

namespace lnxa {

constexpr uint32_t kArpNone = 0, kArpRequest = 1, kArpReply = 2;  // a frame's kind; the two ops (arp/definitions.go)
constexpr uint32_t kErrDrop = 2, kErrUnsupported = 9, kErrMismatch = 10, kErrTruncated = 18;  // errors.go
constexpr uint32_t kEtherArp = 0x0806, kArpBody = 14, kArpV4 = 28, kArpMinL = kArpBody + kArpV4;

// the stack's side, as the bytes lie in memory: mac[0..1], mac[2..5] and ip4 as little-endian words
struct ArpCfg {
  uint32_t m01, m2345, ip;
  uint32_t fcs;  // LNX_TX_FCS given
};
inline ArpCfg arp_cfg_of(const lnx_rst_cfg& c) {
  ArpCfg r{};
  r.m01 = c.mac[0] | ((uint32_t)c.mac[1] << 8);
  r.m2345 = c.mac[2] | ((uint32_t)c.mac[3] << 8) | ((uint32_t)c.mac[4] << 16) | ((uint32_t)c.mac[5] << 24);
  r.ip = c.ip4[0] | ((uint32_t)c.ip4[1] << 8) | ((uint32_t)c.ip4[2] << 16) | ((uint32_t)c.ip4[3] << 24);
  r.fcs = (c.flags & LNX_TX_FCS) != 0;
  return r;
}

// lnx_arp_entry as its three little-endian dwords: hw[0..3]; hw[4..5] (the upper half zero); ip[0..3]
struct ArpEntry {
  uint32_t d0 = 0, d1 = 0, d2 = 0;
};

// Does the frame under this record reach the ARP handler?  Reads bytes 12..13 only, and only of a frame it may reach.
template <class Be16>
LNX_HD bool arp_reaches(uint32_t L, uint32_t rec_verdict, uint32_t rec_handler, Be16 be16) {
  if (rec_verdict != 0 || rec_handler < LNX_H_ETH || rec_handler > LNX_H_ETH + 8u) return false;
  if (L < kArpBody) return false;
  return be16(12) == kEtherArp;
}

// Handler.Demux (rules 1-5) of a frame that reaches it: its kind, and the error number in `verdict`.
// Every byte read lies below 14 + 28 <= L.
template <class Byte>
LNX_HD uint32_t arp_demux(uint32_t L, const ArpCfg& c, Byte byt, uint32_t& verdict) {
  auto be16 = [&](uint32_t o) -> uint32_t { return (byt(kArpBody + o) << 8) | byt(kArpBody + o + 1u); };
  const uint32_t P = L - kArpBody;
  verdict = kErrTruncated;
  if (P < kArpV4) return kArpNone;                                     // 1
  const uint32_t hlen = byt(kArpBody + 4u), ilen = byt(kArpBody + 5u);
  const uint32_t min_len = 8u + 2u * (hlen + ilen);
  if (P < min_len) return kArpNone;                                    // 2
  verdict = kErrDrop;
  if (min_len > 255u) return kArpNone;
  verdict = kErrMismatch;
  if (be16(0) != 1u || hlen != 6u) return kArpNone;                    // 3
  if (be16(2) != 0x0800u || ilen != 4u) return kArpNone;               // 4
  const uint32_t op = be16(6);                                         // 5
  verdict = kErrUnsupported;
  if (op != kArpRequest && op != kArpReply) return kArpNone;
  verdict = 0;
  if (op == kArpReply) return kArpReply;
  const uint32_t target = byt(kArpBody + 24u) | (byt(kArpBody + 25u) << 8) | (byt(kArpBody + 26u) << 16) | (byt(kArpBody + 27u) << 24);
  return target == c.ip ? kArpRequest : kArpNone;
}

// the sender of a frame of kind 1 or 2: b[8:14] and b[14:18]
template <class Byte>
LNX_HD ArpEntry arp_entry_of(Byte byt) {
  auto b = [&](uint32_t o) -> uint32_t { return byt(kArpBody + o); };
  ArpEntry e;
  e.d0 = b(8) | (b(9) << 8) | (b(10) << 16) | (b(11) << 24);
  e.d1 = b(12) | (b(13) << 8);
  e.d2 = b(14) | (b(15) << 8) | (b(16) << 16) | (b(17) << 24);
  return e;
}

LNX_HD bool arp_op_ok(uint32_t op) { return op == kArpRequest || op == kArpReply; }

// dword p < 15 of the frame as it lies in memory: the part the stack's configuration decides ...
LNX_HD uint32_t arp_fixed_word(uint32_t p, const ArpCfg& c) {
  return p == 1 || p == 5 ? c.m01 << 16 : p == 2 || p == 6 ? c.m2345 : p == 3 ? 0x01000608u : p == 4 ? 0x04060008u
       : p == 7 ? c.ip : 0u;
}
// ... and the part the entry and the op decide (0 where the other part stands); op: 1 or 2
LNX_HD uint32_t arp_var_word(uint32_t p, const ArpEntry& e, uint32_t op) {
  const bool query = op == kArpRequest;
  return p == 0 ? (query ? 0xFFFFFFFFu : e.d0) : p == 1 ? (query ? 0xFFFFu : e.d1 & 0xFFFFu) : p == 5 ? (op & 0xFFu) << 8
       : p == 8 ? e.d0 : p == 9 ? (e.d1 & 0xFFFFu) | (e.d2 << 16) : p == 10 ? e.d2 >> 16 : 0u;
}
// fixed = arp_fixed_word(p, cfg)
LNX_HD uint32_t arp_word(uint32_t p, uint32_t fixed, const ArpEntry& e, uint32_t op) { return fixed | arp_var_word(p, e, op); }

// The frame in its slot and its FCS: slot_frame.hpp, over the kRstImgZ tables.

}  // namespace lnxa
