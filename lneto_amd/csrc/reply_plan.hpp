// reply_plan.hpp — the second side effect of StackPorts.Demux for a TCP SYN to
// a port nobody listens on (internet/stack-ports.go:64-84): beside returning
// ErrPacketDrop it queues a RST, and the next Encapsulate turns the queue's
// entry into a frame.  Once, for the kernels (reply_kernel.hip), the per-frame
// host functions (reply_host.cpp: lnx_rx_rst_entry, lnx_tcp_rst_frame,
// lnx_ip4_id_chain) and the CPU test program that runs the same code under
// sanitizers (tests/cpp/reply_plan_host.cpp).
//
// Plain C++17 in the style of deliver_plan.hpp: no intrinsics, no thread indices
// and no memory access of its own.  The caller supplies the frame's fields
// through callables,
//   byt(o)   the byte at frame offset o
//   be32(o)  the big-endian 32-bit field at frame offset o
// and an accessor is called only once o + size <= L is known, whatever the
// record claims: the records are the caller's memory and may be stale, so
// memory safety rests on L (the frame's bytes without its FCS) alone.
//
// The entry a frame queues:
//  1. the delivery record carries kDlvRst (deliver_plan.hpp rule 5: a TCP miss
//     whose flags are SYN without RST / ACK, stack-ports.go:70-74);
//  2. the version nibble of byte 14 is 4.  RSTQueue.Queue keeps 4-byte
//     addresses only (tcp/rst.go:22-33); internal.GetIPAddr hands it buf[12:16]
//     for nibble 4 and the 16-byte buf[8:24] for nibble 6 (internal/ip.go:9-27),
//     which Queue drops in silence.  demux6 never looks at the nibble, so a
//     frame with EtherType 0x86DD and nibble 4 does queue an entry, with the
//     IPv4 offsets: restated as it is;
//  3. a frame with L < 30 or a record with l4_off + 8 > L queues nothing (no
//     such pair comes from the delivery rules; nothing past L is read);
//  4. the entry (stack-ports.go:75-80): remote address = bytes 26..29, remote
//     port = the record's src_port, local port = its dst_port, seq 0,
//     ack = be32(l4_off + 4) + 1 mod 2^32, flags RST|ACK.
//
// The frame an entry becomes: RSTQueue.Drain (tcp/rst.go:38-63) inside
// encapsulate4 (internet/stack-ip4.go:178-231) inside StackEthernet.Encapsulate
// (internet/stack-ethernet.go:170-217).  The reference writes all 54 header
// bytes, so nothing depends on what the carrier buffer held.  As thirty
// big-endian 16-bit fields, field k at bytes 2k, 2k + 1:
//   0-2   gateway MAC (stack-ethernet.go:184)      3-5  our MAC (:197)
//   6     0x0800 (:198)
//   7     0x4500: version 4, IHL 5, ToS 0 (stack-ip4.go:187-188)
//   8     40: total length (:203-204)              9    the ID (:189-191)
//   10    0x4000: don't fragment (:192)            11   0x4006: TTL 64 (:193), protocol TCP (:205)
//   12    CalculateHeaderCRC (:207-209)            13-14 our address (:194)
//   15-16 the entry's remote address (rst.go:58)   17   source port = local port (rst.go:50)
//   18    destination port = remote port (:51)     19-22 seq, ack (:52-56)
//   23    offset 5 << 12 | flags & 0x1ff (SetOffsetAndFlags, tcp/frame.go:92-95)
//   24    window 0 (SetSegment, tcp/frame.go:153)  25   CRCWriteTCPPseudo + PayloadSum16 (stack-ip4.go:215-220)
//   26    urgent pointer 0 (rst.go:57)             27-29 the padding to 60 bytes (stack-ethernet.go:203-207)
// and, with a CRC (stack-ethernet.go:211-215), LE32(CRC32(the 60 bytes)) at
// 60..63; without, the slot's last dword is 0 and the frame is 60 bytes long.
//
// The IP ID (stack-ip4.go:189-195): id' = Prand16((id + 1) ^ ip4[0])
// (internal/prand.go:4-10), serial by nature and the caller's stack state; the
// batch entries take the IDs as data.
//
// NOT restated: RSTQueue holds four entries, drops the rest and drains last-in
// first-out, one per Encapsulate call (tcp/rst.go:8,23,44-45).  That bound
// belongs to the queue, not to the frames: the batch form makes the reply of
// EVERY queueing frame, in arrival order, up to the caller's capacity, and
// reports how many it left out.
#pragma once
#include <cstdint>
#include "../../include/lneto_amd.h"
#include "slot_frame.hpp"
#include "wave_util.hpp"

namespace lnxr {

constexpr uint32_t kDlvRst = LNX_DLV_RST;
constexpr uint32_t kTcpRst = 0x04u, kTcpAck = 0x10u, kTcpFlagMask = 0x1FFu;  // tcp/definitions.go:158-168

// the stack's side of a reply: 16-bit big-endian fields
struct RstCfg {
  uint32_t gw[3], mac[3], ip[2];
  uint32_t fcs;  // LNX_TX_FCS given
};
inline RstCfg rst_cfg_of(const lnx_rst_cfg& c) {
  RstCfg r{};
  for (uint32_t i = 0; i < 3; ++i) {
    r.gw[i] = ((uint32_t)c.gw_mac[2 * i] << 8) | c.gw_mac[2 * i + 1];
    r.mac[i] = ((uint32_t)c.mac[2 * i] << 8) | c.mac[2 * i + 1];
  }
  for (uint32_t i = 0; i < 2; ++i) r.ip[i] = ((uint32_t)c.ip4[2 * i] << 8) | c.ip4[2 * i + 1];
  r.fcs = (c.flags & LNX_TX_FCS) != 0;
  return r;
}

// rstEntry (tcp/rst.go:12-19); addr: the four address bytes as a big-endian number
struct RstEntry {
  uint32_t addr = 0, remote_port = 0, local_port = 0, seq = 0, ack = 0, flags = 0;
};

// rules 1-3: does the frame under this record queue an entry?  Reads byte 14 only, and only of a flagged frame.
template <class Byte>
LNX_HD bool rst_queues(uint32_t L, uint32_t rec_flags, uint32_t l4_off, Byte byt) {
  if ((rec_flags & kDlvRst) == 0) return false;
  if (L < 30 || l4_off + 8 > L) return false;  // bytes 26..29 and l4_off + 4 .. l4_off + 7 lie below L
  return (byt(14) >> 4) == 4;
}

// rule 4, for a frame that queues
template <class Be32>
LNX_HD RstEntry rst_entry_of(uint32_t l4_off, uint32_t src_port, uint32_t dst_port, Be32 be32) {
  RstEntry e;
  e.addr = be32(26);
  e.remote_port = src_port & 0xFFFFu;
  e.local_port = dst_port & 0xFFFFu;
  e.seq = 0;
  e.ack = be32(l4_off + 4) + 1u;
  e.flags = kTcpRst | kTcpAck;
  return e;
}

// internal/prand.go:4-10 on 16 bits, and the chain's step (stack-ip4.go:189-195)
LNX_HD uint32_t prand16(uint32_t seed) {
  seed &= 0xFFFFu;
  seed ^= (seed << 7) & 0xFFFFu;
  seed ^= seed >> 9;
  seed ^= (seed << 8) & 0xFFFFu;
  return seed;
}
LNX_HD uint32_t ip4_id_next(uint32_t id, uint32_t ip4_first) { return prand16(((id + 1u) & 0xFFFFu) ^ (ip4_first & 0xFFu)); }

// CalculateHeaderCRC over fields 7..16 with field 12 zero
LNX_HD uint32_t rst_ip_sum(const RstCfg& c, const RstEntry& e, uint32_t id) {
  const uint32_t s = 0x4500u + 40u + (id & 0xFFFFu) + 0x4000u + 0x4006u + c.ip[0] + c.ip[1] + (e.addr >> 16) + (e.addr & 0xFFFFu);
  return lnx::fold_sum16(s);
}
// the pseudo-header (both addresses, protocol 6, TCP length 20), then fields 17..26 with field 25 zero
LNX_HD uint32_t rst_tcp_sum(const RstCfg& c, const RstEntry& e) {
  const uint32_t s = c.ip[0] + c.ip[1] + (e.addr >> 16) + (e.addr & 0xFFFFu) + 6u + 20u + e.local_port + e.remote_port +
                     (e.seq >> 16) + (e.seq & 0xFFFFu) + (e.ack >> 16) + (e.ack & 0xFFFFu) + (0x5000u | (e.flags & kTcpFlagMask));
  return lnx::fold_sum16(s);
}

// field k of the frame: the part the stack's configuration decides ...
LNX_HD uint32_t rst_fixed_field(uint32_t k, const RstCfg& c) {
  return k < 3 ? c.gw[k] : k < 6 ? c.mac[k - 3] : k == 6 ? 0x0800u : k == 7 ? 0x4500u : k == 8 ? 40u : k == 10 ? 0x4000u
       : k == 11 ? 0x4006u : k == 13 ? c.ip[0] : k == 14 ? c.ip[1] : 0u;
}
// ... and the part the entry, the ID and the two sums decide (0 where the other part stands)
LNX_HD uint32_t rst_var_field(uint32_t k, const RstEntry& e, uint32_t id, uint32_t ip_sum, uint32_t tcp_sum) {
  return k == 9 ? (id & 0xFFFFu) : k == 12 ? ip_sum : k == 15 ? (e.addr >> 16) : k == 16 ? (e.addr & 0xFFFFu)
       : k == 17 ? e.local_port : k == 18 ? e.remote_port : k == 19 ? (e.seq >> 16) : k == 20 ? (e.seq & 0xFFFFu)
       : k == 21 ? (e.ack >> 16) : k == 22 ? (e.ack & 0xFFFFu) : k == 23 ? (0x5000u | (e.flags & kTcpFlagMask))
       : k == 25 ? tcp_sum : 0u;
}
// dword p < 15 of the frame as it lies in memory (slot_frame.hpp slot_pack): the first part ...
LNX_HD uint32_t rst_fixed_word(uint32_t p, const RstCfg& c) { return lnx::slot_pack(rst_fixed_field(2 * p, c), rst_fixed_field(2 * p + 1, c)); }
// ... and the whole: fixed = rst_fixed_word(p, cfg)
LNX_HD uint32_t rst_word(uint32_t p, uint32_t fixed, const RstEntry& e, uint32_t id, uint32_t ip_sum, uint32_t tcp_sum) {
  return fixed | lnx::slot_pack(rst_var_field(2 * p, e, id, ip_sum, tcp_sum), rst_var_field(2 * p + 1, e, id, ip_sum, tcp_sum));
}

// The frame in its slot and its FCS: slot_frame.hpp, over the kRstImgZ tables.

}  // namespace lnxr
