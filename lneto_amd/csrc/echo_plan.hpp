// echo_plan.hpp — the other frame the stack sends back on its own: the echo
// reply of an ICMPv4 echo request.  icmpv4.Client.Demux stores the request's
// identifier, sequence number, source address and data
// (ipv4/icmpv4/client.go:111-132), and the next Encapsulate turns that into an
// echo reply (client.go:162-176, 209-218).  Once, for the kernels
// (echo_kernel.hip), the per-frame host functions (echo_host.cpp:
// lnx_rx_echo_entry, lnx_icmp_echo_reply_frame) and the CPU test program that
// runs the same code under sanitizers (tests/cpp/echo_plan_host.cpp).
//
// Plain C++17 in the style of reply_plan.hpp: no intrinsics, no thread indices
// and no memory access of its own.  The caller supplies the frame's fields
// through callables,
//   byt(o)   the byte at frame offset o
//   be16(o)  the big-endian 16-bit field at frame offset o
//   be32(o)  the big-endian 32-bit field at frame offset o
// and an accessor is called only once o + size <= L is known, whatever the
// record claims: the records are the caller's memory and may be stale, so
// memory safety rests on L (the frame's bytes without its FCS) alone.
//
// Which frame queues a reply:
//  1. its delivery record has verdict 0 and handler LNX_H_IP4 + 1 (demux4 hands
//     protocol 1 to the ICMP client, internet/stack-ip4.go:134-141, 168-170);
//  2. with l4 = rec.l4_off and end = rec.ip_end: 34 <= l4, l4 + 9 <= end and
//     end <= L.  l4 + 8 > end is NewFrame's ErrTruncatedFrame
//     (ipv4/icmpv4/icmpv4.go:62-67); l4 + 8 == end is len(data) == 0, which gives
//     ErrPacketDrop (client.go:119-122).  Anything else that fails these bounds
//     comes only from a record that does not belong to these bytes: it queues
//     nothing and nothing past L is read.  For the same reason a record with
//     end - l4 - 8 > 65507 queues nothing: an IPv4 packet's 16-bit total length
//     allows no more data, and the reply's total length is 28 + d;
//  3. byt(l4) == 8.  An echo reply (type 0) updates host state and sends
//     nothing; other types are dropped (client.go:95-98);
//  4. the version nibble of byte 14 is 4.  demux4 guarantees it under a zero
//     verdict (ipv4/frame.go:229-234).  A stale record over a frame with another
//     nibble queues nothing here; the reference (internal.GetIPAddr failing,
//     client.go:104-110) would answer such a frame to 0.0.0.0, which is
//     deliberately NOT restated;
//  5. the entry: remote address = bytes 26..29, id = be16(l4 + 4),
//     seq = be16(l4 + 6), data = frame[l4 + 8 : end].  The request's code byte is
//     discarded (Encapsulate sets code 0, client.go:210).
// The request's ICMP checksum (client.go:99-102) is the verdict's business under
// LNX_VERIFY_ICMP, as the FCS is: the entry does not check it again.
//
// The frame an entry becomes: Client.Encapsulate (client.go:154-219) inside
// encapsulate4 (internet/stack-ip4.go:178-231) inside StackEthernet.Encapsulate
// (internet/stack-ethernet.go:170-217).  With d = the data length, as twenty-one
// big-endian 16-bit fields, field k at bytes 2k, 2k + 1, then the data:
//   0-2   gateway MAC (stack-ethernet.go:184)      3-5  our MAC (:197)
//   6     0x0800 (:198)
//   7     0x4500: version 4, IHL 5, ToS 0 (stack-ip4.go:187-188)
//   8     28 + d: total length (:203-204)          9    the IP ID (:189-191)
//   10    0x4000: don't fragment (:192)            11   0x4001: TTL 64 (:193), protocol ICMP (:205)
//   12    CalculateHeaderCRC (:207-209)            13-14 our address (:194)
//   15-16 the entry's remote address (client.go:216)
//   17    type 0, code 0 (client.go:166, 210)
//   18    PayloadSum16 over bytes 34 .. 42 + d with this field zero (client.go:211-214)
//   19    id (client.go:167)                       20   seq (:168)
//   bytes 42 .. 42 + d: the data (:170); zero padding to 60 bytes
//   (stack-ethernet.go:203-207); with a CRC (:211-215) LE32(CRC32(all before it)).
// encapsulate4 adds no transport sum for ICMP (stack-ip4.go:213-229 covers TCP
// and UDP only).  The checksum is taken fresh over the reply's bytes: an RFC 1624
// update of the request's checksum is wrong here, since for a request whose id,
// seq and data are all zero it yields 0x0000 where PayloadSum16 gives 0xFFFF.
//
// NOT restated: incomingEcho's capacity and ErrExhausted (client.go:113-116), the
// response ring's size (:123-127), one reply per Encapsulate call and the MTU
// clip of the carrier buffer.  Those bounds belong to the queue, not to the
// frames: the batch form answers EVERY queueing frame, in arrival order, up to
// the caller's capacities, and reports what it left out.
#pragma once
#include <cstdint>
#include "../../include/lneto_amd.h"
#include "reply_plan.hpp"
#include "slot_frame.hpp"
#include "wave_util.hpp"

namespace lnxe {

using lnxr::RstCfg;  // the stack's side of any reply

constexpr uint32_t kHandlerIcmp4 = LNX_H_IP4 + 1u;
constexpr uint32_t kTypeEcho = 8, kTypeEchoReply = 0;  // ipv4/icmpv4/definitions
constexpr uint32_t kEchoHdr = 42, kEchoHdrWords = 10, kEchoPadded = 60, kEchoMaxData = 65507;
constexpr uint32_t kEchoMinL4 = 34;

struct EchoEntry {
  uint32_t addr = 0, id = 0, seq = 0, data_off = 0, data_len = 0;  // addr: the four address bytes as a big-endian number
};

// rules 1-4: reads bytes l4 and 14 only, and only of a frame whose record passes rules 1-2
template <class Byte>
LNX_HD bool echo_queues(uint32_t L, uint32_t verdict, uint32_t handler, uint32_t l4, uint32_t end, Byte byt) {
  if (verdict != 0 || handler != kHandlerIcmp4) return false;
  if (l4 < kEchoMinL4 || end > L || end < l4 + 9u || end - l4 - 8u > kEchoMaxData) return false;  // (l4 < 2^16: no wrap)
  if (byt(l4) != kTypeEcho) return false;
  return (byt(14) >> 4) == 4;
}

// rule 5, for a frame that queues
template <class Be16, class Be32>
LNX_HD EchoEntry echo_entry_of(uint32_t l4, uint32_t end, Be16 be16, Be32 be32) {
  EchoEntry e;
  e.addr = be32(26);
  e.id = be16(l4 + 4);
  e.seq = be16(l4 + 6);
  e.data_off = l4 + 8u;
  e.data_len = end - l4 - 8u;
  return e;
}

// the reply's length without its FCS, with it, and the 64-byte blocks it takes in a batch
LNX_HD uint32_t echo_padded(uint32_t d) { return kEchoHdr + d < kEchoPadded ? kEchoPadded : kEchoHdr + d; }
LNX_HD uint32_t echo_len(uint32_t d, uint32_t fcs) { return echo_padded(d) + (fcs ? 4u : 0u); }
LNX_HD uint32_t echo_blocks(uint32_t d, uint32_t fcs) { return (echo_len(d, fcs) + 63u) / 64u; }

// CalculateHeaderCRC over fields 7..16 with field 12 zero
LNX_HD uint32_t echo_ip_sum(const RstCfg& c, uint32_t addr, uint32_t d, uint32_t ip_id) {
  const uint32_t s = 0x4500u + (28u + d) + (ip_id & 0xFFFFu) + 0x4000u + 0x4001u + c.ip[0] + c.ip[1] + (addr >> 16) + (addr & 0xFFFFu);
  return lnx::fold_sum16(s);
}
// PayloadSum16 over the ICMP message from the plain sum of its big-endian 16-bit words (an odd last byte << 8)
LNX_HD uint32_t echo_icmp_sum(uint32_t be_sum) { return lnx::fold_sum16(be_sum); }
// ... and from the plain sum of the same words read little-endian, as the dwords in memory give them
// (below 2^32 for d <= 65507).  Folded, both sums lie in 1..0xFFFF unless every word is zero, and swapping
// the bytes of one gives the other (a multiplication by 256 modulo 0xFFFF).
LNX_HD uint32_t echo_icmp_sum_le(uint32_t le_sum) {
  le_sum = (le_sum & 0xFFFFu) + (le_sum >> 16);
  le_sum = (le_sum + (le_sum >> 16)) & 0xFFFFu;
  return ~(((le_sum & 0xFFu) << 8) | (le_sum >> 8)) & 0xFFFFu;
}

// field k < 20 of the frame (field 20, seq, shares its dword with the data): the part the stack's
// configuration decides ...
LNX_HD uint32_t echo_fixed_field(uint32_t k, const RstCfg& c) {
  return k < 3 ? c.gw[k] : k < 6 ? c.mac[k - 3] : k == 6 ? 0x0800u : k == 7 ? 0x4500u : k == 10 ? 0x4000u : k == 11 ? 0x4001u
       : k == 13 ? c.ip[0] : k == 14 ? c.ip[1] : 0u;
}
// ... and the part the entry, the ID and the two sums decide (0 where the other part stands)
LNX_HD uint32_t echo_var_field(uint32_t k, uint32_t addr, uint32_t id, uint32_t d, uint32_t ip_id, uint32_t ip_sum, uint32_t icmp_sum) {
  return k == 8 ? 28u + d : k == 9 ? (ip_id & 0xFFFFu) : k == 12 ? ip_sum : k == 15 ? (addr >> 16) : k == 16 ? (addr & 0xFFFFu)
       : k == 18 ? icmp_sum : k == 19 ? (id & 0xFFFFu) : 0u;
}
LNX_HD uint32_t echo_fixed_word(uint32_t p, const RstCfg& c) { return lnx::slot_pack(echo_fixed_field(2 * p, c), echo_fixed_field(2 * p + 1, c)); }
// dword p < 10 of the frame as it lies in memory: fixed = echo_fixed_word(p, cfg)
LNX_HD uint32_t echo_word(uint32_t p, uint32_t fixed, uint32_t addr, uint32_t id, uint32_t d, uint32_t ip_id, uint32_t ip_sum, uint32_t icmp_sum) {
  return fixed | lnx::slot_pack(echo_var_field(2 * p, addr, id, d, ip_id, ip_sum, icmp_sum),
                                echo_var_field(2 * p + 1, addr, id, d, ip_id, ip_sum, icmp_sum));
}

// The FCS.  The CRC register over one more byte, bit-serial (gf2.hpp zbit): the last
// one to three bytes of a frame whose length is no multiple of 4, and the host's whole frame.
LNX_HD uint32_t echo_crc_byte(uint32_t reg, uint32_t b) {
  reg ^= b & 0xFFu;
  for (uint32_t i = 0; i < 8; ++i) reg = (reg >> 1) ^ ((reg & 1u) ? 0xEDB88320u : 0u);
  return reg;
}
// Over dwords: processing a dword w at register r is Z_4(r ^ w) (gf2.hpp), so the register after m
// dwords w_0 .. w_{m-1} is XOR_p Z_{4 (m - p)}(w_p), the register before them folded into w_0.
// tab(t, i, v): entry v of nibble table i of Z_{4 t}, 1 <= t <= kEchoZ (table_layout.hpp kEchoImgZ).
template <class Tab>
LNX_HD uint32_t echo_fcs_part(uint32_t t, uint32_t word, Tab tab) {
  uint32_t z = 0;
  for (uint32_t i = 0; i < 8; ++i) z ^= tab(t, i, (word >> (4 * i)) & 15u);
  return z;
}

// A wave of 64 lanes, lane p holding dword 64 s + p in step s, needs no exchange per step: lane p keeps
// a register of its own, a_p <- Z_256(a_p) ^ w (Horner over its dwords, 256 bytes apart), and after S
// whole steps the frame's register is XOR_p Z_{4 (64 - p)}(a_p).  btab(k, e): entry e of byte table k of
// Z_256 (table_layout.hpp kEchoImgB).
template <class BTab>
LNX_HD uint32_t echo_fcs_step(uint32_t a, BTab btab) {
  return btab(0, a & 255u) ^ btab(1, (a >> 8) & 255u) ^ btab(2, (a >> 16) & 255u) ^ btab(3, a >> 24);
}

}  // namespace lnxe
