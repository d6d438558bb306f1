// frame_plan.hpp — lneto's receive demux rules up to the checksums, once, for
// both kernels that apply them per frame (ingress_kernel.hip's verdict rows
// and rx_verify_kernel.hip's receive check) and for the host program that runs
// the same code in the CPU suite (tests/cpp/frame_plan_host.cpp); with them
// the constants and the byte rotations (cv, conv) that the transmit kernels
// share too.  The transmit (generate) trees stay inline in their two kernels:
// see the note in tx_finish_kernel.
//
// Plain C++17: no intrinsics, no thread indices and no memory access of its
// own.  rx_plan decides from the frame length and the header fields which
// check fails first and which byte ranges the sums cover; the caller supplies
// the fields through callables and takes the sums its own way:
//   be16(o)   the big-endian 16-bit field at the constant frame offset o
//   byt(o)    the byte at the constant frame offset o
//   le32(o)   bytes o .. o + 3 at the constant offset o, little-endian packed
//   dyn16(o)  a big-endian 16-bit field at a header-length-dependent offset
//   mac(D0, D1)  destination MAC bytes 0..3 and 4..5, little-endian packed
// An accessor is called only once the frame is known to hold the field
// (o + size <= L), and only inside the branch that needs it: the callers'
// accessors read memory or other lanes' registers.
#pragma once
#include <cstdint>
#include "rx_filter.hpp"
#include "wave_util.hpp"

namespace lnx {

// lneto errors.go:6-28
constexpr uint32_t kErrPacketDrop = 2, kErrBadCRC = 3, kErrInvalidField = 14, kErrInvalidLengthField = 15,
                   kErrTruncatedFrame = 18;
constexpr uint32_t kVerifyEvilBit = 1, kVerifyIcmp = 2;
static_assert(kVerifyEvilBit == LNX_VERIFY_EVIL_BIT && kVerifyIcmp == LNX_VERIFY_ICMP, "include/lneto_amd.h");

// bit `proto` of a 256-bit mask held in kernel-argument words (a select chain:
// no indexed scratch)
LNX_HD bool proto_bit(const uint32_t (&m)[8], uint32_t proto) {
  const uint32_t w = proto >> 5;
  const uint32_t word = w == 0 ? m[0] : w == 1 ? m[1] : w == 2 ? m[2] : w == 3 ? m[3] : w == 4 ? m[4]
                        : w == 5 ? m[5] : w == 6 ? m[6] : m[7];
  return (word >> (proto & 31u)) & 1u;
}

// The kernels sum a frame's aligned words as little-endian 16-bit halves:
// S = Σ bytes at even addresses + 256 Σ bytes at odd addresses; with the frame
// starting at an odd address (mis & 1) that is 256 E + O itself (E / O = the
// sums of the bytes at even / odd frame offsets), at an even one E + 256 O,
// which is 256 E + O times 256 modulo 65535 (a byte rotation of the folded
// sum).  The sums of a frame under 64 KiB never wrap 2^32, so sum16 of the
// rotated fold equals sum16 of 256 E + O (RFC 1071 §2(B)).
//
// cv: what a 16-bit big-endian field value v at an even frame offset adds to
// S: its high byte sits at address parity mis & 1
LNX_HD uint32_t cv(uint32_t mis, uint32_t v) { return (mis & 1u) ? v : (((v & 0xFFu) << 8) | (v >> 8)); }
// conv: S as 256 E + O, or a value congruent to it modulo 65535 that is zero
// exactly when it is
LNX_HD uint32_t conv(uint32_t mis, uint32_t S) {
  if (mis & 1u) return S;
  uint32_t f = (S & 0xFFFFu) + (S >> 16);
  f = (f & 0xFFFFu) + (f >> 16);
  return ((f << 8) | (f >> 8)) & 0xFFFFu;
}

// ------------------------------------------------------------------ receive
struct RxPlan {
  uint32_t v = 0;       // verdict so far
  uint32_t v_udp4 = 0;  // IPv4 UDP / ICMP size verdict: demux4 reports it only after the header sum passed
  bool hdr_sum = false, l4_sum = false;    // sums requested: the IPv4 header [14, 34), the transport sum
  int32_t pa = 0, pb = 0, la = 0, lb = 0;  // pseudo-address bytes [pa, pb), transport [la, lb)
  uint32_t lseed = 0;                      // length + protocol words of the pseudo-header
};

// The verdict lneto's receive path reaches at its checksum stage for an
// Ethernet frame of L bytes (FCS excluded):
//   StackEthernet.Demux size checks (internet/stack-ethernet.go:139-165,
//   ethernet/frame.go:13-18,119-127), then by EtherType
//   IPv4 demux4 (internet/stack-ip4.go:100-164): ipv4.NewFrame, the first
//          error of ValidateExceptCRC (ipv4/frame.go:214-238), the header sum
//          over the first 20 bytes only (ipv4/frame.go:138-146), TCP / UDP
//          checksums with the pseudo-header seeds (ipv4/frame.go:154-170) and
//          the UDP size checks (udp/frame.go:15-20,96-104);
//   IPv6 demux6 (internet/stack-ip6.go:86-138): ipv6.NewFrame, ValidateSize
//          (ipv6/frame.go:123-128), TCP / UDP sums with CRCWritePseudo
//          (ipv6/frame.go:104-108); the UDP sum covers the whole IPv6 payload;
//   with kVerifyIcmp, ICMP messages also take their client's Demux checks up to
//          the checksum (ipv4/icmpv4/client.go:89-102: size, echo types,
//          sum with no pseudo-header; ipv6/icmpv6/client.go:100-115: size,
//          sum with the pseudo-header, as CRCWritePseudo with proto 58).
// The verdict is 0 (every check passed, or none applies) or the errGeneric
// code the reference returns (errors.go:6-28).  filt.on: the stack's
// destination and handler checks (ErrPacketDrop) at the reference's places
// among the others; FILT = false compiles them out (accept-all).
template <bool FILT, class Be16, class Byte, class Le32, class Dyn16, class Mac>
LNX_HD RxPlan rx_plan(uint32_t L, uint32_t flags, const RxFilter& filt, Be16 be16, Byte byt, Le32 le32, Dyn16 dyn16,
                      Mac mac) {
  RxPlan r;
  uint32_t& v = r.v;
  if (L < 14) {
    v = kErrTruncatedFrame;
  } else {
    const uint32_t et = be16(12);
    bool eth_drop = false, et_handler = true;
    if (FILT && filt.on) {
      // StackEthernet.Demux (internet/stack-ethernet.go:146-152), before
      // ValidateSize: a frame neither broadcast nor for the stack's MAC is
      // dropped unless multicast frames are accepted and the group bit is set
      uint32_t D0, D1;
      mac(D0, D1);
      const bool bcast = D0 == 0xFFFFFFFFu && D1 == 0xFFFFu;
      const bool mine = D0 == filt.mac_lo && D1 == filt.mac_hi;
      eth_drop = !bcast && !mine && !(filt.eth_mc && (D0 & 1u));
      // handlers.demuxByProto(etype) (stack-ethernet.go:158-161): no handler -> drop
      et_handler = false;
#pragma unroll
      for (int i = 0; i < 8; ++i) et_handler = et_handler || (i < (int)filt.n_et && filt.et[i] == et);
    }
    if (eth_drop) {
      v = kErrPacketDrop;
    } else if (et <= 1500 && L < et) {
      v = kErrInvalidLengthField;
    } else if (et == 0x8100 && L < 18) {
      v = kErrTruncatedFrame;
    } else if (!et_handler) {
      v = kErrPacketDrop;
    } else if (et == 0x0800) {
      const uint32_t M = L - 14;
      if (M < 20) {
        v = kErrTruncatedFrame;
      } else {
        const uint32_t b0 = byt(14), tl = be16(16), ihl = b0 & 15u;
        if (FILT && filt.on && filt.ip4 != 0u) {
          // demux4's destination check (internet/stack-ip4.go:108-119), before ValidateExceptCRC
          const uint32_t dst = le32(30);
          const bool mc = (dst & 0xF0u) == 0xE0u, bc = dst == 0xFFFFFFFFu;  // ipv4/definitions.go:17-36
          if (dst != filt.ip4 && !(filt.ip4_mc && mc) && !(filt.ip4_bc && bc)) v = kErrPacketDrop;
        }
        if (v != 0) {
        } else if (tl < 20) v = kErrInvalidLengthField;
        else if (tl > M) v = kErrTruncatedFrame;
        else if (ihl < 5 || ihl * 4 > tl) v = kErrInvalidLengthField;
        else if ((b0 >> 4) != 4) v = kErrInvalidField;
        else if ((flags & kVerifyEvilBit) && (be16(20) & (1u << 13))) v = kErrPacketDrop;
        if (v == 0) {
          r.hdr_sum = true;
          const uint32_t hl = ihl * 4, proto = byt(23), P = tl - hl;
          if (FILT && filt.on && !proto_bit(filt.p4, proto)) {
            r.v_udp4 = kErrPacketDrop;  // nodeByProto nil (stack-ip4.go:135-141), after the header sum
          } else if (proto == 6) {
            r.l4_sum = true;
            r.pa = 26, r.pb = 34, r.la = 14 + hl, r.lb = 14 + tl;
            r.lseed = ((tl - hl) & 0xFFFFu) + 6u;
          } else if (proto == 17) {
            if (P < 8) {
              r.v_udp4 = kErrTruncatedFrame;
            } else {
              const uint32_t ul = dyn16(14 + hl + 4);
              if (ul < 8) r.v_udp4 = kErrInvalidLengthField;
              else if (ul > P) r.v_udp4 = kErrTruncatedFrame;
              else {
                r.l4_sum = true;
                r.pa = 26, r.pb = 34, r.la = 14 + hl, r.lb = 14 + hl + ul;
                r.lseed = ul + 17u;
              }
            }
          } else if (proto == 1 && (flags & kVerifyIcmp)) {
            if (P < 8) {
              r.v_udp4 = kErrTruncatedFrame;
            } else {
              const uint32_t type = dyn16(14 + hl) >> 8;
              if (type != 0 && type != 8) {
                r.v_udp4 = kErrPacketDrop;
              } else {
                r.l4_sum = true;  // no pseudo-header: [pa, pb) empty, lseed 0
                r.la = 14 + hl, r.lb = 14 + tl;
              }
            }
          }
        }
      }
    } else if (et == 0x86DD) {
      const uint32_t M = L - 14;
      if (M < 40) {
        v = kErrTruncatedFrame;
      } else {
        const uint32_t pl = be16(18), proto = byt(20);
        if (FILT && filt.on && (filt.ip6[0] | filt.ip6[1] | filt.ip6[2] | filt.ip6[3]) != 0u) {
          // demux6's destination check (internet/stack-ip6.go:93-98), before ValidateSize
          const uint32_t d0 = le32(38), d1 = le32(42), d2 = le32(46), d3 = le32(50);
          const bool mine = d0 == filt.ip6[0] && d1 == filt.ip6[1] && d2 == filt.ip6[2] && d3 == filt.ip6[3];
          if (!mine && !(filt.ip6_mc && (d0 & 0xFFu) == 0xFFu)) v = kErrPacketDrop;  // internal/ip.go:30-35
        }
        if (v != 0) {
        } else if (pl + 40 > M) {
          v = kErrInvalidLengthField;
        } else if (FILT && filt.on && !proto_bit(filt.p6, proto)) {
          v = kErrPacketDrop;  // nodeByProto nil (stack-ip6.go:107-111), before the sums
        } else if (proto == 6 || proto == 17 || (proto == 58 && (flags & kVerifyIcmp))) {
          // demux6 size-checks the UDP header only; TCP goes straight to the
          // sum (internet/stack-ip6.go:116-137), whatever pl is.  ICMPv6:
          // icmpv6.NewFrame's size check, then the same pseudo-header sum.
          if (proto == 58 && pl < 8) v = kErrTruncatedFrame;
          if (proto == 17) {
            if (pl < 8) v = kErrTruncatedFrame;
            else if (be16(58) < 8) v = kErrInvalidLengthField;
            else if (be16(58) > pl) v = kErrTruncatedFrame;
          }
          if (v == 0) {
            r.l4_sum = true;
            r.pa = 22, r.pb = 54, r.la = 54, r.lb = 54 + pl;  // AddUint32(pl), AddUint32(proto): high halves 0
            r.lseed = pl + proto;
          }
        }
      }
    }
  }
  return r;
}

// The verdict once the sums are in: hX / tX = 256 E + O of the header bytes and
// of the pseudo-address + transport bytes (or conv's congruent value).
LNX_HD uint32_t rx_verdict(const RxPlan& r, uint32_t hX, uint32_t tX) {
  uint32_t v = r.v;
  if (v == 0 && r.hdr_sum && fold_sum16(hX) != 0) v = kErrBadCRC;
  if (v == 0) v = r.v_udp4;  // udp.NewFrame / ValidateSize follow CalculateHeaderCRC (stack-ip4.go:128-159)
  if (v == 0 && r.l4_sum && fold_sum16(tX + r.lseed) != 0) v = kErrBadCRC;
  return v;
}

}  // namespace lnx
