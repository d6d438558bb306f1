"""Echo replies for ICMPv4 echo requests, restated in Python.

``echo_entry`` and ``echo_frame`` restate lneto_amd/csrc/echo_plan.hpp line by
line against the reference, from the byte strings the reference handles (the
library works on 16-bit fields and dwords):

  internet/stack-ip4.go:134-141,168-170  demux4: nodeByProto(1), Demux(frame[:totalLen], off):
                                  the delivery record's handler H_IP4 + 1, l4_off and ip_end
                                  (tests/deliver_ref.py)
  ipv4/icmpv4/icmpv4.go:62-67     NewFrame: fewer than 8 bytes -> ErrTruncatedFrame
  ipv4/icmpv4/client.go:95-98     types other than 8 and 0 are dropped
  ipv4/icmpv4/client.go:99-102    PayloadSum16(rawdata) != 0 -> ErrBadCRC: the receive verdict's
                                  business under VERIFY_ICMP, not checked again here
  ipv4/icmpv4/client.go:103-110   raddr = GetIPAddr(carrierData) source when it has 4 bytes
  internal/ip.go:9-27             nibble 4: src = buf[12:16]
  ipv4/frame.go:229-234           demux4's NewFrame + ValidateExceptCRC: version 4 under a zero verdict
  ipv4/icmpv4/client.go:111-132   type 8: len(data) == 0 -> ErrPacketDrop; else data, id, seq, raddr kept
  ipv4/icmpv4/client.go:162-176   Encapsulate: type 0, id, seq, the data; n = 8 + len(data)
  ipv4/icmpv4/client.go:209-218   code 0, checksum 0, PayloadSum16 over the n bytes, destination address
  internet/stack-ip4.go:178-231   0x45, ToS 0, ID, 0x4000, TTL 64, source, total length 20 + n,
                                  protocol 1, CalculateHeaderCRC; no transport sum for ICMP (:213-229)
  internet/stack-ethernet.go:170-217  gateway MAC, our MAC, EtherType, zero padding to 60,
                                  LE32(crc(0, frame[:n])) appended

incomingEcho's capacity and ErrExhausted (client.go:113-116), the response
ring's size (:123-127), one reply per Encapsulate call and the MTU clip of the
carrier buffer are not restated: ``echo_replies`` answers every queueing frame
in arrival order.  A stale record over a frame whose version
nibble is not 4 queues nothing (the reference would answer it to 0.0.0.0).  No
Go toolchain is available to this suite: the restatement is pinned by these
citations and by the library's own receive checks over every reply
(tests/test_echo_reply.py)."""
from __future__ import annotations

import struct
import zlib

from oracle import oracle as O
from tests import deliver_ref as D
from tests import framegen as G
from tests import reply_ref as R

H_ICMP4 = D.H_IP4 + 1
MAC, GW_MAC, IP4 = R.MAC, R.GW_MAC, R.IP4
CENSUS_SETTING = R.CENSUS_SETTING
MAX_DATA = 65507   # 65535 - 20 - 8
# the data lengths of the edges: padding ends at 60 (18), one / two blocks with the FCS (18 / 19), an MTU, a jumbo frame
EDGE_LENGTHS = (1, 2, 3, 4, 17, 18, 19, 1472, 8972)


def echo_entry(frame: bytes, rec: dict):
    """The entry frame (FCS stripped) queues under its delivery record, or None."""
    L = len(frame)
    if rec["verdict"] != 0 or rec["handler"] != H_ICMP4:
        return None
    l4, end = rec["l4_off"], rec["ip_end"]
    if l4 < 34 or end > L:                 # a record that does not belong to these bytes
        return None
    rawdata = frame[l4:end]                # carrierData[frameOffset:] of frame[:totalLen]
    if len(rawdata) < 8:                   # NewFrame: ErrTruncatedFrame
        return None
    if rawdata[0] != 8:                    # type 0 sends nothing; others are dropped
        return None
    if frame[14] >> 4 != 4:                # (not restated: the reference answers 0.0.0.0)
        return None
    data = rawdata[8:]
    if len(data) == 0 or len(data) > MAX_DATA:   # ErrPacketDrop; more than a total length can say
        return None
    ident, seq = struct.unpack(">HH", rawdata[4:8])
    return dict(remote_addr=bytes(frame[26:30]), id=ident, seq=seq, data_off=l4 + 8, data_len=len(data))


def echo_frame(mac: bytes, gw_mac: bytes, ip4: bytes, fcs: bool, e: dict, data: bytes, ip_id: int) -> bytes:
    icmp = bytearray(struct.pack(">BBHHH", 0, 0, 0, e["id"], e["seq"]) + data)
    icmp[2:4] = struct.pack(">H", O.CRC791().payload_sum16(bytes(icmp)))
    ip = bytearray(struct.pack(">BBHHHBBH", 0x45, 0, 20 + len(icmp), ip_id, 0x4000, 64, 1, 0) + ip4 + e["remote_addr"])
    ip[10:12] = struct.pack(">H", O.ipv4_header_sum16(bytes(ip)))
    f = gw_mac + mac + b"\x08\x00" + bytes(ip) + bytes(icmp)
    f += bytes(max(60 - len(f), 0))
    if fcs:
        f += struct.pack("<I", zlib.crc32(f))
    return f


def echo_replies(frames, recs, mac, gw_mac, ip4, fcs, ip_ids, cap=None, cap_blocks=None):
    """(replies, starts, src, wanted, blocks_wanted) of a batch: reply k answers the k-th
    queueing frame, carries ip_ids[k] and starts at 64 x the earlier replies' blocks."""
    out, starts, src, wanted, blocks, full = [], [], [], 0, 0, False
    for i, (f, r) in enumerate(zip(frames, recs)):
        e = echo_entry(f, r)
        if e is None:
            continue
        n = max(60, 42 + e["data_len"]) + (4 if fcs else 0)
        nb = -(-n // 64)
        if not full and (cap is None or wanted < cap) and (cap_blocks is None or blocks + nb <= cap_blocks):
            out.append(echo_frame(mac, gw_mac, ip4, fcs, e, f[e["data_off"]:e["data_off"] + e["data_len"]], ip_ids[wanted]))
            starts.append(64 * blocks)
            src.append(i)
        else:
            full = True
        wanted += 1
        blocks += nb
    return out, starts, src, wanted, blocks


# ------------------------------------------------------------------ the tests' frames
def echo_request(data: bytes, ident: int = 0x1234, seq: int = 1, opts: bytes = b"", type_: int = 8, code: int = 0) -> bytes:
    """An Ethernet frame (no FCS) with an ICMPv4 message of the echo shape to the stack's address, checksum right."""
    msg = bytearray(G.icmp(type_, data, ident, seq))
    msg[1] = code
    return G.ether(0x0800, G.ipv4(1, bytes(msg), opts=opts))


def record_of(frame: bytes, **over) -> dict:
    """The record the delivery rules give an IPv4 ICMP frame with a zero verdict, fields overridden."""
    ihl = frame[14] & 15
    rec = dict(ip_end=14 + struct.unpack(">H", frame[16:18])[0], handler=H_ICMP4, l4_off=14 + 4 * ihl, src_port=0,
               dst_port=0, verdict=0, flags=0, zero=0)
    rec.update(over)
    return rec


def pattern(n: int, seed: int = 0) -> bytes:
    return bytes((seed + 7 * k + (k >> 8)) & 0xFF for k in range(n))


def self_made_cases() -> list[tuple[str, bytes, dict]]:
    """(label, frame, record): the edges of the entry rule and of the frame that the census does not reach."""
    out = []
    for ihl in range(5, 16):
        f = echo_request(pattern(20 + ihl, ihl), 0x4000 + ihl, ihl, opts=bytes(range(1, 4 * (ihl - 5) + 1)))
        out.append((f"ihl{ihl}", f, record_of(f)))
    for d in EDGE_LENGTHS + (MAX_DATA,):
        f = echo_request(pattern(d, d), 0xBEEF, d & 0xFFFF)
        out.append((f"data{d}", f, record_of(f)))
    f = echo_request(bytes(8), 0, 0)
    out.append(("all_zero", f, record_of(f)))              # the reply's checksum is 0xFFFF
    f = echo_request(bytes(7), 0, 0)
    out.append(("all_zero_odd", f, record_of(f)))
    for d in (1, 2, 31, 32):
        f = echo_request(b"\xff" * d, 0xFFFF, 0xFFFF)
        out.append((f"all_ff{d}", f, record_of(f)))
    f = echo_request(pattern(9), type_=0)
    out.append(("type0", f, record_of(f)))
    f = echo_request(pattern(9), type_=3)
    out.append(("type3", f, record_of(f)))
    f = echo_request(pattern(9, 3), code=7)
    out.append(("code7", f, record_of(f)))                 # the reply's code is 0
    f = echo_request(b"")
    out.append(("no_data", f, record_of(f)))               # l4 + 8 == end
    f = echo_request(pattern(5))
    out.append(("truncated_icmp", f, record_of(f, ip_end=34 + 7)))   # l4 + 8 > end
    out.append(("one_byte_of_data", f, record_of(f, ip_end=34 + 9)))
    f = echo_request(pattern(30, 1))
    assert len(f) == 72
    out.append(("end_is_len", f, record_of(f)))            # end == L: the last byte the copy reads ends the frame
    out.append(("end_past_len", f, record_of(f, ip_end=73)))
    out.append(("trailer", f + bytes(6), record_of(f)))    # end < L: the trailer is not data
    out.append(("l4_33", f, record_of(f, l4_off=33)))
    out.append(("l4_far", f, record_of(f, l4_off=0xFFFF)))
    out.append(("l4_35_forced", f, record_of(f, l4_off=35)))   # whatever lies there decides
    f6 = bytearray(f)
    f6[14] = 0x65
    out.append(("nibble6_forced", bytes(f6), record_of(f)))
    out.append(("handler_igmp", f, record_of(f, handler=D.H_IP4 + 2)))
    out.append(("verdict2", f, record_of(f, verdict=2)))
    out.append(("len0", b"", record_of(f)))
    big = echo_request(pattern(100)) + bytes(70000)
    out.append(("data_past_total_length", big, record_of(big, ip_end=34 + 8 + MAX_DATA + 1)))
    out.append(("data_at_total_length", big, record_of(big, ip_end=34 + 8 + MAX_DATA)))
    return out
