"""ARP for IPv4 over Ethernet, restated in Python.

``arp_demux`` and ``arp_frame`` restate lneto_amd/csrc/arp_plan.hpp line by line
against the reference, from the byte strings the reference handles (the library
works on little-endian dwords):

  internet/stack-ethernet.go:158-161  the EtherType picks the handler: the delivery record's
                                      H_ETH slot (tests/deliver_ref.py rule 3)
  arp/frame.go:17-22                  NewFrame: len(b) < 28 is ErrTruncatedFrame (18)
  arp/frame.go:137-146                ValidateSize: minLen = 8 + 2 (hlen + ilen); len(b) < minLen is
                                      errShortARP (18), else minLen > 255 is errLargeSizes (2)
  arp/handler.go:160-169              Demux: newframe, ValidateSize, before any type check
  arp/handler.go:170-177              hardware type 1 / length 6, protocol type 0x0800 / length 4,
                                      else ErrMismatch (10)
  arp/handler.go:178-187              OpRequest: target address not ours: nil, nothing happens;
                                      else acquireNext().use(sender hw, sender proto, pending response)
  arp/handler.go:188-198              OpReply: cache.Lookup(sender proto): host state, the learn record
  arp/handler.go:199-201              any other op: errARPUnsupported (9)
  arp/handler.go:126-158              Encapsulate: a pending response is OpReply, a pending query OpRequest;
                                      put; the Ethernet destination = broadcast (query) or the ARP
                                      body's target hardware address (reply), trySetEthernetDst :215-219
  arp/cache.go:32-71                  put: hardware 1 / 6, the op, protocol 0x0800 / 4, sender = ours,
                                      target = the entry's mac and addr; n = 28
  arp/handler.go:112-124              StartQuery: the entry's mac is [6]byte{}
  internet/stack-ethernet.go:170-217  gateway MAC (then overwritten, above), our MAC, EtherType,
                                      zero padding to 60, LE32(crc(0, frame[:n])) appended

The cache's size, eviction and ageing, cache.Lookup and the resolve callback
are not restated.  The library takes ONE MAC for the Ethernet
source and the ARP sender.  No Go toolchain is available to this suite: the
restatement is pinned by these citations and by the reference's own TestHandler
as known answers (tests/test_arp_reply.py)."""
from __future__ import annotations

import struct
import zlib

from tests import deliver_ref as D
from tests import framegen as G

OP_REQUEST, OP_REPLY = 1, 2
ERR_DROP, ERR_UNSUPPORTED, ERR_MISMATCH, ERR_TRUNCATED = 2, 9, 10, 18   # errors.go
BROADCAST = b"\xff" * 6


def reaches(frame: bytes, rec: dict) -> bool:
    """The frame under this record is handed to the ARP handler."""
    if rec["verdict"] != 0 or not D.H_ETH <= rec["handler"] <= D.H_ETH + 8:
        return False
    return len(frame) >= 14 and frame[12:14] == b"\x08\x06"


def arp_demux(frame: bytes, rec: dict, our_ip: bytes):
    """(kind, entry, verdict): kind 0 nothing, 1 a request for our_ip, 2 a reply;
    entry the sender as dict(hw=, ip=) for kinds 1 and 2, else None."""
    if not reaches(frame, rec):
        return 0, None, 0
    b = frame[14:]
    if len(b) < 28:                                            # NewFrame
        return 0, None, ERR_TRUNCATED
    hlen, ilen = b[4], b[5]
    min_len = 8 + 2 * (hlen + ilen)                            # ValidateSize
    if len(b) < min_len:
        return 0, None, ERR_TRUNCATED
    if min_len > 255:
        return 0, None, ERR_DROP
    if struct.unpack(">H", b[0:2])[0] != 1 or hlen != 6:
        return 0, None, ERR_MISMATCH
    if struct.unpack(">H", b[2:4])[0] != 0x0800 or ilen != 4:
        return 0, None, ERR_MISMATCH
    op = struct.unpack(">H", b[6:8])[0]
    sender = dict(hw=bytes(b[8:14]), ip=bytes(b[14:18]))       # Sender()
    if op == OP_REQUEST:
        if b[24:28] != our_ip:                                 # Target(): not for us
            return 0, None, 0
        return 1, sender, 0
    if op == OP_REPLY:
        return 2, sender, 0
    return 0, None, ERR_UNSUPPORTED


def arp_frame(mac: bytes, ip4: bytes, fcs: bool, op: int, e: dict) -> bytes:
    body = struct.pack(">HHBBH", 1, 0x0800, 6, 4, op) + mac + ip4 + e["hw"] + e["ip"]   # put
    dst = BROADCAST if op == OP_REQUEST else body[18:24]       # the ARP body's target hardware address
    f = dst + mac + b"\x08\x06" + body
    f += bytes(60 - len(f))
    if fcs:
        f += struct.pack("<I", zlib.crc32(f))
    return f


def arp_batch(frames, recs, mac, ip4, fcs, cap=None, cap_seen=None):
    """(replies, src, seen, counts) of a batch; seen: (hw, ip, frame index)."""
    out, src, seen, w1, w2 = [], [], [], 0, 0
    for i, (f, r) in enumerate(zip(frames, recs)):
        kind, e, _ = arp_demux(f, r, ip4)
        if kind == 1:
            if cap is None or w1 < cap:
                out.append(arp_frame(mac, ip4, fcs, OP_REPLY, e))
                src.append(i)
            w1 += 1
        elif kind == 2:
            if cap_seen is None or w2 < cap_seen:
                seen.append((e["hw"], e["ip"], i))
            w2 += 1
    return out, src, seen, (len(out), w1, len(seen), w2)


# ------------------------------------------------------------------ the tests' stack and frames
MAC, GW_MAC, IP4 = G.MAC_US, bytes.fromhex("4e8b3af9fb6b"), G.IP4_DST   # ether()'s destination / source, ipv4()'s destination
PEER_MAC, PEER_IP = bytes.fromhex("4e8b3af9fb6b"), bytes([192, 168, 10, 77])
OTHER_IP = bytes([192, 168, 10, 99])


def arp_body(op: int = OP_REQUEST, sha: bytes = PEER_MAC, spa: bytes = PEER_IP, tha: bytes = bytes(6), tpa: bytes = IP4,
             htype: int = 1, ptype: int = 0x0800, hlen: int = 6, ilen: int = 4) -> bytes:
    return struct.pack(">HHBBH", htype, ptype, hlen, ilen, op) + sha + spa + tha + tpa


def arp_eth(body: bytes, pad: bool = True, et: int = 0x0806) -> bytes:
    f = G.ether(et, body)
    return f + bytes(max(0, 60 - len(f))) if pad else f


def filt():
    import lneto_amd as L
    return L.RxFilter.make(mac=G.MAC_US, **D.FILTER_KW)   # lists 0x0806: slot 2


def delivered(frame: bytes, filter="stack") -> dict:
    """The record lnx_rx_deliver gives the frame under a zero receive verdict; filter None: the accept-all one."""
    import lneto_amd as L
    return L.rx_deliver(frame, 0, filt() if filter == "stack" else filter, None, 1)


def forced(handler: int = D.H_ETH + 2, verdict: int = 0) -> dict:
    """A record as a stale or foreign one would stand over the frame."""
    return dict(ip_end=0, handler=handler, l4_off=0, src_port=0, dst_port=0, verdict=verdict, flags=0, zero=0)


def self_made_cases() -> list[tuple[str, bytes, dict]]:
    """(label, frame, record)."""
    out = []

    def add(label, f, rec=None):
        out.append((label, f, delivered(f) if rec is None else rec))

    # valid frames
    add("request_padded", arp_eth(arp_body()))
    add("request_unpadded", arp_eth(arp_body(), pad=False))
    for k in range(4):
        tpa = bytearray(IP4)
        tpa[k] ^= 0x01
        add(f"request_other_byte{k}", arp_eth(arp_body(tpa=bytes(tpa))))
    add("reply_for_us", arp_eth(arp_body(OP_REPLY, tha=MAC, tpa=IP4)))
    add("reply_for_other", arp_eth(arp_body(OP_REPLY, tha=bytes.fromhex("0a0b0c0d0e0f"), tpa=OTHER_IP)))
    add("probe_sender_zero", arp_eth(arp_body(spa=bytes(4))))
    add("sender_hw_broadcast", arp_eth(arp_body(sha=BROADCAST)))
    add("sender_hw_multicast", arp_eth(arp_body(sha=bytes.fromhex("01005e000001"))))
    # truncation
    add("p27", arp_eth(arp_body(), pad=False)[:41])
    add("p28", arp_eth(arp_body(), pad=False)[:42])
    # length fields
    big = lambda hlen, ilen, P: G.ether(0x0806, (struct.pack(">HHBBH", 1, 0x0800, hlen, ilen, 1) + bytes(range(256)) * 2)[:P])  # noqa: E731
    add("h6_i16_p46", big(6, 16, 46))
    add("h6_i16_p52", big(6, 16, 52))
    add("h255_i255_p46", big(255, 255, 46))
    add("h100_i28_p263", big(100, 28, 263))
    add("h100_i28_p264", big(100, 28, 264))
    add("h5_i4", arp_eth(arp_body(hlen=5)))
    add("h6_i3", arp_eth(arp_body(ilen=3)))
    # type and op fields
    for htype in (0, 2, 0x0100):
        add(f"htype_{htype:#x}", arp_eth(arp_body(htype=htype)))
    for ptype in (0x86DD, 0x0806):
        add(f"ptype_{ptype:#x}", arp_eth(arp_body(ptype=ptype)))
    for op in (0, 3, 0x0100, 0x0200):
        add(f"op_{op:#x}", arp_eth(arp_body(op=op)))
    # stale records
    req = arp_eth(arp_body(), pad=False)
    for n in (0, 13, 14, 41, 42):
        add(f"forced_len{n}", req[:n], forced())
    ip4 = G.ether(0x0800, G.ipv4(17, G.udp(b"hello")))
    add("forced_over_ip4", ip4, forced())
    add("handler_eth9", req, forced(D.H_ETH + 9))
    add("handler_ip4_1", req, forced(D.H_IP4 + 1))
    add("handler_none", req, forced(D.H_NONE))
    add("verdict_nonzero", req, forced(verdict=2))
    add("null_filter", req, delivered(req, filter=None))
    vlan = G.ether(0x8100, struct.pack(">HH", 5, 0x0806) + arp_body())
    add("vlan_tagged", vlan, delivered(vlan, filter=None))
    add("vlan_tagged_forced", vlan, forced())
    return out


# label -> (kind, verdict): what every self-made case must give
EXPECT = {
    "request_padded": (1, 0), "request_unpadded": (1, 0),
    "request_other_byte0": (0, 0), "request_other_byte1": (0, 0), "request_other_byte2": (0, 0), "request_other_byte3": (0, 0),
    "reply_for_us": (2, 0), "reply_for_other": (2, 0), "probe_sender_zero": (1, 0),
    "sender_hw_broadcast": (1, 0), "sender_hw_multicast": (1, 0),
    "p27": (0, 18), "p28": (1, 0),
    "h6_i16_p46": (0, 18), "h6_i16_p52": (0, 10), "h255_i255_p46": (0, 18), "h100_i28_p263": (0, 18),
    "h100_i28_p264": (0, 2), "h5_i4": (0, 10), "h6_i3": (0, 10),
    "htype_0x0": (0, 10), "htype_0x2": (0, 10), "htype_0x100": (0, 10),
    "ptype_0x86dd": (0, 10), "ptype_0x806": (0, 10),
    "op_0x0": (0, 9), "op_0x3": (0, 9), "op_0x100": (0, 9), "op_0x200": (0, 9),
    "forced_len0": (0, 0), "forced_len13": (0, 0), "forced_len14": (0, 18), "forced_len41": (0, 18), "forced_len42": (1, 0),
    "forced_over_ip4": (0, 0), "handler_eth9": (0, 0), "handler_ip4_1": (0, 0), "handler_none": (0, 0),
    "verdict_nonzero": (0, 0), "null_filter": (1, 0), "vlan_tagged": (0, 0), "vlan_tagged_forced": (0, 0),
}


def census_cases():
    """(frame, host record as a dict) of every census frame under the stack's filter, FCS results all good."""
    import lneto_amd as L
    from oracle import oracle as O
    f_on = filt()
    ofilt = D.ofilter(True)
    return [(f, L.rx_deliver(f, O.ingress_verdict(f, D.VERIFY_FLAGS, ofilt), f_on, None, 1)) for _, f in D.census_frames()]
