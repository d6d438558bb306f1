"""RST replies for SYNs to closed ports, restated in Python.

``rst_entry`` and ``rst_frame`` restate lneto_amd/csrc/reply_plan.hpp line by
line against the reference, from the byte strings the reference handles (the
library works on 16-bit fields and dwords):

  internet/stack-ports.go:70-74   TCP miss, offset + 14 <= len(b), SYN without RST / ACK:
                                  the delivery record's DLV_RST (tests/deliver_ref.py)
  internet/stack-ports.go:75-80   srcaddr = GetIPAddr(b); remotePort = be16(b[offset:]);
                                  segSeq = be32(b[offset + 4:]);
                                  Queue(srcaddr, remotePort, port, 0, segSeq + 1, RST|ACK)
  internal/ip.go:9-27             nibble 4: src = buf[12:16]; nibble 6: src = buf[8:24]
  tcp/rst.go:22-33                Queue keeps len(srcaddr) == 4 only
  tcp/rst.go:38-63                Drain: ports swapped, SetSegment(seq, ack, flags, offset 5),
                                  urgent pointer 0, destination address
  tcp/frame.go:92-95,144-154      offset << 12 | flags & 0x1ff; window = seg.WND = 0
  internet/stack-ip4.go:178-231   0x45, ToS 0, ID, 0x4000, TTL 64, source, total length 40,
                                  protocol 6, CalculateHeaderCRC, CRCWriteTCPPseudo + PayloadSum16
  internet/stack-ip4.go:189-195   seed = (ipID + 1) ^ ip4[0]; id = Prand16(seed); ipID = id
  internal/prand.go:4-10          Prand16: seed ^= seed << 7; seed ^= seed >> 9; seed ^= seed << 8
  internet/stack-ethernet.go:170-217  gateway MAC, our MAC, EtherType, zero padding to 60,
                                  LE32(crc(0, frame[:n])) appended

RSTQueue's bound of four entries and its last-in first-out drain (tcp/rst.go:8,
23,44-45) are not restated: ``rst_replies`` answers every queueing frame in
arrival order.  No Go toolchain is available to this suite:
the restatement is pinned by these citations and by the reference's own tests
as known answers (tests/test_rst_reply.py)."""
from __future__ import annotations

import struct
import zlib

from oracle import oracle as O

DLV_RST = 1
FLAG_SYN, FLAG_RST, FLAG_ACK = 0x02, 0x04, 0x10


def prand16(seed: int) -> int:
    seed &= 0xFFFF
    seed ^= (seed << 7) & 0xFFFF
    seed ^= seed >> 9
    seed ^= (seed << 8) & 0xFFFF
    return seed


def id_chain(ip4_first: int, ip_id: int, n: int) -> list[int]:
    out = []
    for _ in range(n):
        ip_id = prand16(((ip_id + 1) & 0xFFFF) ^ ip4_first)
        out.append(ip_id)
    return out


def rst_entry(frame: bytes, rec: dict):
    """The entry frame (FCS stripped) queues under its delivery record, or None."""
    L = len(frame)
    if not rec["flags"] & DLV_RST:
        return None
    off = rec["l4_off"]
    if L < 30 or off + 8 > L:          # nothing past the frame is read, whatever the record says
        return None
    b = frame[14:]
    if b[0] >> 4 != 4:                 # nibble 6: a 16-byte source, dropped by Queue; others: GetIPAddr fails
        return None
    srcaddr = b[12:16]
    seg_seq = struct.unpack(">I", frame[off + 4:off + 8])[0]
    return dict(remote_addr=bytes(srcaddr), remote_port=rec["src_port"], local_port=rec["dst_port"], seq=0,
                ack=(seg_seq + 1) & 0xFFFFFFFF, flags=FLAG_RST | FLAG_ACK)


def rst_frame(mac: bytes, gw_mac: bytes, ip4: bytes, fcs: bool, e: dict, ip_id: int) -> bytes:
    tcp = bytearray(struct.pack(">HHIIHHHH", e["local_port"], e["remote_port"], e["seq"], e["ack"],
                                (5 << 12) | (e["flags"] & 0x01FF), 0, 0, 0))
    ip = bytearray(struct.pack(">BBHHHBBH", 0x45, 0, 40, ip_id, 0x4000, 64, 6, 0) + ip4 + e["remote_addr"])
    ip[10:12] = struct.pack(">H", O.ipv4_header_sum16(bytes(ip)))
    tcp[16:18] = struct.pack(">H", O.ipv4_tcp_pseudo(bytes(ip)).payload_sum16(bytes(tcp)))
    f = gw_mac + mac + b"\x08\x00" + bytes(ip) + bytes(tcp)
    f += bytes(60 - len(f))
    if fcs:
        f += struct.pack("<I", zlib.crc32(f))
    return f


def rst_replies(frames, recs, mac, gw_mac, ip4, fcs, ip_ids, cap=None):
    """(replies, src, wanted) of a batch: reply k answers the k-th queueing frame
    and carries ip_ids[k]; at most cap replies."""
    out, src, wanted = [], [], 0
    for i, (f, r) in enumerate(zip(frames, recs)):
        e = rst_entry(f, r)
        if e is None:
            continue
        if cap is None or wanted < cap:
            out.append(rst_frame(mac, gw_mac, ip4, fcs, e, ip_ids[wanted]))
            src.append(i)
        wanted += 1
    return out, src, wanted


# ------------------------------------------------------------------ the tests' stack and frames
from tests import deliver_ref as D   # noqa: E402
from tests import framegen as G      # noqa: E402

MAC, GW_MAC, IP4 = G.MAC_US, bytes.fromhex("4e8b3af9fb6b"), G.IP4_DST   # ether()'s destination / source, ipv4()'s destination
CENSUS_SETTING = 4   # deliver_ref.SETTINGS "filt_dup": the stack's filter, ports 7, 80, 80, 443 / 53, 53, 67


def syn_frame(seq: int, sport: int = 5000, dport: int = 443, flags: int = FLAG_SYN, opts: bytes = b"",
              payload: bytes = b"") -> bytes:
    seg = struct.pack(">HHIIHHHH", sport, dport, seq, 0, 0x5000 | flags, 0xFAF0, 0, 0) + payload
    return G.ether(0x0800, G.ipv4(6, seg, opts=opts))


def forced(frame: bytes, l4_off: int, flags: int = DLV_RST) -> dict:
    """A record with the flag forced, as a stale or foreign record would carry it."""
    be16 = lambda o: (frame[o] << 8) | frame[o + 1] if o + 2 <= len(frame) else 0   # noqa: E731
    return dict(ip_end=len(frame), handler=D.H_NONE, l4_off=l4_off, src_port=be16(l4_off), dst_port=be16(l4_off + 2),
                verdict=2, flags=flags, zero=0)


def self_made_cases() -> list[tuple[str, bytes, dict]]:
    """(label, frame, record): the edges of the entry rule that the census does not reach."""
    out = []
    for ihl in range(5, 16):
        f = syn_frame(1000 + ihl, opts=bytes(range(1, 4 * (ihl - 5) + 1)))
        out.append((f"ihl{ihl}", f, forced(f, 14 + 4 * ihl)))
    f = syn_frame(0xFFFFFFFF)
    out.append(("ack_wrap", f, forced(f, 34)))
    seg = struct.pack(">HHIIHHHH", 5000, 443, 77, 0, 0x5002, 0xFAF0, 0, 0)
    for nib in (4, 6):   # demux6 never looks at the nibble; GetIPAddr does (internal/ip.go:9-27)
        f6 = bytearray(G.ether(0x86DD, G.ipv6(6, seg)))
        f6[14] = (nib << 4) | (f6[14] & 15)
        out.append((f"ip6_nib{nib}", bytes(f6), forced(bytes(f6), 54, DLV_RST | D.DLV_IP6)))
    for nib in (0, 5, 15):
        f = bytearray(syn_frame(9))
        f[14] = (nib << 4) | 5
        out.append((f"nib{nib}_forced", bytes(f), forced(bytes(f), 34)))
    f = syn_frame(9)
    out.append(("l4_past_frame", f, forced(f, len(f) - 7)))          # l4_off + 8 = L + 1
    out.append(("l4_ends_frame", f[:42], forced(f[:42], 34)))        # l4_off + 8 = L: the last byte a rule reads
    out.append(("l4_far", f, forced(f, 0xFFFF)))
    out.append(("len29", f[:29], forced(f[:29], 14)))
    out.append(("len30", f[:30], forced(f[:30], 14)))                # bytes 26..29 end the frame; ack from bytes 18..21
    out.append(("len30_l4_22", f[:30], forced(f[:30], 22)))          # l4_off + 8 = 30 = L
    out.append(("len0", b"", forced(b"", 0)))
    out.append(("unflagged", f, forced(f, 34, 0)))
    return out


def census_cases(setting: int = CENSUS_SETTING):
    """(frame, host record as a dict) of every census frame under one setting,
    FCS results all good: the records lnx_rx_deliver gives (tests/test_deliver.py
    checks them against the restatement)."""
    import lneto_amd as L
    _, on, ports = D.SETTINGS[setting]
    filt = L.RxFilter.make(mac=G.MAC_US, **D.FILTER_KW) if on else None
    cp = None if ports is None else L.RxPorts.make(tcp=ports[0], udp=ports[1])
    ofilt = D.ofilter(on)
    out = []
    for _, f in D.census_frames():
        v = O.ingress_verdict(f, D.VERIFY_FLAGS, ofilt)
        out.append((f, L.rx_deliver(f, v, filt, cp, 1)))
    return out, filt, cp
