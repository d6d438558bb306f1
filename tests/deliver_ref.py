"""Receive delivery, restated in Python, and the frames that reach every branch of it.

``deliver`` restates the step lneto's receive path takes once the
checksum-stage verdict is in (lnx_rx_deliver, lneto_amd/csrc/deliver_plan.hpp),
line by line against the reference:

  internet/stack-ethernet.go:158-161   handlers.demuxByProto(etype): the first
                                       registered EtherType (definitions.go:98-106)
  internet/stack-ip4.go:135-170        nodeByProto(proto), then
                                       node.callbacks.Demux(frame[:totalLen], off)
  internet/stack-ip6.go:107-141        the same with frame[:40 + pl], offset 40
  internet/stack-ports.go:25-31        dstPortOff = 2 for TCP and UDP
  internet/stack-ports.go:64-67        dstPortOff + offset + 2 > len(b) -> io.ErrShortBuffer
  internet/stack-ports.go:68-69        port = be16(b[off + 2:]); demuxByPort
  internet/definitions.go:108-116      nodeByPort: the FIRST node with that lport
  internet/definitions.go:141-145      none -> ErrPacketDrop
  internet/stack-ports.go:70-82        TCP, offset + 14 <= len(b): flags =
                                       be16(b[off + 12:]) & 0x1ff; SYN without RST / ACK
                                       queues a RST unless GetIPAddr fails
  internal/ip.go:9-27                  GetIPAddr fails only for a version nibble
                                       other than 4 / 6

The receive verdict it starts from is oracle.ingress_verdict with
oracle.StackFilter.  No Go toolchain is available to this suite, so the
restatement is pinned by these citations and by the hand-worked cases of
tests/test_deliver.py (as tests/test_pcap.py does for the capture rules), not
by running the reference.

The frame builders stand on tests/framegen.py's ether / ipv4 / ipv6 / udp /
icmp.  A TCP segment too short to hold its checksum field still has to verify
(demux4 / demux6 sum whatever the IP lengths say): ``solved4`` / ``solved6``
put the segment's checksum into a word of the source address instead."""
from __future__ import annotations

import struct

import numpy as np

from oracle import oracle as O
from tests import framegen as G

H_ETH, H_IP4, H_IP6, H_TCP, H_UDP, H_COUNT, H_NONE = 0, 16, 272, 528, 800, 1057, 0xFFFF
DLV_RST, DLV_IP6, DLV_FCS = 1, 2, 4
ERR_SHORT_BUFFER = 6  # the library's number for io.ErrShortBuffer (lnx_fcs_append)
VERIFY_FLAGS = O.VERIFY_ICMP  # every receive verdict of these tests is taken with the ICMP checks on

FILTER_KW = dict(ethertypes=(0x0800, 0x86DD, 0x0806, 0x88CC), ip4=G.IP4_DST, ip6=G.IP6_DST)


def _be16(b: bytes, o: int) -> int:
    return (b[o] << 8) | b[o + 1]


def deliver(frame: bytes, v_in: int, ethertypes=None, ports=None, fcs_ok=None):
    """(record dict, outcome tag).  ethertypes: the filter's EtherTypes in
    registration order, None for the accept-all filter.  ports: (tcp list, udp
    list) or None (every port has a handler).  fcs_ok: None for no FCS result."""
    rec = dict(ip_end=0, handler=H_NONE, l4_off=0, src_port=0, dst_port=0, verdict=0, flags=0, zero=0)
    cut = dict(rec, verdict=O.ERR_TRUNCATED_FRAME)
    L = len(frame)
    if fcs_ok is not None and not fcs_ok:                          # rule 1
        return dict(rec, verdict=O.ERR_BAD_CRC, flags=DLV_FCS), "fcs"
    if v_in != 0:                                                  # rule 2
        return dict(rec, verdict=v_in), "vin"
    if L < 14:                                                     # rule 6
        return cut, "cut"
    et = _be16(frame, 12)
    if et not in (0x0800, 0x86DD):                                 # rule 3 (stack-ethernet.go:158-161)
        if ethertypes is None:
            return dict(rec, handler=H_ETH + 8), "eth_any"
        if et in ethertypes:
            return dict(rec, handler=H_ETH + list(ethertypes).index(et)), "eth_slot"   # index(): the first match
        return dict(rec, verdict=O.ERR_PACKET_DROP), "eth_none"
    if et == 0x0800:                                               # rule 4 (stack-ip4.go:135-170)
        if L < 24:
            return cut, "cut"
        rec["l4_off"] = 14 + 4 * (frame[14] & 15)
        rec["ip_end"] = 14 + _be16(frame, 16)
        proto = frame[23]
    else:                                                          # stack-ip6.go:107-141
        if L < 21:
            return cut, "cut"
        rec["l4_off"] = 54
        rec["ip_end"] = 54 + _be16(frame, 18)
        proto = frame[20]
        rec["flags"] = DLV_IP6
    if rec["ip_end"] > L:                                          # rule 6: frame[14:ip_end] would not exist
        return cut, "cut"
    if proto not in (6, 17):
        return dict(rec, handler=(H_IP4 if et == 0x0800 else H_IP6) + proto), "ip_other"
    b, off = frame[14:rec["ip_end"]], rec["l4_off"] - 14           # what StackPorts.Demux(b, offset) gets
    if 2 + off + 2 > len(b):                                       # stack-ports.go:65-67
        return dict(rec, verdict=ERR_SHORT_BUFFER), "short"
    rec["src_port"], rec["dst_port"] = _be16(b, off), _be16(b, off + 2)
    table = None if ports is None else ports[0 if proto == 6 else 1]
    base = H_TCP if proto == 6 else H_UDP
    if table is None:
        return dict(rec, handler=base + 256), "hit_any"
    if rec["dst_port"] in table:                                   # nodeByPort (definitions.go:108-116)
        return dict(rec, handler=base + list(table).index(rec["dst_port"])), "hit"
    rec["verdict"] = O.ERR_PACKET_DROP                             # definitions.go:141-145
    if proto == 6 and off + 14 <= len(b):                          # stack-ports.go:70-82
        fl = _be16(b, off + 12) & 0x01FF
        if fl & 0x02 and not fl & (0x04 | 0x10) and b[0] >> 4 in (4, 6):   # internal/ip.go:9-27
            rec["flags"] |= DLV_RST
            return rec, "miss_rst"
    return rec, "miss"


# ------------------------------------------------------------------ frames
def tcp_seg(sport: int, dport: int, flags: int, payload: bytes = b"") -> bytes:
    """A 20-byte TCP header (data offset 5) with the 9 flag bits of ``flags``."""
    return struct.pack(">HHIIHHHH", sport, dport, 0x4060D5CC, 0, 0x5000 | (flags & 0x1FF), 0xFAF0, 0, 0) + payload


def udp_dgram(sport: int, dport: int, payload: bytes) -> bytes:
    return struct.pack(">HH", sport, dport) + G.udp(payload)[4:]


def solved4(l4: bytes, opts: bytes = b"") -> bytes:
    """Ethernet + IPv4 + a TCP segment of ANY length whose sum verifies: the low
    word of the source address takes the checksum (it is summed in the
    pseudo-header), then the header sum is redone."""
    ip = bytearray(G.ipv4(6, l4, opts=opts, fix_l4=False))
    ip[14:16] = b"\0\0"
    ip[14:16] = struct.pack(">H", O.ipv4_tcp_pseudo(bytes(ip)).payload_sum16(bytes(l4)))
    ip[10:12] = b"\0\0"
    ip[10:12] = struct.pack(">H", O.ipv4_header_sum16(bytes(ip)))
    return G.ether(0x0800, bytes(ip))


def solved6(l4: bytes, hop: int = 64) -> bytes:
    ip = bytearray(G.ipv6(6, l4, fix_l4=False))
    ip[7] = hop
    ip[22:24] = b"\0\0"
    ip[22:24] = struct.pack(">H", O.ipv6_pseudo(bytes(ip)).payload_sum16(bytes(l4)))
    return G.ether(0x86DD, bytes(ip))


# the port tables of the settings below
TCP_FULL = [1000 + i for i in range(256)]
UDP_FULL = [2000 + i for i in range(256)]
TCP_PORTS = (1000, 1100, 1255, 80, 0, 9)   # k = 0, a middle k, k = 255 of the full table; the duplicate; port 0; a miss
UDP_PORTS = (2000, 2100, 2255, 53, 0, 9)
# (name, filter on, ports)
SETTINGS = [
    ("null_null", False, None),
    ("filt_null", True, None),
    ("null_empty", False, ([], [])),
    ("filt_full", True, (TCP_FULL, UDP_FULL)),
    ("filt_dup", True, ([7, 80, 80, 443], [53, 53, 67])),
    ("null_port0", False, ([22, 0, 80], [0, 53])),
]
TCP_VARIANTS = {"psh": 0x018, "syn": 0x002, "synack": 0x012, "synrst": 0x006, "ack": 0x010, "syn8": 0x102,
                # SYN, RST and ACK all clear: the SYN term of the RST condition negated alone
                "null": 0x000, "fin": 0x001, "pshonly": 0x008}
NO_SYN_ALONE = ("null", "fin", "pshonly")
REPS = 16  # a third of the cases end at a bad FCS (fcs_choice): at least 8 of each are left


def census_frames(seed: int = 1717) -> list[tuple[str, bytes]]:
    """(label, frame) pairs, FCS stripped; labels are ``kind/variant/port``."""
    rng = np.random.default_rng(seed)
    out: list[tuple[str, bytes]] = []

    def pay(lo=0, hi=40):
        return rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()

    def wrap(ver, proto, l4, opts=b""):
        return G.ether(0x0800, G.ipv4(proto, l4, opts=opts)) if ver == 4 else G.ether(0x86DD, G.ipv6(proto, l4))

    for ver in (4, 6):
        for rep in range(REPS):
            sport = 1024 + int(rng.integers(0, 60000))
            opts = bytes(4 * (rep % 3)) if ver == 4 else b""
            for port in TCP_PORTS:
                for var in ("psh", "syn"):
                    out.append((f"tcp{ver}/{var}/{port}", wrap(ver, 6, tcp_seg(sport, port, TCP_VARIANTS[var], pay()), opts)))
            for var in ("synack", "synrst", "ack", "syn8") + NO_SYN_ALONE:
                out.append((f"tcp{ver}/{var}/9", wrap(ver, 6, tcp_seg(sport, 9, TCP_VARIANTS[var], pay()), opts)))
            # P = 13 against P = 14: the flags word is the segment's last two bytes
            syn14 = tcp_seg(sport, 9, 0x002)[:14]
            solve = (lambda l4: solved4(l4, opts)) if ver == 4 else (lambda l4: solved6(l4, 64 + rep))
            out.append((f"tcp{ver}/p14/9", solve(syn14)))
            out.append((f"tcp{ver}/p13/9", solve(syn14[:13])))
            out.append((f"tcp{ver}/p14/1000", solve(tcp_seg(sport, 1000, 0x002)[:14])))
            for p in range(4):  # no destination port in the segment: io.ErrShortBuffer
                out.append((f"tcp{ver}/short{p}/-", solve(tcp_seg(sport, 9, 0x002)[:p])))
            for port in UDP_PORTS:
                out.append((f"udp{ver}/dgram/{port}", wrap(ver, 17, udp_dgram(sport, port, pay()), opts)))
            if ver == 6:  # demux6 never looks at the version nibble; GetIPAddr does
                for nib in (4, 6, 5):
                    f = bytearray(wrap(6, 6, tcp_seg(sport, 9, 0x002, pay())))
                    f[14] = (nib << 4) | (f[14] & 15)
                    out.append((f"tcp6/nib{nib}/9", bytes(f)))
            # other protocols: ICMP (checked under VERIFY_ICMP), GRE (no handler under the filter)
            icmp = G.icmp(8 if ver == 4 else 128, pay(0, 32), seq=rep)
            out.append((f"icmp{ver}/echo/-", wrap(ver, 1 if ver == 4 else 58, icmp, opts)))
            out.append((f"gre{ver}/any/-", wrap(ver, 47, pay(4, 32), opts)))
    for rep in range(REPS):
        out.append(("eth/arp/-", G.ether(0x0806, pay(28, 46))))
        out.append(("eth/lldp/-", G.ether(0x88CC, pay(10, 46))))
        out.append(("eth/vlan/-", G.ether(0x8100, pay(4, 46))))       # no handler under the filter
        out.append(("eth/len46/-", G.ether(46, pay(46, 60))))         # an 802.3 length: never registered
    # the suite's generic mixes: broken sums, bad lengths, trailing bytes (most verdicts non-zero)
    out += [("mix/frames/-", f) for f in G.frames(seed=seed, count=400)]
    out += [("mix/trailing/-", f) for f in G.trailing_frames(seed=seed, count=100)]
    out += [("mix/icmp/-", f) for f in G.icmp_frames(seed=seed, count=100)]
    return out


def truncation_wholes() -> list[tuple[str, bytes]]:
    """Valid TCP / UDP frames longer than 74 bytes: cut at every length 0..74 and
    paired with a zero verdict they are the inconsistent inputs of rule 6."""
    p = bytes(range(40))
    return [("tcp4opt", G.ether(0x0800, G.ipv4(6, tcp_seg(4000, 1000, 0x002, p[:10]), opts=bytes(range(1, 41))))),
            ("udp4", G.ether(0x0800, G.ipv4(17, udp_dgram(4000, 2000, p)))),
            ("tcp6", G.ether(0x86DD, G.ipv6(6, tcp_seg(4000, 1000, 0x002, p[:10])))),
            ("udp6", G.ether(0x86DD, G.ipv6(17, udp_dgram(4000, 2000, p))))]


def truncation_sweep() -> list[tuple[str, bytes]]:
    return [(f"{name}/cut{n}", whole[:n]) for name, whole in truncation_wholes() for n in range(75)]


def ofilter(on: bool):
    return O.StackFilter(mac=G.MAC_US, **FILTER_KW) if on else None


def fcs_choice(i: int, j: int):
    """The FCS result of frame i under setting j: none, good, bad by turns."""
    return (None, 1, 0)[(i + j) % 3]
