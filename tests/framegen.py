"""Synthetic Ethernet/IPv4/IPv6/TCP/UDP frames with valid or broken checksums,
shaped like lneto's own test generators (internal/ltesto/ltesto.go:99-135,209-228:
Ethernet + IPv4 (IHL 5) + TCP/UDP with the checksums filled in), widened with IP
options, IPv6, other protocols and the malformed cases demux4 / demux6 reject.

Checksum fields are filled with the oracle restatement of crc.go / ipv4/frame.go /
ipv6/frame.go (tests/test_oracle.py pins it on lneto_test.go:119-160)."""
from __future__ import annotations

import struct

import numpy as np

from oracle import oracle as O


def ether(et: int, payload: bytes) -> bytes:
    return bytes.fromhex("c0ffee00dead") + bytes.fromhex("4e8b3af9fb6b") + struct.pack(">H", et) + payload


IP4_DST = bytes([192, 168, 10, 2])
IP6_DST = bytes(range(0x30, 0x40))


def ipv4(proto: int, l4: bytes, opts: bytes = b"", flags: int = 0x4000, fix_l4: bool = True,
         dst: bytes = IP4_DST) -> bytes:
    ihl = 5 + len(opts) // 4
    tl = ihl * 4 + len(l4)
    hdr = bytearray(struct.pack(">BBHHHBBH4s4s", 0x40 | ihl, 0, tl, 0x1234, flags, 64, proto, 0,
                                bytes([192, 168, 10, 1]), dst)) + opts
    hdr[10:12] = struct.pack(">H", O.ipv4_header_sum16(bytes(hdr)))  # covers 20 bytes only
    l4 = bytearray(l4)
    if fix_l4 and proto == O.IPPROTO_TCP and len(l4) >= 18:
        l4[16:18] = b"\0\0"
        l4[16:18] = struct.pack(">H", O.ipv4_tcp_pseudo(bytes(hdr)).payload_sum16(bytes(l4)))
    if fix_l4 and proto == O.IPPROTO_ICMP and len(l4) >= 8:  # no pseudo-header (ltesto.go:224-227)
        l4[2:4] = b"\0\0"
        l4[2:4] = struct.pack(">H", O.CRC791().payload_sum16(bytes(l4)))
    if fix_l4 and proto == O.IPPROTO_UDP and len(l4) >= 8:
        ul = struct.unpack(">H", l4[4:6])[0]
        l4[6:8] = b"\0\0"
        if ul <= len(l4):
            l4[6:8] = struct.pack(">H", O.ipv4_udp_pseudo(bytes(hdr), ul).payload_sum16(bytes(l4[:ul])))
    return bytes(hdr) + bytes(l4)


def ipv6(proto: int, l4: bytes, fix_l4: bool = True, dst: bytes = IP6_DST) -> bytes:
    hdr = bytearray(struct.pack(">IHBB", 0x60000000, len(l4), proto, 64)) + bytes(range(0x20, 0x30)) + dst
    l4 = bytearray(l4)
    if fix_l4 and proto == O.IPPROTO_TCP and len(l4) >= 18:
        l4[16:18] = b"\0\0"
        l4[16:18] = struct.pack(">H", O.ipv6_pseudo(bytes(hdr)).payload_sum16(bytes(l4)))
    if fix_l4 and proto == O.IPPROTO_ICMPV6 and len(l4) >= 8:  # ipv6/icmpv6/client.go:141-148
        l4[2:4] = b"\0\0"
        l4[2:4] = struct.pack(">H", O.ipv6_pseudo(bytes(hdr)).payload_sum16(bytes(l4)))
    if fix_l4 and proto == O.IPPROTO_UDP and len(l4) >= 8:
        l4[6:8] = b"\0\0"  # the stack sums the whole payload (stack-ip6.go:133-134)
        l4[6:8] = struct.pack(">H", O.ipv6_pseudo(bytes(hdr)).payload_sum16(bytes(l4)))
    return bytes(hdr) + bytes(l4)


def tcp(payload: bytes) -> bytes:
    return struct.pack(">HHIIBBHHH", 0xE70A, 80, 0x4060D5CC, 0, 0x50, 0x18, 0xFAF0, 0, 0) + payload


def udp(payload: bytes, length: int | None = None) -> bytes:
    ul = 8 + len(payload) if length is None else length
    return struct.pack(">HHHH", 5353, 53, ul, 0) + payload


def icmp(type_: int, payload: bytes, ident: int = 0x1234, seq: int = 1) -> bytes:
    """An ICMPv4 / ICMPv6 message with an echo-shaped header (type, code 0,
    checksum, identifier, sequence number); ipv4() / ipv6() fill the checksum."""
    return struct.pack(">BBHHH", type_, 0, 0, ident, seq) + payload


def ltesto_icmp_echo(payload: bytes, ident: int, seq: int) -> bytes:
    """ltesto.PacketGen.AppendIPv4ICMPEcho (internal/ltesto/ltesto.go:175-231)
    with the addresses of TestStackAsync_ICMPEchoChecksum
    (x/xnet/xnet_test.go:1015-1045): IHL 5, ID 0, flags 0, TTL 64, protocol
    ICMP, header CRC; echo request (type 8, code 0) whose checksum covers the
    whole ICMP message."""
    tl = 20 + 8 + len(payload)
    hdr = bytearray(struct.pack(">BBHHHBBH4s4s", 0x45, 0, tl, 0, 0, 64, O.IPPROTO_ICMP, 0,
                                bytes([192, 168, 1, 1]), bytes([192, 168, 1, 99])))
    hdr[10:12] = struct.pack(">H", O.ipv4_header_sum16(bytes(hdr)))
    msg = bytearray(struct.pack(">BBHHH", 8, 0, 0, ident, seq) + payload)
    msg[2:4] = struct.pack(">H", O.CRC791().payload_sum16(bytes(msg)))
    return bytes([0xAA, 0xBB, 0xCC, 0xDD, 0xEE, 0xFF, 0x00, 0x11, 0x22, 0x33, 0x44, 0x55, 0x08, 0x00]) \
        + bytes(hdr) + bytes(msg)


def icmp_frames(seed: int = 3, count: int = 1200) -> list[bytes]:
    """ICMPv4 / ICMPv6 frames for the ICMP clients' checks (LNX_VERIFY_ICMP):
    echo and echo reply, other types (ICMPv4 drops them before the sum), one
    flipped byte, messages under 8 bytes, trailing bytes past tl / pl + 40
    (ignored), IPv4 options, and a broken IPv4 header in front of a non-echo
    type (the header sum comes first)."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        pay = rng.integers(0, 256, size=int(rng.integers(0, 1400)), dtype=np.uint8).tobytes()
        kind = i % 12
        if kind in (0, 1):
            f = ether(0x0800, ipv4(1, icmp(8 if kind == 0 else 0, pay)))
        elif kind == 2:
            f = ether(0x0800, ipv4(1, icmp(int(rng.choice([3, 5, 11, 13, 14, 42, 255])), pay)))
        elif kind == 3:
            b = bytearray(ether(0x0800, ipv4(1, icmp(8, pay))))
            b[int(rng.integers(34, len(b)))] ^= 1 << int(rng.integers(0, 8))
            f = bytes(b)
        elif kind == 4:
            f = ether(0x0800, ipv4(1, rng.integers(0, 256, size=int(rng.integers(0, 8)), dtype=np.uint8).tobytes()))
        elif kind == 5:
            f = ether(0x0800, ipv4(1, icmp(0, pay))) + bytes.fromhex("deadbeef")
        elif kind == 6:
            f = ether(0x86DD, ipv6(58, icmp(int(rng.choice([1, 128, 129, 135, 136, 200])), pay)))
        elif kind == 7:
            b = bytearray(ether(0x86DD, ipv6(58, icmp(128, pay))))
            b[int(rng.integers(54, len(b)))] ^= 1 << int(rng.integers(0, 8))
            f = bytes(b)
        elif kind == 8:
            f = ether(0x86DD, ipv6(58, rng.integers(0, 256, size=int(rng.integers(0, 8)), dtype=np.uint8).tobytes()))
        elif kind == 9:
            f = ether(0x86DD, ipv6(58, icmp(129, pay))) + rng.integers(1, 256, size=20, dtype=np.uint8).tobytes()
        elif kind == 10:
            b = bytearray(ether(0x0800, ipv4(1, icmp(3, pay))))
            b[22] ^= 0x01  # TTL
            f = bytes(b)
        else:
            f = ether(0x0800, ipv4(1, icmp(8, pay), opts=bytes(4 * int(rng.integers(1, 11)))))
        out.append(f)
    return out


def short_tcp6(rng) -> bytes:
    """0..7 payload bytes under IPv6 next-header TCP; demux6 does no size check
    for TCP (internet/stack-ip6.go:116-121), so the verdict is the sum alone.
    Half of the >= 2-byte ones carry their own checksum in the first word."""
    raw = bytearray(rng.integers(0, 256, size=int(rng.integers(0, 8)), dtype=np.uint8).tobytes())
    if len(raw) >= 2 and rng.integers(0, 2):
        hdr = struct.pack(">IHBB", 0x60000000, len(raw), O.IPPROTO_TCP, 64) + bytes(range(0x20, 0x40))
        raw[0:2] = b"\0\0"
        raw[0:2] = struct.pack(">H", O.ipv6_pseudo(hdr).payload_sum16(bytes(raw)))
    return bytes(raw)


def trailing_frames(seed: int = 7, count: int = 600) -> list[bytes]:
    """Frames whose transport data ends before the frame does, followed by
    non-zero bytes the receive path must ignore: IPv4 TCP / UDP with bytes past
    tl (internet/stack-ip4.go:100-107 slices the frame to tl), IPv4 UDP whose
    UDP length is below the IP payload (the sum covers ufrm.RawData()[:Length()],
    stack-ip4.go:161-163), and IPv6 with bytes past pl + 40 (ipv6 payload is
    sliced by PayloadLength, stack-ip6.go:86-138).  Transport payloads of
    150-1200 B so the ignored bytes land in the middle of a row's batch;
    a third of the frames carry one flipped byte inside the covered range."""
    rng = np.random.default_rng(seed)
    out = []
    for i in range(count):
        n = int(rng.integers(150, 1200))
        pay = rng.integers(0, 256, size=n, dtype=np.uint8).tobytes()
        tail = (rng.integers(1, 256, size=int(rng.integers(16, 300)), dtype=np.uint8)).tobytes()
        kind = i % 5
        if kind == 0:
            f = ether(0x0800, ipv4(6, tcp(pay))) + tail
        elif kind == 1:
            f = ether(0x0800, ipv4(17, udp(pay))) + tail
        elif kind == 2:  # UDP length < IP payload: the rest of the IP payload is outside the sum
            ul = 8 + int(rng.integers(0, n))
            f = ether(0x0800, ipv4(17, udp(pay, length=ul)))
        elif kind == 3:
            f = ether(0x86DD, ipv6(6, tcp(pay))) + tail
        else:
            f = ether(0x86DD, ipv6(17, udp(pay))) + tail
        if i % 3 == 0:
            b = bytearray(f)
            end = 14 + (struct.unpack(">H", b[16:18])[0] if kind < 3 else 40 + struct.unpack(">H", b[18:20])[0])
            if kind == 2:
                end = 14 + 20 + struct.unpack(">H", b[38:40])[0]
            b[int(rng.integers(min(60, end - 1), end))] ^= 0x04
            f = bytes(b)
        out.append(f)
    return out


def frames(seed: int = 1, count: int = 3000) -> list[bytes]:
    """A mixed batch: valid frames of every kind plus every malformation the
    receive path distinguishes, with random payload sizes (odd ones too)."""
    rng = np.random.default_rng(seed)

    def pay(lo=0, hi=1400):
        return rng.integers(0, 256, size=int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()

    out = []
    for i in range(count):
        kind = i % 24
        if kind == 0:
            f = ether(0x0800, ipv4(6, tcp(pay())))
        elif kind == 1:
            f = ether(0x0800, ipv4(17, udp(pay())))
        elif kind == 2:  # IP options: the header sum still covers 20 bytes only (ipv4/frame.go:144-146)
            f = ether(0x0800, ipv4(6, tcp(pay()), opts=bytes(4 * int(rng.integers(1, 11)))))
        elif kind == 3 and (i // 24) % 2:  # IPv6 TCP shorter than a TCP header: demux6 sums it anyway
            f = ether(0x86DD, ipv6(6, short_tcp6(rng)))
        elif kind == 3:
            f = ether(0x86DD, ipv6(6, tcp(pay())))
        elif kind == 4:
            f = ether(0x86DD, ipv6(17, udp(pay())))
        elif kind == 5:  # corrupted payload byte
            b = bytearray(ether(0x0800, ipv4(int(rng.choice([6, 17])), tcp(pay(1)))))
            b[int(rng.integers(34, len(b)))] ^= 1 << int(rng.integers(0, 8))
            f = bytes(b)
        elif kind == 6:  # corrupted IPv4 header byte (not the length/version fields)
            b = bytearray(ether(0x0800, ipv4(6, tcp(pay()))))
            b[int(rng.choice([15, 18, 19, 22, 26, 27, 30, 33]))] ^= 0x10
            f = bytes(b)
        elif kind == 7:  # corrupted IPv6 payload
            b = bytearray(ether(0x86DD, ipv6(int(rng.choice([6, 17])), udp(pay(1)))))
            b[int(rng.integers(54, len(b)))] ^= 0x80
            f = bytes(b)
        elif kind == 8:  # UDP checksum 0 on IPv4: NOT special-cased by the stack (stack-ip4.go:152-167)
            b = bytearray(ether(0x0800, ipv4(17, udp(pay()))))
            b[40:42] = b"\0\0"
            f = bytes(b)
        elif kind == 9:  # other IP protocols: no transport sum
            f = ether(0x0800, ipv4(1, pay(8)))
        elif kind == 10:
            f = ether(0x86DD, ipv6(58, pay(8)))
        elif kind == 11:  # truncated total length: tl > buffer
            b = bytearray(ether(0x0800, ipv4(6, tcp(pay()))))
            b = b[: int(rng.integers(34, len(b)))]
            f = bytes(b)
        elif kind == 12:  # trailing bytes past tl (Ethernet padding): ignored
            f = ether(0x0800, ipv4(17, udp(pay(0, 10)))) + bytes(int(rng.integers(1, 30)))
        elif kind == 13:  # bad IHL / tl / version fields
            b = bytearray(ether(0x0800, ipv4(6, tcp(pay()))))
            m = int(rng.integers(0, 4))
            if m == 0:
                b[14] = 0x40 | int(rng.integers(0, 5))   # ihl < 5
            elif m == 1:
                b[16:18] = struct.pack(">H", int(rng.integers(0, 20)))  # tl < 20
            elif m == 2:
                b[14] = 0x60 | (b[14] & 15)              # version 6
            else:
                b[14] = 0x4F                             # ihl*4 = 60 > tl possibly
            f = bytes(b)
        elif kind == 14:  # evil bit (only rejected with VERIFY_EVIL_BIT)
            f = ether(0x0800, ipv4(6, tcp(pay()), flags=0x2000))
        elif kind == 15:  # UDP length field broken
            ul = int(rng.choice([0, 3, 7, 9000]))
            f = ether(0x0800, ipv4(17, udp(pay(), length=ul)))
        elif kind == 16:  # IPv6 payload length too large / UDP too short
            b = bytearray(ether(0x86DD, ipv6(17, udp(pay(0, 6)))))
            if rng.integers(0, 2):
                b[18:20] = struct.pack(">H", len(b))
            else:
                b = b[: 14 + 40 + int(rng.integers(0, 8))]
                b[18:20] = struct.pack(">H", len(b) - 54)
            f = bytes(b)
        elif kind == 17:  # short frames
            f = pay(0, 60)
        elif kind == 18:  # VLAN, size-type, ARP EtherTypes
            et = int(rng.choice([0x8100, 0x0806, 46, 1500, 0x88CC]))
            f = ether(et, pay(0, 100))
            if et == 0x8100 and rng.integers(0, 2):
                f = f[: int(rng.integers(14, 18))]
        elif kind == 19:  # IPv4 with a UDP payload shorter than the UDP header
            f = ether(0x0800, ipv4(17, pay(0, 8), fix_l4=False))
        elif kind == 20:  # random bytes behind IPv4 / IPv6 EtherTypes
            f = ether(int(rng.choice([0x0800, 0x86DD])), pay(0, 200))
        elif kind == 21:  # odd-length TCP segment (trailing byte weighted << 8)
            f = ether(0x0800, ipv4(6, tcp(pay(1, 50) + b"\x7f")))
        elif kind == 22:  # jumbo-ish
            f = ether(0x0800, ipv4(6, tcp(pay(3000, 8900))))
        else:  # minimum-size frame with Ethernet padding
            f = ether(0x0800, ipv4(17, udp(b"")))
            f = f + bytes(max(0, 60 - len(f)))
        out.append(f)
    return out


MAC_US = bytes.fromhex("c0ffee00dead")  # ether()'s destination: the stack's own MAC in filter_frames


def filter_frames(seed: int = 21, count: int = 2400) -> list[bytes]:
    """Frames for the stack filter (lnx_rx_filter / oracle.StackFilter): every
    destination class at each layer (the stack's MAC / broadcast / another
    unicast MAC / a multicast MAC; the stack's IPv4 address / another / 224/4 /
    255.255.255.255; the stack's IPv6 address / another / ff02::1), EtherTypes
    and IP protocols with and without a handler, crossed with broken sums and
    sizes, so a frame the stack would drop also carries an error that a later
    check would report (the precedence is the test)."""
    rng = np.random.default_rng(seed)
    macs = [MAC_US, b"\xff" * 6, bytes.fromhex("02aabbccddee"), bytes.fromhex("01005e000001")]
    ip4s = [IP4_DST, bytes([192, 168, 10, 77]), bytes([224, 0, 0, 251]), b"\xff" * 4]
    ip6s = [IP6_DST, bytes(range(0x50, 0x60)), bytes.fromhex("ff020000000000000000000000000001")]
    out = []
    for i in range(count):
        pay = rng.integers(0, 256, size=int(rng.integers(0, 600)), dtype=np.uint8).tobytes()
        fam = i % 5
        if fam in (0, 1):
            proto = int(rng.choice([6, 17, 1, 47]))
            l4 = tcp(pay) if proto == 6 else udp(pay) if proto == 17 else icmp(8, pay) if proto == 1 else pay
            f = ether(0x0800, ipv4(proto, l4, dst=ip4s[int(rng.integers(0, 4))]))
        elif fam in (2, 3):
            proto = int(rng.choice([6, 17, 58, 47]))
            l4 = tcp(pay) if proto == 6 else udp(pay) if proto == 17 else icmp(128, pay) if proto == 58 else pay
            f = ether(0x86DD, ipv6(proto, l4, dst=ip6s[int(rng.integers(0, 3))]))
        else:
            et = int(rng.choice([0x0806, 0x88CC, 0x8100, 46]))
            f = ether(et, pay + bytes(46))
        b = bytearray(f)
        b[0:6] = macs[int(rng.choice(4, p=[0.55, 0.15, 0.15, 0.15]))]
        r = rng.random()
        if r < 0.2 and len(b) > 34:          # a broken sum somewhere past the Ethernet header
            b[int(rng.integers(14, len(b)))] ^= 1 << int(rng.integers(0, 8))
        elif r < 0.27:                       # a size error
            b = b[: int(rng.integers(14, max(15, len(b) - 1)))]
        out.append(bytes(b))
    return out


def _udp6_pcap(proto: int, pay: bytes, extra: bytes = b"") -> bytes:
    """An IPv6 UDP / UDPLite packet whose checksum covers the UDP length only,
    as pcap sums it (internet/pcap/capture.go:184-198), followed by `extra`
    bytes inside the IPv6 payload but outside the UDP length."""
    l4 = bytearray(udp(pay)) + extra
    hdr = bytearray(struct.pack(">IHBB", 0x60000000, len(l4), proto, 64)) + bytes(range(0x20, 0x30)) + IP6_DST
    ul = 8 + len(pay)
    l4[6:8] = struct.pack(">H", O.ipv6_pseudo(bytes(hdr)).payload_sum16(bytes(l4[:ul])))
    return bytes(hdr) + bytes(l4)


def pcap_frames(seed: int = 31, count: int = 2400) -> list[bytes]:
    """Frames for pcap's checksum re-verification (oracle.pcap_checksums):
    the receive-path mix (frames()) plus what pcap treats differently — a bad
    IPv4 header sum in front of a good / bad transport sum, IPv4 UDP with a
    zero checksum, ICMPv4 of any type (good / flipped), IPv6 UDP and UDPLite
    summed over the UDP length with bytes after it, TCP data offsets below 5 or
    past the payload, IPv4 TCP payloads under 20 bytes and UDP under 8."""
    rng = np.random.default_rng(seed)

    def pay(lo=0, hi=1400):
        return rng.integers(0, 256, size=int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()

    def flip(f: bytes, lo: int, hi: int | None = None) -> bytes:
        b = bytearray(f)
        b[int(rng.integers(lo, len(b) if hi is None else hi))] ^= 1 << int(rng.integers(0, 8))
        return bytes(b)

    out = []
    base = frames(seed=seed + 1, count=count // 2)
    for i in range(count - len(base)):
        kind = i % 12
        if kind == 0:    # bad header sum (TTL / ID byte), transport good
            f = flip(ether(0x0800, ipv4(int(rng.choice([1, 6, 17])), tcp(pay()))), 18, 24)
        elif kind == 1:  # bad header sum and bad transport sum
            f = flip(flip(ether(0x0800, ipv4(6, tcp(pay(1)))), 22, 23), 34)
        elif kind == 2:  # IPv4 UDP with checksum 0: not checked, whatever the payload
            b = bytearray(flip(ether(0x0800, ipv4(17, udp(pay(1)))), 42))
            b[40:42] = b"\0\0"
            f = bytes(b)
        elif kind == 3:  # ICMPv4 of any type, good or flipped
            f = ether(0x0800, ipv4(1, icmp(int(rng.integers(0, 256)), pay())))
            if rng.integers(0, 2):
                f = flip(f, 34)
        elif kind == 4:  # ICMPv4 under 8 bytes: icmpv4.NewFrame refuses it, no check
            f = ether(0x0800, ipv4(1, pay(0, 8), fix_l4=False))
        elif kind == 5:  # IPv6 UDP / UDPLite over the UDP length, bytes after it
            f = ether(0x86DD, _udp6_pcap(int(rng.choice([17, 136])), pay(), pay(0, 40)))
            if rng.integers(0, 2):
                f = flip(f, 54, 54 + 8 + ((f[58] << 8) | f[59]) - 8)
        elif kind == 6:  # IPv6 UDPLite / UDP size errors
            b = bytearray(ether(0x86DD, _udp6_pcap(int(rng.choice([17, 136])), pay(0, 30))))
            m = int(rng.integers(0, 3))
            if m == 0:
                b[58:60] = struct.pack(">H", int(rng.integers(0, 8)))        # ul < 8
            elif m == 1:
                b[58:60] = struct.pack(">H", len(b) - 54 + int(rng.integers(1, 100)))  # ul > pl
            else:
                b = b[:54 + int(rng.integers(0, 8))]                        # pl < 8
                b[18:20] = struct.pack(">H", len(b) - 54)
            f = bytes(b)
        elif kind == 7:  # TCP data offset < 5 or past the payload (the capture ends)
            b = bytearray(ether(0x0800, ipv4(6, tcp(pay(0, 40)))))
            b[46] = (int(rng.integers(0, 5)) if rng.integers(0, 2) else 15) << 4
            f = flip(bytes(b), 22, 23) if rng.integers(0, 2) else bytes(b)
        elif kind == 8:  # IPv4 TCP payload under 20 bytes: tcp.NewFrame refuses it, no check
            f = ether(0x0800, ipv4(6, pay(0, 20), fix_l4=False))
        elif kind == 9:  # IPv4 UDP length errors behind a bad header sum
            f = flip(ether(0x0800, ipv4(17, udp(pay(), length=int(rng.choice([0, 7, 4000]))))), 22, 23)
        elif kind == 10:  # IPv6 TCP, any length from 0 (no NewFrame check there)
            f = ether(0x86DD, ipv6(6, short_tcp6(rng) if rng.integers(0, 2) else tcp(pay())))
            if rng.integers(0, 3) == 0 and len(f) > 54:
                f = flip(f, 54)
        else:            # IPv6 UDP summed the receive path's way (whole payload): pcap's differs
            f = ether(0x86DD, ipv6(17, udp(pay())) + pay(1, 20))
            b = bytearray(f)
            b[18:20] = struct.pack(">H", len(b) - 54)  # the trailing bytes inside pl
            f = bytes(b)
        out.append(f)
    return base + out


# ------------------------------------------------ frames at the 16-bit limits
LIMIT_KINDS4 = ("tcp4", "udp4", "icmp4", "tcp4opt")   # IPv4; tcp4opt: 40 option bytes (IHL 15)
LIMIT_KINDS6 = ("tcp6", "udp6", "icmp6")
LIMIT_TL4 = (65535, 65534, 65533, 32769)              # IPv4 total length
LIMIT_PL6 = (65535, 65534, 32769)                     # IPv6 payload length
LIMIT_FILLS = ("ff", "00", "ff00", "00ff", "rand")
LIMIT_VARIANTS4 = ("flip_last", "flip_first", "trail1", "trail4097", "cut1", "udp_len_plus1", "bad_hdr")
LIMIT_VARIANTS6 = ("flip_last", "flip_first", "trail1", "trail4097", "cut1")


def limit_fill(fill: str, n: int, rng) -> bytes:
    """n payload bytes: all 0xFF / all 0x00 (the even- and odd-offset byte sums
    E and O both at their maximum / minimum), FF 00 / 00 FF repeated (one of
    them at its maximum, the other 0), or random."""
    if fill == "rand":
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()
    unit = {"ff": b"\xff\xff", "00": b"\0\0", "ff00": b"\xff\x00", "00ff": b"\x00\xff"}[fill]
    return (unit * ((n + 1) // 2))[:n]


def _limit_packet(kind: str, n_l4: int, fill: str, rng, fix_l4: bool = True) -> bytes:
    """One Ethernet frame of `kind` whose transport data (header included) has n_l4 bytes."""
    hdr = 20 if kind.startswith("tcp") else 8
    pay = limit_fill(fill, n_l4 - hdr, rng)
    if kind in ("tcp4", "tcp4opt"):
        return ether(0x0800, ipv4(6, tcp(pay), opts=bytes(40) if kind == "tcp4opt" else b"", fix_l4=fix_l4))
    if kind == "udp4":
        return ether(0x0800, ipv4(17, udp(pay), fix_l4=fix_l4))
    if kind == "icmp4":
        return ether(0x0800, ipv4(1, icmp(8, pay), fix_l4=fix_l4))
    if kind == "tcp6":
        return ether(0x86DD, ipv6(6, tcp(pay), fix_l4=fix_l4))
    if kind == "udp6":
        return ether(0x86DD, ipv6(17, udp(pay), fix_l4=fix_l4))
    return ether(0x86DD, ipv6(58, icmp(128, pay), fix_l4=fix_l4))


def _limit_l4_start(kind: str) -> int:
    return 54 if kind.endswith("6") else 74 if kind == "tcp4opt" else 34


def _limit_variant(frame: bytes, kind: str, variant: str) -> bytes:
    """A receive variant of a valid frame (the frame ends where tl / pl + 40 does)."""
    b = bytearray(frame)
    la = _limit_l4_start(kind)
    if variant == "flip_last":        # one bit of the last covered byte
        b[-1] ^= 0x01
    elif variant == "flip_first":     # one bit of the first transport byte
        b[la] ^= 0x01
    elif variant == "trail1":         # non-zero bytes past tl / pl + 40: ignored
        b += b"\xa5"
    elif variant == "trail4097":      # ... the frame is then longer than 64 KiB + 14
        b += bytes(1 + (i * 7) % 255 for i in range(4097))
    elif variant == "cut1":           # tl / pl + 40 one past the frame
        del b[-1]
    elif variant == "udp_len_plus1":  # IPv4 UDP: the UDP length one above the IP payload
        ul = struct.unpack(">H", b[la + 4:la + 6])[0]
        b[la + 4:la + 6] = struct.pack(">H", ul + 1)
    elif variant == "bad_hdr":        # IPv4: a valid transport sum behind a broken header sum (TTL)
        b[22] ^= 0x01
    else:
        raise ValueError(variant)
    return bytes(b)


def _limit_garble(frame: bytes, kind: str, rng) -> bytes:
    """Garbage in every field the transmit checksum step writes."""
    b = bytearray(frame)
    la = _limit_l4_start(kind)
    at = [18] if kind.endswith("6") else [16, 24]
    at += {"tcp": [la + 16], "udp": [la + 4, la + 6], "icm": [la + 2]}[kind[:3]]
    for o in at:
        b[o:o + 2] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
    return bytes(b)


def _limit_zero_sum(kind: str, n_l4: int, fill: str, rng) -> bytes:
    """A frame of `kind` whose transport checksum computes to 0: the last whole
    16-bit word of the transport data is set to the checksum the data has with
    that word (and the checksum field) zero; the field itself is left 0."""
    f = bytearray(_limit_packet(kind, n_l4, fill, rng, fix_l4=False))
    la = _limit_l4_start(kind)
    at = la + (16 if kind.startswith("tcp") else 6)
    w = la + ((n_l4 - 2) & ~1)
    f[at:at + 2] = b"\0\0"
    f[w:w + 2] = b"\0\0"
    g, st = O.tx_checksum(bytes(f))
    assert st == 0
    c = g[at:at + 2]
    f[w:w + 2] = b"\0\0" if c == b"\xff\xff" and kind.startswith("udp") else c  # (NeverZeroSum: the sum was 0 already)
    return bytes(f)


def limit_frames(seed: int = 65535) -> list[tuple[str, bytes]]:
    """(name, frame) pairs at the largest lengths lneto's stack accepts (any IPv4
    total length and IPv6 payload length up to 65535: internet/stack-ip4.go:100-107,
    internet/stack-ip6.go:86-138) with payloads that saturate the checksum
    accumulators.  Deterministic.

    rx/<kind>/<length>/<fill>/asis: every kind (LIMIT_KINDS4 x LIMIT_TL4,
      LIMIT_KINDS6 x LIMIT_PL6) x LIMIT_FILLS, valid; each followed by one
      receive variant of it (LIMIT_VARIANTS4 / LIMIT_VARIANTS6 in rotation, so
      that every variant meets every fill).
    twin/...: a maximum-size TCP frame whose correct checksum is 0x0000 with the
      field 0x0000 and with 0xFFFF (both valid), and maximum-size IPv4 / IPv6
      UDP frames whose sum computes to 0, carrying 0xFFFF (NeverZeroSum).
    tx/<kind>/<L - 14 or L - 54>/<fill>: transmit inputs with garbage in every
      field the step writes, at the largest length the step accepts (every
      fill) and one byte more (status 15, frame untouched; one fill each, in
      rotation); and the zero-sum UDP frames with a garbled checksum field."""
    rng = np.random.default_rng(seed)
    out = []
    for kinds, lengths, variants, extra in ((LIMIT_KINDS4, LIMIT_TL4, LIMIT_VARIANTS4, 20),
                                            (LIMIT_KINDS6, LIMIT_PL6, LIMIT_VARIANTS6, 0)):
        i = 0
        for kind in kinds:
            for length in lengths:
                n_l4 = length - extra - (40 if kind == "tcp4opt" else 0)
                for fill in LIMIT_FILLS:
                    f = _limit_packet(kind, n_l4, fill, rng)
                    out.append((f"rx/{kind}/{length}/{fill}/asis", f))
                    v = variants[(i + i // len(LIMIT_FILLS)) % len(variants)]
                    if v == "udp_len_plus1" and kind != "udp4":
                        v = "bad_hdr"
                    out.append((f"rx/{kind}/{length}/{fill}/{v}", _limit_variant(f, kind, v)))
                    i += 1
    z = _limit_zero_sum("tcp4", 65535 - 20, "ff", rng)
    out.append(("twin/tcp4/65535/sum_0000", z))
    out.append(("twin/tcp4/65535/sum_ffff", z[:50] + b"\xff\xff" + z[52:]))
    zero_udp = []
    for kind, n_l4, at in (("udp4", 65535 - 20, 40), ("udp6", 65535, 60)):
        z = _limit_zero_sum(kind, n_l4, "rand", rng)
        z = z[:at] + b"\xff\xff" + z[at + 2:]
        zero_udp.append((kind, z))
        out.append((f"twin/{kind}/65535/sum_zero", z))
    j = 0
    for kinds, top, extra in ((LIMIT_KINDS4, 65535, 20), (LIMIT_KINDS6, 65535, 0)):
        for kind in kinds:
            n_l4 = top - extra - (40 if kind == "tcp4opt" else 0)
            for fill in LIMIT_FILLS:
                f = _limit_garble(_limit_packet(kind, n_l4, fill, rng, fix_l4=False), kind, rng)
                out.append((f"tx/{kind}/{top}/{fill}", f))
            fill = LIMIT_FILLS[j % len(LIMIT_FILLS)]
            f = _limit_garble(_limit_packet(kind, n_l4, fill, rng, fix_l4=False), kind, rng)
            out.append((f"tx/{kind}/{top + 1}/{fill}", f + limit_fill(fill, 2, rng)[-1:]))
            j += 1
    for kind, z in zero_udp:
        out.append((f"tx/{kind}/65535/sum_zero", _limit_garble(z, kind, rng)))
    return out


# ------------------------------------------------ IPv4 options in front of every transport
OPT_L4 = ("tcp", "udp", "echo", "reply", "icmp3", "p47")   # ICMP echo (type 8), echo reply (0), type 3; protocol 47
OPT_FILLS = ("rand", "ramp", "first", "last")              # the discriminating fills; "ff" beside them for carries
OPT_LENGTHS = (0, 1, 2, 3, 7, 8, 9, 17, 18, 19, 64, 65, 200, 1401)  # transport payload bytes; 4000 once per (IHL, L4)
OPT_VARIANT_LENGTHS = (0, 1, 9, 18, 65, 1401)              # the lengths the variants are crossed with
OPT_PROTO = {"tcp": 6, "udp": 17, "echo": 1, "reply": 1, "icmp3": 1, "p47": 47}


def opt_fill(fill: str, n: int, rng) -> bytes:
    """n option bytes (n = 4 (IHL - 5)).  rand: bytes 1..255; ramp: a non-zero
    ramp; first / last: only that byte non-zero; ff: all 0xFF (carries only: a
    0xFFFF word is one's-complement zero).  rand and ramp are redrawn until
    the options' 16-bit words do not sum to a multiple of 0xFFFF, so that a sum
    which wrongly covers them always differs."""
    if n == 0:
        return b""
    while True:
        if fill == "rand":
            b = rng.integers(1, 256, n, dtype=np.uint8).tobytes()
        elif fill == "ramp":
            k = int(rng.integers(0, 255))
            b = bytes(1 + (k + 7 * i) % 255 for i in range(n))
        elif fill == "first":
            b = bytes([int(rng.integers(1, 256))]) + bytes(n - 1)
        elif fill == "last":
            b = bytes(n - 1) + bytes([int(rng.integers(1, 256))])
        elif fill == "ff":
            return b"\xff" * n
        else:
            raise ValueError(fill)
        if O.sum_write_even(0, b) % 0xFFFF != 0:
            return b


def _opt_l4(l4: str, pay: bytes) -> bytes:
    if l4 == "tcp":
        return tcp(pay)
    if l4 == "udp":
        return udp(pay)
    if l4 == "p47":
        return pay
    return icmp({"echo": 8, "reply": 0, "icmp3": 3}[l4], pay)


def _refix_header(b: bytearray) -> None:
    b[24:26] = b"\0\0"
    b[24:26] = struct.pack(">H", O.ipv4_header_sum16(bytes(b[14:34])))


def ip4_option_frames(seed: int = 4015) -> list[tuple[str, bytes]]:
    """(label, frame) pairs with NON-ZERO IPv4 options in front of every transport
    the checksum kernels know.  The header sum covers 20 bytes whatever the IHL
    (ipv4/frame.go:144-146) and the transport segment starts at 14 + 4 IHL, so
    the option bytes belong to neither sum.  Deterministic.

    rx/<l4>/ihl<k>/<fill>/<n>/valid: OPT_L4 x IHL 5..15 x OPT_FILLS and "ff" x
      OPT_LENGTHS (n transport payload bytes), and n = 4000 once per (IHL, L4).
    rx/<l4>/ihl<k>/<fill>/<n>/<variant>: OPT_L4 x IHL x OPT_VARIANT_LENGTHS, the
      fills of OPT_FILLS in rotation, with
        optflip (one option byte changed: verdict and pcap status as `valid`),
        l4flip, srcflip (pseudo-header), ttl (header sum), ttl+l4flip, trail
        (non-zero bytes past tl), runt (zero-padded to 60 bytes), cut1 (last
        byte missing), cutopt (the frame ends inside the options), tl=hl-1,
        tl=hl (header sum redone), ver5, evil (header sum redone);
        UDP: ulen7, ulenP+1, ulenP+1+ttl, ulen_short (a UDP length below the IP
        payload, non-zero bytes after it), csum0 (checksum field 0);
        TCP: doff4, doff4+ttl, doff15 (the TCP checksum is valid).
    tx/<l4>/ihl<k>/<fill>/<n>/stale: every valid frame of a fill in OPT_FILLS
      with random bytes in the total length, the header CRC, the transport
      checksum and the UDP length.
    tx/udp/ihl<k>/<fill>/18/zero_sum: a UDP datagram behind options whose
      checksum computes to 0 (NeverZeroSum stores 0xFFFF), the field stale.
    tx/<l4>/ihl<k>/...: IHL 0..4 (ihl_low), a frame that ends inside the
      options (cutopt), a transport header too short (short_l4)."""
    rng = np.random.default_rng(seed)
    out = []

    def payload(n):
        return rng.integers(0, 256, n, dtype=np.uint8).tobytes()

    def base(l4, ihl, fill, n, fix=True, evil=False, pay=None):
        opts = opt_fill(fill, 4 * (ihl - 5), rng)
        body = _opt_l4(l4, payload(n) if pay is None else pay)
        return ether(0x0800, ipv4(OPT_PROTO[l4], body, opts=opts, flags=0x2000 if evil else 0x4000, fix_l4=fix))

    def stale(f, l4, ihl):
        b = bytearray(f)
        la = 14 + 4 * ihl
        at = [16, 24] + {"tcp": [la + 16], "udp": [la + 4, la + 6], "p47": []}.get(l4, [la + 2])
        for o in at:
            if o + 2 <= len(b):
                b[o:o + 2] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
        return bytes(b)

    # ---- the valid matrix and its transmit form
    for l4 in OPT_L4:
        for ihl in range(5, 16):
            for fill in OPT_FILLS + ("ff",):
                for n in OPT_LENGTHS + ((4000,) if fill == "rand" else ()):
                    f = base(l4, ihl, fill, n)
                    out.append((f"rx/{l4}/ihl{ihl}/{fill}/{n}/valid", f))
                    if fill != "ff":
                        out.append((f"tx/{l4}/ihl{ihl}/{fill}/{n}/stale", stale(f, l4, ihl)))

    # ---- the receive variants
    rot = 0
    for l4 in OPT_L4:
        hdr = {"tcp": 20, "udp": 8, "p47": 0}.get(l4, 8)
        for ihl in range(5, 16):
            hl, la = 4 * ihl, 14 + 4 * ihl
            for n in OPT_VARIANT_LENGTHS:
                fill = OPT_FILLS[rot % len(OPT_FILLS)]
                rot += 1
                f = base(l4, ihl, fill, n)
                tag = f"rx/{l4}/ihl{ihl}/{fill}/{n}/"

                def put(name, b):
                    out.append((tag + name, bytes(b)))

                if ihl > 5:  # the first, the last or any option byte (the last lies past the staged bytes at IHL 13-15)
                    b = bytearray(f)
                    at = [34, la - 1, int(rng.integers(34, la))][rot % 3]
                    b[at] ^= 1 << int(rng.integers(0, 8))
                    put("optflip", b)
                    put("cutopt", f[:int(rng.integers(35, la))])
                if hdr + n > 0:
                    b = bytearray(f)
                    b[int(rng.integers(la, len(b)))] ^= 1 << int(rng.integers(0, 8))
                    put("l4flip", b)
                    b[22] ^= 0x01
                    put("ttl+l4flip", b)
                b = bytearray(f)
                b[int(rng.integers(26, 30))] ^= 1 << int(rng.integers(0, 8))
                put("srcflip", b)
                b = bytearray(f)
                b[22] ^= 0x01
                put("ttl", b)
                put("trail", f + rng.integers(1, 256, int(rng.integers(1, 31)), dtype=np.uint8).tobytes())
                if len(f) < 60:
                    put("runt", f + bytes(60 - len(f)))
                put("cut1", f[:-1])
                for name, tl in (("tl=hl-1", hl - 1), ("tl=hl", hl)):
                    b = bytearray(f)
                    b[16:18] = struct.pack(">H", tl)
                    _refix_header(b)
                    put(name, b)
                b = bytearray(f)
                b[14] = 0x50 | ihl
                put("ver5", b)
                put("evil", base(l4, ihl, fill, n, evil=True))
                if l4 == "udp":
                    for name, ul in (("ulen7", 7), ("ulenP+1", 8 + n + 1)):
                        b = bytearray(f)
                        b[la + 4:la + 6] = struct.pack(">H", ul)
                        put(name, b)
                    b[22] ^= 0x01
                    put("ulenP+1+ttl", b)
                    if n >= 1:  # the checksum covers ul bytes; what follows them is non-zero and outside it
                        ul = 8 + int(rng.integers(0, n))
                        pay = rng.integers(1, 256, n, dtype=np.uint8).tobytes()
                        opts = opt_fill(fill, 4 * (ihl - 5), rng)
                        put("ulen_short", ether(0x0800, ipv4(17, udp(pay, length=ul), opts=opts)))
                    b = bytearray(f)
                    b[la + 6:la + 8] = b"\0\0"
                    put("csum0", b)
                if l4 == "tcp":
                    for name, doff in (("doff4", 4), ("doff15", 15)):
                        seg = bytearray(tcp(payload(n)))
                        seg[12] = doff << 4
                        b = bytearray(ether(0x0800, ipv4(6, bytes(seg), opts=opt_fill(fill, 4 * (ihl - 5), rng))))
                        put(name, b)
                        if doff == 4:
                            b[22] ^= 0x01
                            put("doff4+ttl", b)

    # ---- the transmit forms that are no valid frame
    for ihl in range(5, 16):
        fill = OPT_FILLS[ihl % len(OPT_FILLS)]
        opts = opt_fill(fill, 4 * (ihl - 5), rng)
        la = 14 + 4 * ihl
        f = bytearray(ether(0x0800, ipv4(17, udp(payload(16) + bytes(2)), opts=opts, fix_l4=False)))
        g, st = O.tx_checksum(bytes(f))
        assert st == 0
        f[-2:] = g[la + 6:la + 8]          # the sum now computes to 0
        f[la + 6:la + 8] = b"\x12\x34"     # and the field is stale
        out.append((f"tx/udp/ihl{ihl}/{fill}/18/zero_sum", bytes(f)))
        for l4 in ("tcp", "udp", "echo"):
            f = stale(base(l4, ihl, fill, 33, fix=False), l4, ihl)
            if ihl > 5:
                out.append((f"tx/{l4}/ihl{ihl}/{fill}/33/cutopt", f[:int(rng.integers(35, la))]))
            short = {"tcp": 20, "udp": 8, "echo": 8}[l4]
            out.append((f"tx/{l4}/ihl{ihl}/{fill}/33/short_l4", f[:la + int(rng.integers(0, short))]))
    for low in range(5):
        for l4 in ("tcp", "udp", "echo"):
            b = bytearray(stale(base(l4, 7, "rand", 40, fix=False), l4, 7))
            b[14] = 0x40 | low
            out.append((f"tx/{l4}/ihl{low}/rand/40/ihl_low", bytes(b)))
    return out


# ------------------------------------------------ near-miss destinations and every protocol value
EDGE_IP4S = {"only_low": bytes([0, 0, 0, 1]), "only_high": bytes([1, 0, 0, 0])}   # stack addresses with one non-zero byte
EDGE_IP6S = {"byte5": bytes(5) + b"\x01" + bytes(10), "byte10": bytes(10) + b"\x80" + bytes(5),
             "byte15": bytes(15) + b"\x01"}
EDGE_ETHERTYPES = (0x0000, 0x0001, 1500, 1501, 0x0800, 0x0806, 0x86DD, 0x8100, 0x88CC, 0x88A8, 0xFFFF) \
    + tuple(0x0F0F * i for i in range(1, 17))   # sixteen spread values between 0x0F0F and 0xF0F0
EDGE_MAC_L4 = ("tcp4", "udp4", "udp6", "arp")


def with_byte(b: bytes, k: int, v: int) -> bytes:
    return b[:k] + bytes([v]) + b[k + 1:]


def _near(b: bytes) -> list[tuple[str, bytes]]:
    """b with each single byte changed: its low bit flipped (^k) and the byte complemented (~k)."""
    return [(f"^{k}", with_byte(b, k, b[k] ^ 0x01)) for k in range(len(b))] \
        + [(f"~{k}", with_byte(b, k, b[k] ^ 0xFF)) for k in range(len(b))]


def edge_macs() -> list[tuple[str, bytes]]:
    """Destination MACs around the two that StackEthernet.Demux accepts (internet/stack-ethernet.go:146-152)."""
    ones = b"\xff" * 6
    out = [("us", MAC_US)] + [("us" + t, m) for t, m in _near(MAC_US)] + [("bcast", ones)]
    out += [(f"bcast.fe{k}", with_byte(ones, k, 0xFE)) for k in range(6)]   # fe:ff:..: no group bit; ..:ff:fe: group bit
    out += [(f"bcast.00{k}", with_byte(ones, k, 0x00)) for k in range(6)]
    return out + [("zero", bytes(6)), ("mc4", bytes.fromhex("01005e000001")), ("mc6", bytes.fromhex("333300000001"))]


def edge_ip4s() -> list[tuple[str, bytes]]:
    """IPv4 destinations around demux4's rules (internet/stack-ip4.go:108-119, ipv4/definitions.go:17-36)."""
    ones = b"\xff" * 4
    out = [("us", IP4_DST)] + [("us" + t, a) for t, a in _near(IP4_DST)] + [("zero", bytes(4))]
    out += [(".".join(map(str, a)), bytes(a)) for a in ((223, 255, 255, 255), (224, 0, 0, 0), (239, 255, 255, 255),
                                                         (240, 0, 0, 0), (254, 255, 255, 255))]
    out += [("bcast", ones)] + [(f"bcast.fe{k}", with_byte(ones, k, 0xFE)) for k in range(4)]
    return out + [(nm, a) for nm, a in EDGE_IP4S.items()]


def edge_ip6s() -> list[tuple[str, bytes]]:
    """IPv6 destinations around demux6's rules (internet/stack-ip6.go:93-98, internal/ip.go:30-38)."""
    out = [("us", IP6_DST)] + [("us" + t, a) for t, a in _near(IP6_DST)] + [("zero", bytes(16))]
    for nm, head in (("ff00::", "ff00"), ("ff02::1", "ff02"), ("fe80::1", "fe80"), ("feff::1", "feff"), ("00ff::1", "00ff")):
        out.append((nm, bytes.fromhex(head) + bytes(13) + bytes([0 if nm == "ff00::" else 1])))
    return out + [(nm, a) for nm, a in EDGE_IP6S.items()]


def filter_edge_frames(seed: int = 146) -> list[tuple[str, bytes]]:
    """(label, frame) pairs for the comparisons behind the stack filter (lnx_rx_filter / oracle.StackFilter):
    destinations one byte away from those the stack accepts, every IP protocol value on both IP versions and
    EtherTypes around the size / type boundary.  Frames of 60-230 B with valid sums unless the variant says
    otherwise, so the destination or handler decision alone sets the verdict; about a fifth carry a broken sum or
    a size error besides, so a wrongly accepted frame shows another code than 0.  Deterministic.

    label = <class>/<case>/<l4>/<variant>/<mac>:
      mac/<case>/<tcp4|udp4|udp6|arp>/..: edge_macs() as the destination MAC (the IP destination is the stack's).
      ip4/<case>/<tcp|udp>.ihl<5|7>/..: edge_ip4s() as the IPv4 destination, without options and behind 8 non-zero
        option bytes (the destination stays at frame offset 30, the transport moves).
      ip6/<case>/<tcp|udp>/..: edge_ip6s() as the IPv6 destination.
      proto4/p<k>/<l4>/.., proto6/p<k>/<l4>/..: every protocol / next-header value 0..255; a correctly summed
        TCP / UDP / ICMP echo / ICMPv6 echo where the reference sums one, 16 random bytes otherwise (`raw`; the
        IPv4 ones once with a valid header sum and once with the TTL changed: a missing handler shows as
        ErrPacketDrop only behind a header sum that passes).
      et/<hex>/raw/..: EDGE_ETHERTYPES in front of 46 zero bytes.
    variant: valid; l4flip (last transport byte), ttl (IPv4 header sum), cut1 (last byte missing).
    mac: `-` in the mac class; else `us`, followed by the same frame as `tw<k>` with byte k of the destination
      MAC changed (low bit and complement in turn), so every frame for the stack's MAC has a twin that is not."""
    rng = np.random.default_rng(seed)
    out = []
    twins = [0]

    def payload(lo=18, hi=150):
        return rng.integers(0, 256, int(rng.integers(lo, hi)), dtype=np.uint8).tobytes()

    def packet(l4, dst4=IP4_DST, dst6=IP6_DST, opts=b""):
        if l4 == "tcp4":
            return ether(0x0800, ipv4(6, tcp(payload()), opts=opts, dst=dst4))
        if l4 == "udp4":
            return ether(0x0800, ipv4(17, udp(payload()), opts=opts, dst=dst4))
        if l4 == "tcp6":
            return ether(0x86DD, ipv6(6, tcp(payload()), dst=dst6))
        if l4 == "udp6":
            return ether(0x86DD, ipv6(17, udp(payload()), dst=dst6))
        return ether(0x0806, payload(28, 29) + bytes(18))  # ARP: 28 bytes and the padding to 60

    def broken(f, variant):
        b = bytearray(f)
        if variant == "l4flip":
            b[-1] ^= 1 << int(rng.integers(0, 8))
        elif variant == "ttl":
            b[22] ^= 0x01
        elif variant == "cut1":
            del b[-1]
        return bytes(b)

    def put(label, f, twin=True):
        if not twin:
            out.append((label + "/-", f))
            return
        out.append((label + "/us", f))
        k, t = twins[0] % 6, twins[0]
        twins[0] += 1
        out.append((f"{label}/tw{k}", with_byte(f, k, f[k] ^ (0x01 if (t // 6) % 2 == 0 else 0xFF))))

    def with_variants(tag, f, v4, i, twin=True):
        """the valid frame and its broken forms: all of them for a destination the stack accepts
        (us, bcast), one in rotation for every fifth of the others."""
        put(f"{tag}/valid", f, twin)
        forms = ("l4flip", "ttl", "cut1") if v4 else ("l4flip", "cut1")
        if tag.split("/")[1] not in ("us", "bcast"):
            forms = (forms[(i // 5) % len(forms)],) if i % 5 == 0 else ()
        for v in forms:
            put(f"{tag}/{v}", broken(f, v), twin)

    i = 0
    for case, m in edge_macs():
        for l4 in EDGE_MAC_L4:
            f = m + packet(l4)[6:]
            if l4 == "arp":
                put(f"mac/{case}/{l4}/valid", f, False)
            else:
                with_variants(f"mac/{case}/{l4}", f, l4.endswith("4"), i, False)
            i += 1
    for case, a in edge_ip4s():
        for l4 in ("tcp", "udp"):
            for ihl in (5, 7):
                f = packet(l4 + "4", dst4=a, opts=opt_fill("rand", 4 * (ihl - 5), rng))
                with_variants(f"ip4/{case}/{l4}.ihl{ihl}", f, True, i)
                i += 1
    for case, a in edge_ip6s():
        for l4 in ("tcp", "udp"):
            with_variants(f"ip6/{case}/{l4}", packet(l4 + "6", dst6=a), False, i)
            i += 1
    for p in range(256):
        kind = {6: "tcp", 17: "udp", 1: "echo"}.get(p, "raw")
        l4 = tcp(payload()) if p == 6 else udp(payload()) if p == 17 else icmp(8, payload()) if p == 1 \
            else rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        f = ether(0x0800, ipv4(p, l4))
        f += bytes(max(0, 60 - len(f)))
        put(f"proto4/p{p}/{kind}/valid", f)
        put(f"proto4/p{p}/{kind}/" + ("ttl" if kind == "raw" else "l4flip"), broken(f, "ttl" if kind == "raw" else "l4flip"))
    for p in range(256):
        kind = {6: "tcp", 17: "udp", 58: "echo"}.get(p, "raw")
        l4 = tcp(payload()) if p == 6 else udp(payload()) if p == 17 else icmp(128, payload()) if p == 58 \
            else rng.integers(0, 256, 16, dtype=np.uint8).tobytes()
        f = ether(0x86DD, ipv6(p, l4))
        put(f"proto6/p{p}/{kind}/valid", f)
        if kind != "raw":
            put(f"proto6/p{p}/{kind}/l4flip", broken(f, "l4flip"))
        elif p % 8 == 3:
            put(f"proto6/p{p}/{kind}/cut1", broken(f, "cut1"))
    for et in EDGE_ETHERTYPES:
        put(f"et/{et:04x}/raw/valid", ether(et, bytes(46)))
    return out
