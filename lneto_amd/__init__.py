"""lneto_amd — MI355X-native batched checksum path of lneto.

Python binding (ctypes) of the C-ABI in include/lneto_amd.h, implemented by
lneto_amd/liblneto_amd.so (hand-written HIP kernels for gfx950 + host C++).
PyTorch is used only as device-memory / stream plumbing for the batch calls.

Mirrors the reference's API for this path:
    ethernet.CRC32 / CRC32Search / crc32.Update   -> crc32, crc32_search, crc32_update
    lneto.CRC791 / NeverZeroSum                   -> CRC791, never_zero_sum
    batch (device-resident) extensions            -> crc32_batch, fcs_verify_batch, sum16_batch

There is no CPU fallback for the batch calls: if the library is missing this
module raises at import; if no HIP device is usable the batch calls raise
LnetoError.
"""
from __future__ import annotations

import ctypes
import os

__all__ = [
    "LnetoError", "lib", "crc32", "crc32_update", "crc32_search", "sum_write_even", "sum16",
    "payload_sum16", "never_zero_sum", "CRC791", "crc32_batch", "fcs_verify_batch", "sum16_batch",
    "crc32_combine", "crc32_combine_batch", "crc32_update_batch", "crc32_chain_batch", "fcs_verify_chain_batch",
    "sum_partial", "sum16_chain", "sum_partial_batch", "sum16_chain_batch",
    "crc32_batch_host", "crc32_batch_multi", "tx_checksum_batch", "rx_verify_batch", "device_count", "version", "build_id", "LIB_PATH",
    "CRC32_RESIDUE", "RxRing", "RxFilter", "RX_NO_FCS", "research_lib",
    "RxPorts", "DELIVERY_DTYPE", "rx_deliver", "rx_deliver_batch", "rx_deliver_ws_bytes", "rx_verify_deliver_batch",
    "H_ETH", "H_IP4", "H_IP6", "H_TCP", "H_UDP", "H_COUNT", "H_NONE", "DLV_RST", "DLV_IP6", "DLV_FCS",
    "RstCfg", "TcpRst", "TX_FCS", "TCP_RST", "TCP_ACK", "ip4_id_chain", "rx_rst_entry", "tcp_rst_frame",
    "rx_rst_ws_bytes", "rx_rst_reply_batch", "tcp_rst_frames_batch",
    "IcmpEcho", "rx_echo_entry", "icmp_echo_reply_frame", "rx_echo_ws_bytes", "rx_echo_reply_batch",
    "ArpEntry", "ARP_SEEN_DTYPE", "ARP_REQUEST", "ARP_REPLY", "rx_arp_entry", "arp_frame", "rx_arp_ws_bytes",
    "rx_arp_batch", "arp_frames_batch",
]

HERE = os.path.dirname(os.path.abspath(__file__))
# LNETO_AMD_LIB selects an alternative in-tree build (profiling experiments only).
LIB_PATH = os.environ.get("LNETO_AMD_LIB") or os.path.join(HERE, "liblneto_amd.so")
CRC32_RESIDUE = 0x2144DF1C

LNX_OK, LNX_EINVAL, LNX_ENODEV, LNX_EHIP, LNX_ENOMEM = 0, -1, -2, -3, -5
_ERRNAMES = {LNX_EINVAL: "EINVAL", LNX_ENODEV: "ENODEV", LNX_EHIP: "EHIP", LNX_ENOMEM: "ENOMEM"}


class LnetoError(RuntimeError):
    pass


if not os.path.exists(LIB_PATH):
    raise ImportError(f"{LIB_PATH} is not built; run `python -c 'import __graft_entry__ as g; g.build()'` "
                      "or `make -C lneto_amd/csrc`")

# PyTorch-ROCm bundles its own libamdhip64.so.7 / libhsa-runtime64.so.1.  If this
# library were loaded first it would pull /opt/rocm's copies in, and torch would
# then load its bundled ones as well: two HSA runtimes in one process, and HIP
# calls from one of them see no device.  Importing torch first makes the dynamic
# linker resolve our libamdhip64.so.7 dependency to torch's already-loaded one,
# so the process has exactly one HIP runtime.  (C / C++ / cgo users get /opt/rocm's.)
try:
    import torch as _torch  # noqa: F401
except ImportError:  # pragma: no cover - torch is plumbing, not a dependency of the C-ABI
    _torch = None

lib = ctypes.CDLL(LIB_PATH)

_u8p = ctypes.POINTER(ctypes.c_uint8)
_vp = ctypes.c_void_p


class RxFilter(ctypes.Structure):
    """lnx_rx_filter (include/lneto_amd.h): the stack configuration behind the
    receive verdicts' ErrPacketDrop checks (internet/stack-ethernet.go:146-161,
    internet/stack-ip4.go:108-141, internet/stack-ip6.go:93-111).  Build it with
    RxFilter.make(mac=..., ip4=..., ...)."""
    _fields_ = [
        ("mac", ctypes.c_uint8 * 6), ("eth_accept_multicast", ctypes.c_uint8),
        ("ip4_accept_multicast", ctypes.c_uint8), ("ip4_accept_broadcast", ctypes.c_uint8),
        ("ip6_accept_multicast", ctypes.c_uint8), ("ip4", ctypes.c_uint8 * 4), ("ip6", ctypes.c_uint8 * 16),
        ("ethertypes", ctypes.c_uint16 * 8), ("n_ethertypes", ctypes.c_uint32),
        ("ip4_protocols", ctypes.c_uint8 * 32), ("ip6_protocols", ctypes.c_uint8 * 32),
    ]

    @classmethod
    def make(cls, mac: bytes, ethertypes=(0x0800, 0x86DD, 0x0806), ip4: bytes = bytes(4), ip6: bytes = bytes(16),
             ip4_protocols=(1, 6, 17), ip6_protocols=(6, 17, 58), eth_accept_multicast: bool = False,
             ip4_accept_multicast: bool = False, ip4_accept_broadcast: bool = False,
             ip6_accept_multicast: bool = False) -> "RxFilter":
        if len(mac) != 6 or len(ip4) != 4 or len(ip6) != 16 or len(ethertypes) > 8:
            raise LnetoError("RxFilter: mac 6 bytes, ip4 4, ip6 16, at most 8 EtherTypes")
        if any(et <= 1500 or et > 0xFFFF for et in ethertypes):
            # RegisterEthernet: proto > MaxUint16 || proto <= 1500 -> ErrInvalidConfig (internet/stack-ethernet.go:131-135)
            raise LnetoError("RxFilter: EtherTypes must be in (1500, 0xFFFF] (RegisterEthernet)")
        f = cls()
        f.mac[:] = list(mac)
        f.ip4[:] = list(ip4)
        f.ip6[:] = list(ip6)
        f.eth_accept_multicast, f.ip4_accept_multicast = int(eth_accept_multicast), int(ip4_accept_multicast)
        f.ip4_accept_broadcast, f.ip6_accept_multicast = int(ip4_accept_broadcast), int(ip6_accept_multicast)
        f.n_ethertypes = len(ethertypes)
        for i, et in enumerate(ethertypes):
            f.ethertypes[i] = et
        for arr, protos in ((f.ip4_protocols, ip4_protocols), (f.ip6_protocols, ip6_protocols)):
            for p in protos:
                arr[p >> 3] |= 1 << (p & 7)
        return f


class RxPorts(ctypes.Structure):
    """lnx_rx_ports (include/lneto_amd.h): the local ports of the nodes registered
    on StackPorts, per protocol and in registration order (Register,
    internet/stack-ports.go:88-97; nodeByPort takes the first match,
    internet/definitions.go:108-116).  Build it with RxPorts.make(tcp=..., udp=...)."""
    _fields_ = [("tcp", ctypes.c_uint16 * 256), ("n_tcp", ctypes.c_uint32),
                ("udp", ctypes.c_uint16 * 256), ("n_udp", ctypes.c_uint32)]

    @classmethod
    def make(cls, tcp=(), udp=()) -> "RxPorts":
        tcp, udp = list(tcp), list(udp)
        if len(tcp) > 256 or len(udp) > 256 or any(not 0 <= p <= 0xFFFF for p in tcp + udp):
            raise LnetoError("RxPorts: at most 256 ports per protocol, each in [0, 0xFFFF]")
        r = cls()
        r.n_tcp, r.n_udp = len(tcp), len(udp)
        for i, p in enumerate(tcp):
            r.tcp[i] = p
        for i, p in enumerate(udp):
            r.udp[i] = p
        return r


class RstCfg(ctypes.Structure):
    """lnx_rst_cfg (include/lneto_amd.h): the stack's side of a RST reply —
    StackEthernet's MAC and gateway MAC (internet/stack-ethernet.go:184,197),
    stackip4's address (internet/stack-ip4.go:194) and whether the link layer
    appends the CRC (:211-215).  Build it with RstCfg.make(mac=, gw_mac=, ip4=, fcs=)."""
    _fields_ = [("mac", ctypes.c_uint8 * 6), ("gw_mac", ctypes.c_uint8 * 6), ("ip4", ctypes.c_uint8 * 4),
                ("flags", ctypes.c_uint32)]

    @classmethod
    def make(cls, mac: bytes, gw_mac: bytes, ip4: bytes, fcs: bool = True) -> "RstCfg":
        if len(mac) != 6 or len(gw_mac) != 6 or len(ip4) != 4:
            raise LnetoError("RstCfg: mac 6 bytes, gw_mac 6, ip4 4")
        c = cls()
        c.mac[:] = list(mac)
        c.gw_mac[:] = list(gw_mac)
        c.ip4[:] = list(ip4)
        c.flags = 2 if fcs else 0  # LNX_TX_FCS
        return c


class TcpRst(ctypes.Structure):
    """lnx_tcp_rst (include/lneto_amd.h): rstEntry, tcp/rst.go:12-19."""
    _fields_ = [("remote_addr", ctypes.c_uint8 * 4), ("remote_port", ctypes.c_uint16), ("local_port", ctypes.c_uint16),
                ("seq", ctypes.c_uint32), ("ack", ctypes.c_uint32), ("flags", ctypes.c_uint16), ("zero", ctypes.c_uint16)]

    @classmethod
    def make(cls, remote_addr: bytes, remote_port: int, local_port: int, seq: int, ack: int, flags: int) -> "TcpRst":
        if len(remote_addr) != 4:
            raise LnetoError("TcpRst: remote_addr 4 bytes (RSTQueue.Queue keeps nothing else, tcp/rst.go:23)")
        e = cls()
        e.remote_addr[:] = list(remote_addr)
        e.remote_port, e.local_port = remote_port & 0xFFFF, local_port & 0xFFFF
        e.seq, e.ack, e.flags = seq & 0xFFFFFFFF, ack & 0xFFFFFFFF, flags & 0xFFFF
        return e


class IcmpEcho(ctypes.Structure):
    """lnx_icmp_echo (include/lneto_amd.h): what icmpv4.Client.Demux keeps of an echo
    request (ipv4/icmpv4/client.go:128-132), the data as a range of the frame."""
    _fields_ = [("remote_addr", ctypes.c_uint8 * 4), ("id", ctypes.c_uint16), ("seq", ctypes.c_uint16),
                ("data_off", ctypes.c_uint32), ("data_len", ctypes.c_uint32)]

    @classmethod
    def make(cls, remote_addr: bytes, id: int, seq: int, data_off: int, data_len: int) -> "IcmpEcho":
        if len(remote_addr) != 4:
            raise LnetoError("IcmpEcho: remote_addr 4 bytes")
        e = cls()
        e.remote_addr[:] = list(remote_addr)
        e.id, e.seq = id & 0xFFFF, seq & 0xFFFF
        e.data_off, e.data_len = data_off, data_len
        return e


class ArpEntry(ctypes.Structure):
    """lnx_arp_entry (include/lneto_amd.h): a hardware address and the protocol
    address it belongs to — the sender of an ARP frame, or what the cache's
    entry.put writes into the target fields (arp/cache.go:65-67)."""
    _fields_ = [("hw", ctypes.c_uint8 * 6), ("zero", ctypes.c_uint16), ("ip", ctypes.c_uint8 * 4)]

    @classmethod
    def make(cls, hw: bytes, ip: bytes) -> "ArpEntry":
        if len(hw) != 6 or len(ip) != 4:
            raise LnetoError("ArpEntry: hw 6 bytes, ip 4")
        e = cls()
        e.hw[:] = list(hw)
        e.ip[:] = list(ip)
        return e


_sig = {
    "lnx_rx_arp_entry": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp, _vp, _vp]),
    "lnx_arp_frame": (ctypes.c_int, [_vp, ctypes.c_uint16, _vp, _vp, _vp]),
    "lnx_rx_arp_ws_bytes": (ctypes.c_uint64, [ctypes.c_uint64]),
    "lnx_rx_arp_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, ctypes.c_uint64,
                                        ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lnx_arp_frames_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_rx_echo_entry": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp]),
    "lnx_icmp_echo_reply_frame": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint16, _vp, ctypes.c_uint32, _vp]),
    "lnx_rx_echo_ws_bytes": (ctypes.c_uint64, [ctypes.c_uint64]),
    "lnx_rx_echo_reply_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint64,
                                               ctypes.c_uint64, _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lnx_ip4_id_chain": (None, [ctypes.c_uint8, ctypes.c_uint16, ctypes.c_uint64, _vp]),
    "lnx_rx_rst_entry": (ctypes.c_int, [_vp, ctypes.c_size_t, _vp, _vp]),
    "lnx_tcp_rst_frame": (ctypes.c_int, [_vp, _vp, ctypes.c_uint16, _vp, _vp]),
    "lnx_rx_rst_ws_bytes": (ctypes.c_uint64, [ctypes.c_uint64]),
    "lnx_rx_rst_reply_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp, _vp, ctypes.c_uint64,
                                              _vp, _vp, _vp, _vp, _vp]),
    "lnx_tcp_rst_frames_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "lnx_crc32_update": (ctypes.c_uint32, [ctypes.c_uint32, _u8p, ctypes.c_size_t]),
    "lnx_crc32": (ctypes.c_uint32, [_u8p, ctypes.c_size_t]),
    "lnx_crc32_combine": (ctypes.c_uint32, [ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint64]),
    "lnx_crc32_combine_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_crc32_update_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "lnx_crc32_chain_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp]),
    "lnx_fcs_verify_chain_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp]),
    "lnx_crc32_search": (ctypes.c_int64, [_u8p, ctypes.c_size_t, ctypes.c_int64]),
    "lnx_sum_write_even": (ctypes.c_uint32, [ctypes.c_uint32, _u8p, ctypes.c_size_t]),
    "lnx_sum16": (ctypes.c_uint16, [ctypes.c_uint32]),
    "lnx_sum16_payload": (ctypes.c_uint16, [ctypes.c_uint32, _u8p, ctypes.c_size_t]),
    "lnx_never_zero_sum": (ctypes.c_uint16, [ctypes.c_uint16]),
    "lnx_sum_partial": (ctypes.c_uint32, [ctypes.c_uint32, _u8p, ctypes.c_size_t, ctypes.c_int]),
    "lnx_sum16_chain": (ctypes.c_uint16, [ctypes.c_uint32, _vp, _vp, ctypes.c_size_t]),
    "lnx_sum_partial_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_sum16_chain_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, _vp, _vp, _vp,
                                             _vp]),
    "lnx_crc32_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_fcs_verify_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_sum16_batch": (ctypes.c_int, [_vp, _vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_ingress_verify_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "lnx_ingress_verify_batch_filtered": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                                         ctypes.POINTER(RxFilter), _vp, _vp]),
    "lnx_rx_ring_set_filter": (ctypes.c_int, [_vp, ctypes.POINTER(RxFilter)]),
    "lnx_crc32_search_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_crc32_segments": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_fcs_append_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, _vp, _vp]),
    "lnx_tx_checksum_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_crc32_batch_host": (ctypes.c_int, [_vp, ctypes.c_uint64, _vp, ctypes.c_uint64, _vp, ctypes.c_int]),
    "lnx_crc32_batch_multi": (ctypes.c_int, [ctypes.c_int, _vp, _vp, _vp, _vp, _vp]),
    "lnx_rx_ring_create": (ctypes.c_int, [ctypes.c_int, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, ctypes.POINTER(_vp)]),
    "lnx_rx_ring_destroy": (None, [_vp]),
    "lnx_rx_ring_slots": (_vp, [_vp]),
    "lnx_rx_ring_lengths": (_vp, [_vp]),
    "lnx_rx_ring_ingress": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                           _vp, _vp]),
    "lnx_ingress_packets": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                           _vp, _vp]),
    "lnx_crc32_batch_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp]),
    "lnx_fcs_verify_batch_ex": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, ctypes.c_uint32, _vp]),
    "lnx_egress_packets": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                          ctypes.c_uint32, _vp]),
    "lnx_rx_verify_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(RxFilter),
                                            _vp, _vp, _vp]),
    "lnx_rx_deliver": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.POINTER(RxFilter), ctypes.POINTER(RxPorts),
                                      ctypes.c_int, ctypes.c_uint8, _vp]),
    "lnx_rx_deliver_ws_bytes": (ctypes.c_uint64, [ctypes.c_uint64]),
    "lnx_rx_deliver_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(RxFilter),
                                            ctypes.POINTER(RxPorts), _vp, _vp, _vp, _vp, _vp, _vp, _vp]),
    "lnx_rx_verify_deliver_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32,
                                                   ctypes.POINTER(RxFilter), ctypes.POINTER(RxPorts), _vp, _vp, _vp,
                                                   _vp, _vp, _vp, _vp]),
    "lnx_rx_ring_set_ports": (ctypes.c_int, [_vp, ctypes.POINTER(RxPorts)]),
    "lnx_rx_ring_ingress_deliver": (ctypes.c_int, [_vp, ctypes.c_uint32, ctypes.c_uint32, ctypes.c_uint32,
                                                   ctypes.c_uint32, _vp, _vp, _vp, _vp, _vp]),
    "lnx_ingress_packets_deliver": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32,
                                                   _vp, _vp, _vp, _vp, _vp]),
    "lnx_ingress_verdict": (ctypes.c_int, [_vp, ctypes.c_size_t, ctypes.c_uint32, ctypes.POINTER(RxFilter)]),
    "lnx_pcap_checksums": (ctypes.c_int, [_vp, ctypes.c_size_t]),
    "lnx_pcap_verify_batch": (ctypes.c_int, [_vp, _vp, ctypes.c_uint64, _vp, _vp]),
    "lnx_tx_checksum": (ctypes.c_int, [_vp, ctypes.c_size_t]),
    "lnx_fcs_append": (ctypes.c_int, [_vp, ctypes.POINTER(ctypes.c_uint32), ctypes.c_uint32]),
    "lnx_rx_ring_set_host_threshold": (ctypes.c_int, [_vp, ctypes.c_uint32]),
    "lnx_rx_ring_stats": (ctypes.c_int, [_vp, _vp]),
    "lnx_rx_ring_set_zero_copy": (ctypes.c_int, [_vp, ctypes.c_int]),
    "lnx_tx_finish_batch": (ctypes.c_int, [_vp, _vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.c_uint32, _vp, _vp]),
    "lnx_device_count": (ctypes.c_int, []),
    "lnx_last_error": (ctypes.c_char_p, []),
    "lnx_version": (ctypes.c_char_p, []),
}
for _name, (_res, _args) in _sig.items():
    _f = getattr(lib, _name)
    _f.restype = _res
    _f.argtypes = _args


def _check(rc: int, what: str) -> None:
    if rc != LNX_OK:
        detail = lib.lnx_last_error().decode() if rc == LNX_EHIP else ""
        raise LnetoError(f"{what} failed: {_ERRNAMES.get(rc, rc)} {detail}".strip())


def _buf(data: bytes):
    data = bytes(data)
    return (ctypes.c_uint8 * max(len(data), 1)).from_buffer_copy(data or b"\0"), len(data)


# ----------------------------------------------------------- per-frame (host)
def crc32_update(crc: int, p: bytes) -> int:
    """Go crc32.Update(crc, IEEETable, p) — the CRC32Update hook (internet/stack-ethernet.go:31-32)."""
    b, n = _buf(p)
    return lib.lnx_crc32_update(crc & 0xFFFFFFFF, b, n)


def crc32(p: bytes) -> int:
    """ethernet.CRC32 (ethernet/crc.go:19-21)."""
    b, n = _buf(p)
    return lib.lnx_crc32(b, n)


def crc32_combine(crc_a: int, crc_b: int, len_b: int) -> int:
    """CRC32(A || B) from CRC32(A), CRC32(B) and len(B) (lnx_crc32_combine; zlib's crc32_combine).
    crc32_combine(seed, crc32(B), len(B)) == crc32_update(seed, B)."""
    if not 0 <= len_b < 2**64:
        raise LnetoError("crc32_combine: len_b must be in [0, 2**64)")
    return lib.lnx_crc32_combine(crc_a & 0xFFFFFFFF, crc_b & 0xFFFFFFFF, len_b)


def crc32_search(p: bytes, min_off: int) -> int:
    """ethernet.CRC32Search (ethernet/crc.go:28-47); -1 for every int64 min_off above len(p) - 4."""
    b, n = _buf(p)
    return lib.lnx_crc32_search(b, n, min_off)


def sum_write_even(s: int, p: bytes) -> int:
    if len(p) & 1:
        raise IndexError("WriteEven requires an even-length buffer (crc.go:30)")
    b, n = _buf(p)
    return lib.lnx_sum_write_even(s & 0xFFFFFFFF, b, n)


def sum16(s: int) -> int:
    return lib.lnx_sum16(s & 0xFFFFFFFF)


def payload_sum16(s: int, p: bytes) -> int:
    b, n = _buf(p)
    return lib.lnx_sum16_payload(s & 0xFFFFFFFF, b, n)


def never_zero_sum(x: int) -> int:
    return lib.lnx_never_zero_sum(x & 0xFFFF)


def sum_partial(s: int, p: bytes, phase: int = 0) -> int:
    """The raw 32-bit running sum of CRC791 over a piece of a packet (lnx_sum_partial):
    any length; phase = the parity of the piece's offset in its packet.
    sum16(sum_partial(s, p)) == payload_sum16(s, p)."""
    b, n = _buf(p)
    return lib.lnx_sum_partial(s & 0xFFFFFFFF, b, n, phase & 1)


def sum16_chain(seed: int, segs) -> int:
    """CRC791{seed}.PayloadSum16 over the concatenation of the buffers in ``segs`` (lnx_sum16_chain)."""
    segs = [bytes(g) for g in segs]
    m = len(segs)
    bufs = [_buf(g)[0] for g in segs]  # kept alive until the call returns
    ptrs = (ctypes.c_void_p * max(m, 1))(*[ctypes.addressof(b) for b in bufs])
    lens = (ctypes.c_size_t * max(m, 1))(*[len(g) for g in segs])
    return lib.lnx_sum16_chain(seed & 0xFFFFFFFF, ctypes.addressof(ptrs), ctypes.addressof(lens), m)


class CRC791:
    """lneto.CRC791 (crc.go:13-62): running RFC 791 one's-complement sum."""

    __slots__ = ("sum",)

    def __init__(self) -> None:
        self.sum = 0

    def WriteEven(self, buff: bytes) -> None:
        self.sum = sum_write_even(self.sum, buff)

    def AddUint16(self, v: int) -> None:
        self.sum = (self.sum + (v & 0xFFFF)) & 0xFFFFFFFF

    def AddUint32(self, v: int) -> None:
        self.AddUint16((v >> 16) & 0xFFFF)
        self.AddUint16(v & 0xFFFF)

    def Sum16(self) -> int:
        return sum16(self.sum)

    def PayloadSum16(self, buff: bytes) -> int:
        return payload_sum16(self.sum, buff)

    def Reset(self) -> None:
        self.sum = 0


# ------------------------------------------------------- batched (device)
def _dtypes(*names):
    import torch
    table = {
        "u8": (torch.uint8, torch.int8),
        "i16": (torch.int16, getattr(torch, "uint16", torch.int16)),
        "i32": (torch.int32, getattr(torch, "uint32", torch.int32)),
        "i64": (torch.int64, getattr(torch, "uint64", torch.int64)),
    }
    return [table[n] for n in names]


class _Batch:
    """Argument check and device scope of one batch call.

    Every tensor must be a contiguous device tensor of the 8-, 16-, 32- or 64-bit
    width the C-ABI reads through it (signedness is free: the kernels see the
    bits), and all of them must live on ONE device.  The call then runs with that
    device current and on its stream (the caller's ``stream`` must be on the same
    device), so the library's per-device context and the kernel's memory agree.
    """

    def __init__(self, what, args, stream):
        import torch
        self.what = what
        dev = None
        # a kind ending in "?" marks an optional argument (NULL in the C-ABI)
        for name, t, kind in args:
            if t is None and not kind.endswith("?"):
                raise LnetoError(f"{what}: {name} is required")
        for name, t, kind in args:
            kind = kind.rstrip("?")
            if t is None:
                continue
            if not isinstance(t, torch.Tensor) or not t.is_cuda or not t.is_contiguous():
                raise LnetoError(f"{what}: {name} must be a contiguous device tensor")
            if t.dtype not in _dtypes(kind)[0]:
                raise LnetoError(f"{what}: {name} must be {kind} (got {t.dtype})")
            if dev is None:
                dev = t.device
            elif t.device != dev:
                raise LnetoError(f"{what}: {name} is on {t.device}, other arguments on {dev}")
        self.device = dev
        if stream is not None and stream.device != dev:
            raise LnetoError(f"{what}: stream is on {stream.device}, tensors on {dev}")
        self._stream = stream
        self._ctx = torch.cuda.device(dev)

    def __enter__(self):
        import torch
        self._ctx.__enter__()
        s = self._stream if self._stream is not None else torch.cuda.current_stream(self.device)
        return s.cuda_stream

    def __exit__(self, *exc):
        return self._ctx.__exit__(*exc)


def _out(what, out, n, dtype, kind, device):
    """Caller-supplied output: checked like an input and at least n elements; else allocated."""
    import torch
    if out is None:
        return torch.empty(max(n, 0), dtype=dtype, device=device)
    if not isinstance(out, torch.Tensor) or not out.is_cuda or not out.is_contiguous():
        raise LnetoError(f"{what}: out must be a contiguous device tensor")
    if out.dtype not in _dtypes(kind)[0]:
        raise LnetoError(f"{what}: out must be {kind} (got {out.dtype})")
    if out.device != device:
        raise LnetoError(f"{what}: out is on {out.device}, inputs on {device}")
    if out.numel() < n:
        raise LnetoError(f"{what}: out holds {out.numel()} elements, {n} needed")
    return out


def _need_len(what, name, t, n):
    if t is not None and t.numel() < n:
        raise LnetoError(f"{what}: {name} holds {t.numel()} elements, {n} needed")


BATCH_SHORT_FRAMES = 1  # LNX_BATCH_SHORT_FRAMES


def crc32_batch(d_bytes, d_off, out=None, stream=None, short_frames=False):
    """CRC32 of every frame d_bytes[d_off[i]:d_off[i+1]] on the GPU.

    d_bytes: uint8 device tensor; d_off: int64 device tensor of N+1 offsets.
    Returns an int32 device tensor holding the uint32 CRCs bit-for-bit.
    short_frames=True (lnx_crc32_batch_ex with LNX_BATCH_SHORT_FRAMES): the
    staged lane-stream kernel reads every slice that is not giant, where the
    plain entry picks the kernel per slice on the device (same results).
    """
    import torch
    what = "lnx_crc32_batch_ex" if short_frames else "lnx_crc32_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    out = _out(what, out, n, torch.int32, "i32", b.device)
    if n > 0:
        with b as s:
            if short_frames:
                _check(lib.lnx_crc32_batch_ex(d_bytes.data_ptr(), d_off.data_ptr(), n, out.data_ptr(),
                                              BATCH_SHORT_FRAMES, s), what)
            else:
                _check(lib.lnx_crc32_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, out.data_ptr(), s), what)
    return out


def fcs_verify_batch(d_bytes, d_off, out=None, stream=None, short_frames=False):
    """1 where frame i (payload + trailing LE FCS) passes the FCS check, else 0
    (short_frames as crc32_batch)."""
    import torch
    what = "lnx_fcs_verify_batch_ex" if short_frames else "lnx_fcs_verify_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    out = _out(what, out, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            if short_frames:
                _check(lib.lnx_fcs_verify_batch_ex(d_bytes.data_ptr(), d_off.data_ptr(), n, out.data_ptr(),
                                                   BATCH_SHORT_FRAMES, s), what)
            else:
                _check(lib.lnx_fcs_verify_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, out.data_ptr(), s), what)
    return out


def crc32_segments(d_bytes, d_start, d_len, out=None, stream=None):
    """CRC32 of every frame d_bytes[d_start[i] : d_start[i] + d_len[i]] (lnx_crc32_segments);
    d_start int64, d_len int32; frames in address order, not overlapping."""
    import torch
    what = "lnx_crc32_segments"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_start", d_start, "i64"), ("d_len", d_len, "i32")], stream)
    n = d_start.numel()
    _need_len(what, "d_len", d_len, n)
    out = _out(what, out, n, torch.int32, "i32", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_crc32_segments(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n,
                                          out.data_ptr(), s), what)
    return out


def _ptr(t):
    return t.data_ptr() if t is not None else None


def crc32_combine_batch(d_crc_a, d_crc_b, d_len_b, out=None, stream=None):
    """out[i] = crc32_combine(d_crc_a[i], d_crc_b[i], d_len_b[i]) on the GPU
    (lnx_crc32_combine_batch).  d_crc_a, d_crc_b: int32 (N, uint32 bits); d_len_b:
    int64 (N).  ``out`` may be d_crc_a or d_crc_b.  Returns int32 (N)."""
    import torch
    what = "lnx_crc32_combine_batch"
    b = _Batch(what, [("d_crc_a", d_crc_a, "i32"), ("d_crc_b", d_crc_b, "i32"), ("d_len_b", d_len_b, "i64")], stream)
    n = d_crc_a.numel()
    _need_len(what, "d_crc_b", d_crc_b, n)
    _need_len(what, "d_len_b", d_len_b, n)
    out = _out(what, out, n, torch.int32, "i32", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_crc32_combine_batch(d_crc_a.data_ptr(), d_crc_b.data_ptr(), d_len_b.data_ptr(), n,
                                               out.data_ptr(), s), what)
    return out


def crc32_update_batch(d_bytes, d_off, d_seed=None, out=None, stream=None):
    """The CRC32Update hook with its crc argument, batched (lnx_crc32_update_batch):
    out[i] = crc32_update(d_seed[i], d_bytes[d_off[i]:d_off[i+1]]).  d_seed: int32
    (N) or None (all zero: crc32_batch).  ``out`` must not overlap d_seed; a
    running CRC over several calls ping-pongs two arrays.  Returns int32 (N)."""
    import torch
    what = "lnx_crc32_update_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_seed", d_seed, "i32?")], stream)
    n = d_off.numel() - 1
    _need_len(what, "d_seed", d_seed, n)
    out = _out(what, out, n, torch.int32, "i32", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_crc32_update_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, _ptr(d_seed), out.data_ptr(), s),
                   what)
    return out


def _chain_args(what, d_bytes, d_start, d_len, d_first, d_seed, seg_crc, nseg, stream, ws_per_seg=1):
    import torch
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_start", d_start, "i64"), ("d_len", d_len, "i32"),
                      ("d_first", d_first, "i64"), ("d_seed", d_seed, "i32?")], stream)
    nframes = d_first.numel() - 1
    if nseg is None:
        nseg = d_start.numel()
    _need_len(what, "d_start", d_start, nseg)
    _need_len(what, "d_len", d_len, nseg)
    _need_len(what, "d_seed", d_seed, nframes)
    # the library allocates nothing: the workspace is made here when the caller passes none
    seg_crc = _out(what, seg_crc, ws_per_seg * nseg, torch.int32, "i32", b.device)
    return b, nseg, nframes, seg_crc


def crc32_chain_batch(d_bytes, d_start, d_len, d_first, d_seed=None, out=None, seg_crc=None, nseg=None, stream=None):
    """CRC32 of frames made of segments (lnx_crc32_chain_batch): frame f is the
    concatenation of segments d_first[f] .. d_first[f+1]-1, segment k is
    d_bytes[d_start[k] : d_start[k] + d_len[k]] (int64 starts, int32 lengths,
    int64 d_first of nframes+1 entries); out[f] = crc32_update(d_seed[f] or 0,
    frame f).  ``seg_crc`` (int32, nseg) is the workspace, allocated when None
    and left holding each segment's own CRC; ``nseg`` (default: all of d_start)
    counts the segments in use.  Returns int32 (nframes)."""
    import torch
    what = "lnx_crc32_chain_batch"
    b, nseg, nframes, seg_crc = _chain_args(what, d_bytes, d_start, d_len, d_first, d_seed, seg_crc, nseg, stream)
    out = _out(what, out, nframes, torch.int32, "i32", b.device)
    if nframes > 0:
        with b as s:
            _check(lib.lnx_crc32_chain_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), nseg,
                                             d_first.data_ptr(), nframes, _ptr(d_seed), seg_crc.data_ptr(),
                                             out.data_ptr(), s), what)
    return out


def fcs_verify_chain_batch(d_bytes, d_start, d_len, d_first, out=None, seg_crc=None, nseg=None, stream=None):
    """1 where frame f (segments as crc32_chain_batch, trailing LE FCS included,
    wherever its 4 bytes fall) passes the FCS check, else 0
    (lnx_fcs_verify_chain_batch).  Returns uint8 (nframes)."""
    import torch
    what = "lnx_fcs_verify_chain_batch"
    b, nseg, nframes, seg_crc = _chain_args(what, d_bytes, d_start, d_len, d_first, None, seg_crc, nseg, stream)
    out = _out(what, out, nframes, torch.uint8, "u8", b.device)
    if nframes > 0:
        with b as s:
            _check(lib.lnx_fcs_verify_chain_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), nseg,
                                                  d_first.data_ptr(), nframes, seg_crc.data_ptr(), out.data_ptr(), s),
                   what)
    return out


def fcs_append_batch(d_bytes, d_start, d_len, capacity: int, status=None, stream=None):
    """TX FCS append in place (lnx_fcs_append_batch): pad to 60, append LE FCS,
    d_len (int32, updated) += padding + 4.  Returns the uint8 status (0 or 6)."""
    import torch
    what = "lnx_fcs_append_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_start", d_start, "i64"), ("d_len", d_len, "i32")], stream)
    n = d_start.numel()
    _need_len(what, "d_len", d_len, n)
    status = _out(what, status, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_fcs_append_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n, capacity,
                                            status.data_ptr(), s), what)
    return status


def tx_checksum_batch(d_bytes, d_start, d_len, status=None, stream=None):
    """Transmit checksum generate in place (lnx_tx_checksum_batch): IPv4 / IPv6
    length fields, IPv4 header CRC, TCP / UDP / ICMP CRCs of every frame
    d_bytes[d_start[i] : d_start[i] + d_len[i]] (int64 starts, int32 lengths).
    Returns the uint8 status (0, 18 ErrTruncatedFrame, 15 ErrInvalidLengthField)."""
    import torch
    what = "lnx_tx_checksum_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_start", d_start, "i64"), ("d_len", d_len, "i32")], stream)
    n = d_start.numel()
    _need_len(what, "d_len", d_len, n)
    status = _out(what, status, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_tx_checksum_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n,
                                             status.data_ptr(), s), what)
    return status


def tx_finish_batch(d_bytes, d_start, d_len, capacity: int, flags: int = 3, status=None, stream=None):
    """The transmit tail in one read (lnx_tx_finish_batch): the checksum step
    (flags & TX_CHECKSUM) then padding + FCS (flags & TX_FCS) of every frame
    d_bytes[d_start[i] : d_start[i] + d_len[i]], in place; d_len (int32) is
    updated.  Returns the uint8 status (the checksum step's if non-zero, else
    the append's)."""
    import torch
    what = "lnx_tx_finish_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_start", d_start, "i64"), ("d_len", d_len, "i32")], stream)
    n = d_start.numel()
    _need_len(what, "d_len", d_len, n)
    status = _out(what, status, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_tx_finish_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), n, capacity,
                                           flags, status.data_ptr(), s), what)
    return status


def crc32_search_batch(d_bytes, d_off, d_min_off=None, out=None, stream=None):
    """ethernet.CRC32Search of every capture d_bytes[d_off[i]:d_off[i+1]] on the GPU
    (lnx_crc32_search_batch).  d_min_off: int64 (N) or None (all 0).  Returns int64 (N), -1 = none:
    also for every int64 d_min_off[i] above the capture's length - 4."""
    import torch
    what = "lnx_crc32_search_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_min_off", d_min_off, "i64?")],
               stream)
    n = d_off.numel() - 1
    _need_len(what, "d_min_off", d_min_off, n)
    out = _out(what, out, n, torch.int64, "i64", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_crc32_search_batch(d_bytes.data_ptr(), d_off.data_ptr(),
                                              d_min_off.data_ptr() if d_min_off is not None else None, n,
                                              out.data_ptr(), s), what)
    return out


VERIFY_EVIL_BIT = 1  # LNX_VERIFY_EVIL_BIT
VERIFY_ICMP = 2      # LNX_VERIFY_ICMP
RX_NO_FCS = 4        # LNX_RX_NO_FCS: the device strips the FCS (x/netdev/interface.go:34-40)
TX_CHECKSUM, TX_FCS = 1, 2  # LNX_TX_CHECKSUM, LNX_TX_FCS
HOST_BATCH_DEFAULT = 64  # LNX_HOST_BATCH_DEFAULT: packet batches below it run on the host


def ingress_verify_batch(d_bytes, d_off, flags: int = 0, out=None, stream=None, filter: RxFilter | None = None):
    """Receive-path checksum verdict per Ethernet frame (lnx_ingress_verify_batch,
    or lnx_ingress_verify_batch_filtered with a stack ``filter``): 0 = checks
    passed / none apply, else lneto's errGeneric code (3 = ErrBadCRC, 2 = ErrPacketDrop, ...)."""
    import torch
    what = "lnx_ingress_verify_batch" if filter is None else "lnx_ingress_verify_batch_filtered"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    out = _out(what, out, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            if filter is None:
                rc = lib.lnx_ingress_verify_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags, out.data_ptr(), s)
            else:
                rc = lib.lnx_ingress_verify_batch_filtered(d_bytes.data_ptr(), d_off.data_ptr(), n, flags,
                                                           ctypes.byref(filter), out.data_ptr(), s)
            _check(rc, what)
    return out


def rx_verify_batch(d_bytes, d_off, flags: int = 0, filter: RxFilter | None = None, out=None, stream=None):
    """lneto's whole receive check in one pass over each frame (lnx_rx_verify_batch):
    returns (fcs_ok, verdict) uint8 tensors — the FCS residue test of every frame
    d_bytes[d_off[i]:d_off[i+1]] (FCS included) and the verdict of the frame
    without its FCS.  flags: VERIFY_EVIL_BIT | VERIFY_ICMP | RX_NO_FCS."""
    import torch
    what = "lnx_rx_verify_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    ok, verdict = out if out is not None else (None, None)
    ok = _out(what, ok, n, torch.uint8, "u8", b.device)
    verdict = _out(what, verdict, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_rx_verify_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags,
                                           ctypes.byref(filter) if filter is not None else None, ok.data_ptr(),
                                           verdict.data_ptr(), s), what)
    return ok, verdict


# Receive delivery (lnx_rx_deliver*): handler ids LNX_H_*, record flags LNX_DLV_*
H_ETH, H_IP4, H_IP6, H_TCP, H_UDP, H_COUNT, H_NONE = 0, 16, 272, 528, 800, 1057, 0xFFFF
DLV_RST, DLV_IP6, DLV_FCS = 1, 2, 4
# lnx_rx_delivery as a numpy structured dtype (16 bytes): rec.cpu().numpy().view(DELIVERY_DTYPE).
# None without numpy, which only this constant needs (torch brings it along).
try:
    import numpy as _np
    DELIVERY_DTYPE = _np.dtype([("ip_end", "<u4"), ("handler", "<u2"), ("l4_off", "<u2"), ("src_port", "<u2"),
                                ("dst_port", "<u2"), ("verdict", "u1"), ("flags", "u1"), ("zero", "<u2")])
    assert DELIVERY_DTYPE.itemsize == 16
except ImportError:  # pragma: no cover
    DELIVERY_DTYPE = None


def rx_deliver(frame: bytes, verdict_in: int, filter: RxFilter | None = None, ports: RxPorts | None = None,
               fcs_ok: int | None = None) -> dict:
    """The delivery record of ONE frame (FCS stripped) on the host (lnx_rx_deliver):
    a dict of lnx_rx_delivery's fields.  verdict_in: the frame's receive verdict;
    fcs_ok: its FCS result, None for none."""
    buf = bytes(frame)
    out = (ctypes.c_uint8 * 16)()
    _check(lib.lnx_rx_deliver(buf, len(buf), ctypes.byref(filter) if filter is not None else None,
                              ctypes.byref(ports) if ports is not None else None,
                              -1 if fcs_ok is None else int(bool(fcs_ok)), verdict_in & 0xFF, ctypes.addressof(out)),
           "lnx_rx_deliver")
    raw = bytes(out)
    ip_end = int.from_bytes(raw[0:4], "little")
    handler, l4_off, src_port, dst_port = (int.from_bytes(raw[i:i + 2], "little") for i in (4, 6, 8, 10))
    return dict(ip_end=ip_end, handler=handler, l4_off=l4_off, src_port=src_port, dst_port=dst_port,
                verdict=raw[12], flags=raw[13], zero=int.from_bytes(raw[14:16], "little"))


def rx_deliver_ws_bytes(n: int) -> int:
    """Bytes of device workspace lnx_rx_deliver_batch needs to group n frames."""
    return lib.lnx_rx_deliver_ws_bytes(n)


def rx_deliver_batch(d_bytes, d_off, d_verdict, d_fcs_ok=None, flags: int = 0, filter: RxFilter | None = None,
                     ports: RxPorts | None = None, group: bool = True, stream=None):
    """Delivery records of a batch behind rx_verify_batch / ingress_verify_batch
    on the same d_off (lnx_rx_deliver_batch): returns (rec, order, count).
    rec is [n, 16] uint8, one lnx_rx_delivery a row (rec.cpu().numpy().view(DELIVERY_DTYPE));
    with ``group`` order (int32, n) lists the frames by ascending handler id,
    the frames not delivered last, in arrival order within every bucket, and
    count (int32, H_COUNT + 1) the buckets' sizes; else both are None and no
    workspace is allocated.  flags: RX_NO_FCS or 0 (frames carry their FCS)."""
    import torch
    what = "lnx_rx_deliver_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_verdict", d_verdict, "u8"),
                      ("d_fcs_ok", d_fcs_ok, "u8?")], stream)
    n = d_off.numel() - 1
    if n < 0:
        raise LnetoError(f"{what}: d_off holds no offset")
    _need_len(what, "d_verdict", d_verdict, n)
    _need_len(what, "d_fcs_ok", d_fcs_ok, n)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=b.device)
    order = count = ws = None
    if group:
        order = torch.empty(max(n, 1), dtype=torch.int32, device=b.device)  # (n = 0: still a pointer to pass)
        count = torch.empty(H_COUNT + 1, dtype=torch.int32, device=b.device)
        ws = torch.empty(rx_deliver_ws_bytes(n), dtype=torch.uint8, device=b.device)
    with b as s:
        _check(lib.lnx_rx_deliver_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags,
                                        ctypes.byref(filter) if filter is not None else None,
                                        ctypes.byref(ports) if ports is not None else None,
                                        d_fcs_ok.data_ptr() if d_fcs_ok is not None else None, d_verdict.data_ptr(),
                                        rec.data_ptr(), order.data_ptr() if group else None,
                                        count.data_ptr() if group else None, ws.data_ptr() if group else None, s),
               what)
        if ws is not None and stream is not None:
            ws.record_stream(stream)  # freed on return: not to be reused before the stream is done with it
    return rec, (order[:n] if group else None), count


def rx_verify_deliver_batch(d_bytes, d_off, flags: int = 0, filter: RxFilter | None = None,
                            ports: RxPorts | None = None, group: bool = True, stream=None):
    """The receive check and the delivery records from ONE read of each frame
    (lnx_rx_verify_deliver_batch): returns (ok, verdict, rec, order, count) —
    ok and verdict as rx_verify_batch gives them, rec / order / count as
    rx_deliver_batch gives them behind it.  flags: VERIFY_EVIL_BIT | VERIFY_ICMP
    | RX_NO_FCS.  Without ``group`` order and count are None and no workspace is
    allocated."""
    import torch
    what = "lnx_rx_verify_deliver_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    if n < 0:
        raise LnetoError(f"{what}: d_off holds no offset")
    ok = torch.empty(n, dtype=torch.uint8, device=b.device)
    verdict = torch.empty(n, dtype=torch.uint8, device=b.device)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=b.device)
    order = count = ws = None
    if group:
        order = torch.empty(max(n, 1), dtype=torch.int32, device=b.device)  # (n = 0: still a pointer to pass)
        count = torch.empty(H_COUNT + 1, dtype=torch.int32, device=b.device)
        ws = torch.empty(rx_deliver_ws_bytes(n), dtype=torch.uint8, device=b.device)
    with b as s:
        _check(lib.lnx_rx_verify_deliver_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags,
                                               ctypes.byref(filter) if filter is not None else None,
                                               ctypes.byref(ports) if ports is not None else None,
                                               ok.data_ptr(), verdict.data_ptr(), rec.data_ptr(),
                                               order.data_ptr() if group else None,
                                               count.data_ptr() if group else None, ws.data_ptr() if group else None, s),
               what)
        if ws is not None and stream is not None:
            ws.record_stream(stream)  # freed on return: not to be reused before the stream is done with it
    return ok, verdict, rec, (order[:n] if group else None), count


# ------------------------------------------------------- RST replies
TX_FCS = 2  # LNX_TX_FCS
TCP_RST, TCP_ACK = 0x04, 0x10  # tcp.FlagRST, tcp.FlagACK


def ip4_id_chain(ip4_first: int, ip_id: int, n: int) -> list:
    """The IP IDs of the next n packets of a stack whose ipID is ip_id (lnx_ip4_id_chain):
    Prand16((id + 1) ^ ip4[0]) step by step (internet/stack-ip4.go:189-195)."""
    out = (ctypes.c_uint16 * max(n, 1))()
    lib.lnx_ip4_id_chain(ip4_first & 0xFF, ip_id & 0xFFFF, n, out)
    return list(out[:n])


def _rst_entry_dict(e: TcpRst) -> dict:
    return dict(remote_addr=bytes(e.remote_addr), remote_port=e.remote_port, local_port=e.local_port, seq=e.seq,
                ack=e.ack, flags=e.flags)


def rx_rst_entry(frame: bytes, rec) -> dict | None:
    """The RST entry ONE frame (FCS stripped) queues under its delivery record
    (lnx_rx_rst_entry), None for none.  rec: rx_deliver's dict, or the 16 record bytes."""
    raw = _record_bytes("rx_rst_entry", rec)
    buf = bytes(frame)
    e = TcpRst()
    rc = lib.lnx_rx_rst_entry(buf, len(buf), raw, ctypes.byref(e))
    if rc < 0:
        _check(rc, "lnx_rx_rst_entry")
    return _rst_entry_dict(e) if rc == 1 else None


def tcp_rst_frame(cfg: RstCfg, entry, ip_id: int) -> bytes:
    """The reply of one entry (a TcpRst, or a dict as rx_rst_entry gives) with IP ID
    ip_id (lnx_tcp_rst_frame): 64 bytes with cfg's fcs, else 60."""
    e = entry if isinstance(entry, TcpRst) else TcpRst.make(**entry)
    out = (ctypes.c_uint8 * 64)()
    n = ctypes.c_uint32(0)
    _check(lib.lnx_tcp_rst_frame(ctypes.byref(cfg), ctypes.byref(e), ip_id & 0xFFFF, out, ctypes.byref(n)),
           "lnx_tcp_rst_frame")
    return bytes(out[:n.value])


def rx_rst_ws_bytes(n: int) -> int:
    """Bytes of device workspace lnx_rx_rst_reply_batch needs for n frames."""
    return lib.lnx_rx_rst_ws_bytes(n)


def rx_rst_reply_batch(d_bytes, d_off, d_rec, cfg: RstCfg, ip_id: int | None = None, ip_ids=None, cap: int | None = None,
                       flags: int = 0, stream=None):
    """The RST replies of a batch behind rx_deliver_batch / rx_verify_deliver_batch
    on the same d_off and records (lnx_rx_rst_reply_batch): returns (reply, src,
    n_written, n_wanted).  reply is [cap, 64] uint8, reply k in row k (its first
    60 bytes without cfg's fcs), answering frame src[k] (int32, cap); rows at or
    past n_written are left as allocated.  ip_id: the stack's ipID, from which
    the chain of ``cap`` IDs is computed on the host and uploaded; or ip_ids: an
    int16 device tensor of at least ``cap`` IDs.  cap defaults to the number of
    frames.  flags: RX_NO_FCS or 0.  Synchronises to return the two counts."""
    import torch
    what = "lnx_rx_rst_reply_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_rec", d_rec, "u8"),
                      ("ip_ids", ip_ids, "i16?")], stream)
    n = d_off.numel() - 1
    if n < 0:
        raise LnetoError(f"{what}: d_off holds no offset")
    _need_len(what, "d_rec", d_rec, 16 * n)
    if (ip_id is None) == (ip_ids is None):
        raise LnetoError(f"{what}: give ip_id or ip_ids")
    cap = n if cap is None else int(cap)
    if ip_ids is None:
        import numpy as np
        ids = np.array(ip4_id_chain(cfg.ip4[0], ip_id, cap), dtype=np.uint16).view(np.int16)
        ip_ids = torch.from_numpy(ids).to(b.device)
    _need_len(what, "ip_ids", ip_ids, cap)
    reply = torch.empty((cap, 64), dtype=torch.uint8, device=b.device)
    src = torch.empty(cap, dtype=torch.int32, device=b.device)
    d_n = torch.empty(2, dtype=torch.int32, device=b.device)  # (written by every call)
    ws = torch.empty(rx_rst_ws_bytes(n), dtype=torch.uint8, device=b.device)
    with b as s:
        _check(lib.lnx_rx_rst_reply_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags, d_rec.data_ptr(),
                                          ctypes.byref(cfg), ip_ids.data_ptr() if cap else None, cap,
                                          reply.data_ptr() if cap else None, src.data_ptr() if cap else None,
                                          d_n.data_ptr(), ws.data_ptr(), s), what)
        if stream is not None:
            for t in (ws, ip_ids):
                t.record_stream(stream)
            stream.synchronize()
        counts = d_n.cpu().numpy().view("uint32")
    return reply, src, int(counts[0]), int(counts[1])


def tcp_rst_frames_batch(cfg: RstCfg, d_entry, ip_ids, out=None, stream=None):
    """The replies of explicit entries (lnx_tcp_rst_frames_batch): d_entry is
    [n, 20] uint8, one lnx_tcp_rst a row (TcpRst / RST_ENTRY_DTYPE), ip_ids an int16
    device tensor of n IDs; returns reply [n, 64] uint8."""
    import torch
    what = "lnx_tcp_rst_frames_batch"
    b = _Batch(what, [("d_entry", d_entry, "u8"), ("ip_ids", ip_ids, "i16")], stream)
    if d_entry.numel() % 20:
        raise LnetoError(f"{what}: d_entry holds 20 bytes an entry")
    n = d_entry.numel() // 20
    _need_len(what, "ip_ids", ip_ids, n)
    reply = _out(what, out, 64 * n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_tcp_rst_frames_batch(ctypes.byref(cfg), d_entry.data_ptr(), n, ip_ids.data_ptr(),
                                                reply.data_ptr(), s), what)
    return reply.view(-1)[:64 * n].view(n, 64)


# ------------------------------------------------------- echo replies
def _record_bytes(what: str, rec) -> bytes:
    if isinstance(rec, dict):
        raw = (rec["ip_end"].to_bytes(4, "little") + b"".join(rec[k].to_bytes(2, "little") for k in
               ("handler", "l4_off", "src_port", "dst_port")) + bytes([rec["verdict"], rec["flags"]]) +
               rec.get("zero", 0).to_bytes(2, "little"))
    else:
        raw = bytes(rec)
    if len(raw) != 16:
        raise LnetoError(f"{what}: a delivery record is 16 bytes")
    return raw


def rx_echo_entry(frame: bytes, rec) -> dict | None:
    """The echo entry ONE frame (FCS stripped) queues under its delivery record
    (lnx_rx_echo_entry), None for none.  rec: rx_deliver's dict, or the 16 record
    bytes, from a receive check with VERIFY_ICMP."""
    raw = _record_bytes("rx_echo_entry", rec)
    buf = bytes(frame)
    e = IcmpEcho()
    rc = lib.lnx_rx_echo_entry(buf, len(buf), raw, ctypes.byref(e))
    if rc < 0:
        _check(rc, "lnx_rx_echo_entry")
    if rc != 1:
        return None
    return dict(remote_addr=bytes(e.remote_addr), id=e.id, seq=e.seq, data_off=e.data_off, data_len=e.data_len)


def icmp_echo_reply_frame(cfg: RstCfg, entry, data: bytes, ip_id: int, out_cap: int | None = None) -> bytes:
    """The reply of one entry (an IcmpEcho, or a dict as rx_echo_entry gives) whose
    data is ``data`` (frame[data_off : data_off + data_len]) with IP ID ip_id
    (lnx_icmp_echo_reply_frame): max(60, 42 + data_len) bytes, 4 more with cfg's
    fcs.  out_cap: the room offered (default: enough); too little raises with
    the library's ErrShortBuffer (6)."""
    e = entry if isinstance(entry, IcmpEcho) else IcmpEcho.make(**entry)
    data = bytes(data)
    if len(data) != e.data_len:
        raise LnetoError("icmp_echo_reply_frame: data holds data_len bytes")
    room = max(60, 42 + len(data)) + 4 if out_cap is None else int(out_cap)
    out = (ctypes.c_uint8 * max(room, 1))()
    n = ctypes.c_uint32(0)
    rc = lib.lnx_icmp_echo_reply_frame(ctypes.byref(cfg), ctypes.byref(e), data, ip_id & 0xFFFF, out, room, ctypes.byref(n))
    if rc == 6:
        raise LnetoError("lnx_icmp_echo_reply_frame failed: short buffer (6)")
    _check(rc, "lnx_icmp_echo_reply_frame")
    return bytes(out[:n.value])


def rx_echo_ws_bytes(n: int) -> int:
    """Bytes of device workspace lnx_rx_echo_reply_batch needs for n frames."""
    return lib.lnx_rx_echo_ws_bytes(n)


def rx_echo_reply_batch(d_bytes, d_off, d_rec, cfg: RstCfg, ip_id: int | None = None, ip_ids=None, flags: int = 0,
                        cap: int | None = None, cap_blocks: int | None = None, stream=None):
    """The echo replies of a batch behind rx_deliver_batch / rx_verify_deliver_batch
    (with VERIFY_ICMP) on the same d_off and records (lnx_rx_echo_reply_batch):
    returns (reply, start, length, src, written, wanted).  reply is [cap_blocks,
    64] uint8; reply k is reply.view(-1)[start[k] : start[k] + length[k]] (int64
    start, int32 length: the form fcs_verify / tx_finish_batch take), in whole
    64-byte blocks, zero past its length, and answers frame src[k] (int32);
    entries at or past ``written`` are left as allocated.  ip_id: the stack's
    ipID, from which the chain of ``cap`` IDs is computed on the host and
    uploaded (ip4_id_chain; RST and echo replies draw from ONE chain, which the
    caller splits); or ip_ids: an int16 device tensor of at least ``cap`` IDs.
    cap defaults to the number of frames, cap_blocks to what the replies of
    that many frames packed back to back in d_bytes can take.  flags:
    RX_NO_FCS or 0.  Synchronises to return the two counts."""
    import torch
    what = "lnx_rx_echo_reply_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_rec", d_rec, "u8"),
                      ("ip_ids", ip_ids, "i16?")], stream)
    n = d_off.numel() - 1
    if n < 0:
        raise LnetoError(f"{what}: d_off holds no offset")
    _need_len(what, "d_rec", d_rec, 16 * n)
    if (ip_id is None) == (ip_ids is None):
        raise LnetoError(f"{what}: give ip_id or ip_ids")
    cap = n if cap is None else int(cap)
    if cap_blocks is None:   # a reply is at most 4 bytes longer than its request, and at least one block
        cap_blocks = min(d_bytes.numel() // 64 + 2 * n, 1025 * cap)
    cap_blocks = int(cap_blocks)
    if ip_ids is None:
        import numpy as np
        ids = np.array(ip4_id_chain(cfg.ip4[0], ip_id, cap), dtype=np.uint16).view(np.int16)
        ip_ids = torch.from_numpy(ids).to(b.device)
    _need_len(what, "ip_ids", ip_ids, cap)
    reply = torch.empty((cap_blocks, 64), dtype=torch.uint8, device=b.device)
    start = torch.empty(cap, dtype=torch.int64, device=b.device)
    length = torch.empty(cap, dtype=torch.int32, device=b.device)
    src = torch.empty(cap, dtype=torch.int32, device=b.device)
    d_n = torch.empty(4, dtype=torch.int32, device=b.device)  # (written by every call)
    ws = torch.empty(rx_echo_ws_bytes(n), dtype=torch.uint8, device=b.device)
    room = cap > 0 and cap_blocks > 0
    with b as s:
        _check(lib.lnx_rx_echo_reply_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags, d_rec.data_ptr(),
                                           ctypes.byref(cfg), ip_ids.data_ptr() if room else None, cap, cap_blocks,
                                           reply.data_ptr() if room else None, start.data_ptr() if room else None,
                                           length.data_ptr() if room else None, src.data_ptr() if room else None,
                                           d_n.data_ptr(), ws.data_ptr(), s), what)
        if stream is not None:
            for t in (ws, ip_ids):
                t.record_stream(stream)
            stream.synchronize()
        counts = d_n.cpu().numpy().view("uint32")
    return reply, start, length, src, int(counts[0]), int(counts[1])


# ------------------------------------------------------- ARP
ARP_REQUEST, ARP_REPLY = 1, 2  # arp.OpRequest, arp.OpReply: the ops, and the kinds rx_arp_entry gives
# lnx_arp_seen as a numpy structured dtype (16 bytes): seen.cpu().numpy().view(ARP_SEEN_DTYPE)
try:
    ARP_SEEN_DTYPE = _np.dtype([("hw", "u1", (6,)), ("zero", "<u2"), ("ip", "u1", (4,)), ("src", "<u4")])
    assert ARP_SEEN_DTYPE.itemsize == 16
except NameError:  # pragma: no cover  (no numpy)
    ARP_SEEN_DTYPE = None


def rx_arp_entry(frame: bytes, rec, cfg: RstCfg):
    """What arp.Handler.Demux does with ONE frame (FCS stripped) under its delivery
    record (lnx_rx_arp_entry): returns (kind, entry, verdict) — kind 0 nothing,
    ARP_REQUEST a request for cfg's address, ARP_REPLY an ARP reply; entry the
    sender as dict(hw=, ip=), None for kind 0; verdict Demux's error number (0
    when the frame never reaches the handler).  rec: rx_deliver's dict, or the 16
    record bytes."""
    raw = _record_bytes("rx_arp_entry", rec)
    buf = bytes(frame)
    e = ArpEntry()
    v = ctypes.c_uint8(0)
    rc = lib.lnx_rx_arp_entry(buf, len(buf), raw, ctypes.byref(cfg), ctypes.byref(e), ctypes.byref(v))
    if rc < 0:
        _check(rc, "lnx_rx_arp_entry")
    return rc, (dict(hw=bytes(e.hw), ip=bytes(e.ip)) if rc else None), v.value


def arp_frame(cfg: RstCfg, op: int, entry) -> bytes:
    """The frame of one entry (an ArpEntry, or a dict as rx_arp_entry gives), op
    ARP_REQUEST (a query) or ARP_REPLY (lnx_arp_frame): 64 bytes with cfg's fcs, else 60."""
    e = entry if isinstance(entry, ArpEntry) else ArpEntry.make(**entry)
    out = (ctypes.c_uint8 * 64)()
    n = ctypes.c_uint32(0)
    _check(lib.lnx_arp_frame(ctypes.byref(cfg), op & 0xFFFF, ctypes.byref(e), out, ctypes.byref(n)), "lnx_arp_frame")
    return bytes(out[:n.value])


def rx_arp_ws_bytes(n: int) -> int:
    """Bytes of device workspace lnx_rx_arp_batch needs for n frames."""
    return lib.lnx_rx_arp_ws_bytes(n)


def rx_arp_batch(d_bytes, d_off, d_rec, cfg: RstCfg, cap: int | None = None, cap_seen: int | None = None, flags: int = 0,
                 stream=None):
    """The ARP replies and learn records of a batch behind rx_deliver_batch /
    rx_verify_deliver_batch on the same d_off and records (lnx_rx_arp_batch):
    returns (reply, src, seen, counts).  reply is [cap, 64] uint8, reply k in row
    k (its first 60 bytes without cfg's fcs), answering frame src[k] (int32, cap);
    seen is [cap_seen, 16] uint8, one lnx_arp_seen a row
    (seen.cpu().numpy().view(ARP_SEEN_DTYPE)); counts = (replies written, replies
    wanted, seen written, seen wanted); rows at or past what was written are left
    as allocated.  Both capacities default to the number of frames.  flags:
    RX_NO_FCS or 0.  Synchronises to return the counts."""
    import torch
    what = "lnx_rx_arp_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_rec", d_rec, "u8")], stream)
    n = d_off.numel() - 1
    if n < 0:
        raise LnetoError(f"{what}: d_off holds no offset")
    _need_len(what, "d_rec", d_rec, 16 * n)
    cap = n if cap is None else int(cap)
    cap_seen = n if cap_seen is None else int(cap_seen)
    reply = torch.empty((cap, 64), dtype=torch.uint8, device=b.device)
    src = torch.empty(cap, dtype=torch.int32, device=b.device)
    seen = torch.empty((cap_seen, 16), dtype=torch.uint8, device=b.device)
    d_n = torch.empty(4, dtype=torch.int32, device=b.device)  # (written by every call)
    ws = torch.empty(rx_arp_ws_bytes(n), dtype=torch.uint8, device=b.device)
    with b as s:
        _check(lib.lnx_rx_arp_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, flags, d_rec.data_ptr(), ctypes.byref(cfg),
                                    cap, cap_seen, reply.data_ptr() if cap else None, src.data_ptr() if cap else None,
                                    seen.data_ptr() if cap_seen else None, d_n.data_ptr(), ws.data_ptr(), s), what)
        if stream is not None:
            ws.record_stream(stream)
            stream.synchronize()
        counts = d_n.cpu().numpy().view("uint32")
    return reply, src, seen, tuple(int(c) for c in counts)


def arp_frames_batch(cfg: RstCfg, d_entry, d_op, out=None, stream=None):
    """The frames of explicit entries (lnx_arp_frames_batch): d_entry is [n, 12]
    uint8, one lnx_arp_entry a row (ArpEntry), d_op an int16 device tensor of n
    ops (ARP_REQUEST / ARP_REPLY; any other op gives an all-zero slot); returns
    reply [n, 64] uint8."""
    import torch
    what = "lnx_arp_frames_batch"
    b = _Batch(what, [("d_entry", d_entry, "u8"), ("d_op", d_op, "i16")], stream)
    if d_entry.numel() % 12:
        raise LnetoError(f"{what}: d_entry holds 12 bytes an entry")
    n = d_entry.numel() // 12
    _need_len(what, "d_op", d_op, n)
    reply = _out(what, out, 64 * n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_arp_frames_batch(ctypes.byref(cfg), d_entry.data_ptr(), d_op.data_ptr(), n, reply.data_ptr(), s),
                   what)
    return reply.view(-1)[:64 * n].view(n, 64)


PCAP_IP_HDR_BAD, PCAP_PROTO_BAD = 1, 2  # LNX_PCAP_IP_HDR_BAD, LNX_PCAP_PROTO_BAD


def pcap_checksums(frame: bytes) -> int:
    """pcap's checksum findings for ONE Ethernet frame on the host
    (lnx_pcap_checksums, internet/pcap/capture.go:67-277): PCAP_IP_HDR_BAD |
    PCAP_PROTO_BAD | code << 2."""
    buf = bytes(frame)
    rc = lib.lnx_pcap_checksums(buf, len(buf))
    if rc < 0:
        _check(rc, "lnx_pcap_checksums")
    return rc


def pcap_verify_batch(d_bytes, d_off, out=None, stream=None):
    """pcap's checksum findings per Ethernet frame d_bytes[d_off[i]:d_off[i+1]]
    (lnx_pcap_verify_batch): a uint8 status tensor, as pcap_checksums."""
    import torch
    what = "lnx_pcap_verify_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], stream)
    n = d_off.numel() - 1
    out = _out(what, out, n, torch.uint8, "u8", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_pcap_verify_batch(d_bytes.data_ptr(), d_off.data_ptr(), n, out.data_ptr(), s), what)
    return out


def sum16_batch(d_bytes, d_off, d_len, d_seed=None, out=None, stream=None):
    """CRC791{seed[i]}.PayloadSum16(d_bytes[off[i]:off[i]+len[i]]) on the GPU.

    d_off: int64 (N), d_len: int32 (N), d_seed: int32 (N) or None.  Returns int16 (uint16 bits).
    """
    import torch
    what = "lnx_sum16_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_len", d_len, "i32"),
                      ("d_seed", d_seed, "i32?")], stream)
    n = d_off.numel()
    _need_len(what, "d_len", d_len, n)
    _need_len(what, "d_seed", d_seed, n)
    out = _out(what, out, n, torch.int16, "i16", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_sum16_batch(d_bytes.data_ptr(), d_off.data_ptr(), d_len.data_ptr(),
                                       d_seed.data_ptr() if d_seed is not None else None, n,
                                       out.data_ptr(), s), what)
    return out


def sum_partial_batch(d_bytes, d_off, d_len, d_seed=None, d_phase=None, out=None, stream=None):
    """The raw 32-bit running sums of N segments on the GPU (lnx_sum_partial_batch):
    out[i] = sum_partial(d_seed[i] or 0, d_bytes[off[i]:off[i]+len[i]], d_phase[i] or 0).

    d_off: int64 (N), d_len: int32 (N), d_seed: int32 (N) or None, d_phase: uint8
    (N, bit 0 read) or None.  ``out`` must not overlap d_seed; a running sum over
    several calls ping-pongs two arrays.  sum16_batch with d_seed = a raw sum and
    zero lengths is Sum16() of it.  Returns int32 (uint32 bits)."""
    import torch
    what = "lnx_sum_partial_batch"
    b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64"), ("d_len", d_len, "i32"),
                      ("d_seed", d_seed, "i32?"), ("d_phase", d_phase, "u8?")], stream)
    n = d_off.numel()
    _need_len(what, "d_len", d_len, n)
    _need_len(what, "d_seed", d_seed, n)
    _need_len(what, "d_phase", d_phase, n)
    out = _out(what, out, n, torch.int32, "i32", b.device)
    if n > 0:
        with b as s:
            _check(lib.lnx_sum_partial_batch(d_bytes.data_ptr(), d_off.data_ptr(), d_len.data_ptr(), _ptr(d_seed),
                                             _ptr(d_phase), n, out.data_ptr(), s), what)
    return out


def sum16_chain_batch(d_bytes, d_start, d_len, d_first, d_seed=None, out16=True, sum32=False, seg_eo=None, nseg=None,
                      stream=None):
    """Internet checksum of frames made of segments (lnx_sum16_chain_batch; the
    layout of crc32_chain_batch): out16[f] = CRC791{d_seed[f] or 0}.PayloadSum16(
    frame f), sum32[f] = the raw 32-bit sum before the fold.  ``out16`` /
    ``sum32``: a tensor (int16 / int32, nframes) to write, True to allocate one,
    False for none (NULL in the C-ABI; not both).  ``seg_eo`` (int32, 2 * nseg)
    is the workspace, allocated when None and left holding every segment's sum
    of even-offset bytes in [0, nseg) and of odd-offset bytes in [nseg, 2 nseg).
    Returns (out16 or None, sum32 or None)."""
    import torch
    what = "lnx_sum16_chain_batch"
    if (out16 is False or out16 is None) and (sum32 is False or sum32 is None):
        raise LnetoError(f"{what}: one of out16 and sum32 is required")
    b, nseg, nframes, seg_eo = _chain_args(what, d_bytes, d_start, d_len, d_first, d_seed, seg_eo, nseg, stream, 2)
    o16 = None if out16 is False or out16 is None else _out(what, None if out16 is True else out16, nframes,
                                                             torch.int16, "i16", b.device)
    s32 = None if sum32 is False or sum32 is None else _out(what, None if sum32 is True else sum32, nframes,
                                                             torch.int32, "i32", b.device)
    if nframes > 0:
        with b as s:
            _check(lib.lnx_sum16_chain_batch(d_bytes.data_ptr(), d_start.data_ptr(), d_len.data_ptr(), nseg,
                                             d_first.data_ptr(), nframes, _ptr(d_seed), seg_eo.data_ptr(), _ptr(o16),
                                             _ptr(s32), s), what)
    return o16, s32


def crc32_batch_multi(parts, devices):
    """lnx_crc32_batch_multi: one host thread per entry of ``devices``; part g is
    a (d_bytes, d_off) pair on device ``devices[g]`` (offsets local to its own
    buffer).  Synchronous; returns one int32 CRC tensor per part.  The same
    device may appear more than once (a one-GPU rehearsal of the partition)."""
    import torch
    what = "lnx_crc32_batch_multi"
    if len(parts) != len(devices) or not parts:
        raise LnetoError(f"{what}: one (d_bytes, d_off) part per device")
    outs = []
    for g, (d_bytes, d_off) in enumerate(parts):
        b = _Batch(what, [("d_bytes", d_bytes, "u8"), ("d_off", d_off, "i64")], None)
        if b.device.index != devices[g]:
            raise LnetoError(f"{what}: part {g} is on {b.device}, devices[{g}] = {devices[g]}")
        outs.append(torch.empty(max(d_off.numel() - 1, 0), dtype=torch.int32, device=b.device))
    ng = len(parts)
    devs = (ctypes.c_int * ng)(*devices)
    bp = (ctypes.c_void_p * ng)(*[p[0].data_ptr() for p in parts])
    op = (ctypes.c_void_p * ng)(*[p[1].data_ptr() for p in parts])
    ns = (ctypes.c_uint64 * ng)(*[max(p[1].numel() - 1, 0) for p in parts])
    cp = (ctypes.c_void_p * ng)(*[o.data_ptr() for o in outs])
    for d in set(devices):  # the library's threads use the null stream: order after torch's work
        torch.cuda.synchronize(d)
    _check(lib.lnx_crc32_batch_multi(ng, devs, bp, op, ns, cp), what)
    return outs


def crc32_batch_host(h_bytes, h_off, device: int = 0):
    """Host-memory convenience (H2D + kernel + D2H); numpy uint8 / uint64 in, uint32 out."""
    import numpy as np
    h_bytes = np.ascontiguousarray(h_bytes, dtype=np.uint8)
    h_off = np.ascontiguousarray(h_off, dtype=np.uint64)
    n = len(h_off) - 1
    out = np.zeros(max(n, 1), dtype=np.uint32)
    if n > 0:
        _check(lib.lnx_crc32_batch_host(h_bytes.ctypes.data, h_bytes.nbytes, h_off.ctypes.data, n,
                                        out.ctypes.data, device), "lnx_crc32_batch_host")
    return out[:max(n, 0)]


class RxRing:
    """Pinned receive ring + batched FCS verify / ingress verdicts (lnx_rx_ring_*,
    SURVEY.md §8(f).1), the batch form of netdev.Stack.IngressPackets
    (x/netdev/interface.go:82-89) over bufferSelect-style slots (x/netdev/buffer.go).

    ``slots`` is a (nslots, slot_cap) uint8 numpy view of the pinned slot memory
    and ``lengths`` a uint32 view of the per-slot buffer lengths: a producer
    writes frames (with their FCS) there, then ``ingress(first, count, offset)``
    returns (fcs_ok, verdict) uint8 arrays.  ``ingress_packets(bufs, offset)``
    takes caller-owned buffers instead (IngressPackets(bufs, offset) exactly).
    """

    def __init__(self, nslots: int, slot_cap: int = 2048, batch_slots: int = 0, depth: int = 3, device: int = 0,
                 host_threshold: int | None = None):
        import numpy as np
        h = _vp()
        _check(lib.lnx_rx_ring_create(device, nslots, slot_cap, batch_slots, depth, ctypes.byref(h)),
               "lnx_rx_ring_create")
        self._h = h
        if host_threshold is not None:
            self.set_host_threshold(host_threshold)
        self.nslots, self.slot_cap = nslots, slot_cap
        sp = lib.lnx_rx_ring_slots(h)
        lp = lib.lnx_rx_ring_lengths(h)
        self.slots = np.ctypeslib.as_array((ctypes.c_uint8 * (nslots * slot_cap)).from_address(sp)).reshape(
            nslots, slot_cap)
        self.lengths = np.ctypeslib.as_array((ctypes.c_uint32 * nslots).from_address(lp))

    def set_host_threshold(self, frames: int) -> None:
        """Batches of fewer frames run on the host, no launch (lnx_rx_ring_set_host_threshold;
        HOST_BATCH_DEFAULT unless set; 0 = every batch on the GPU)."""
        _check(lib.lnx_rx_ring_set_host_threshold(self._h, frames), "lnx_rx_ring_set_host_threshold")

    def stats(self) -> dict:
        """{host_frames, device_frames, device_batches, zero_copy_frames} since creation (lnx_rx_ring_stats)."""
        c = (ctypes.c_uint64 * 4)()
        _check(lib.lnx_rx_ring_stats(self._h, c), "lnx_rx_ring_stats")
        return {"host_frames": c[0], "device_frames": c[1], "device_batches": c[2], "zero_copy_frames": c[3]}

    def set_zero_copy(self, on: bool) -> None:
        """Kernels read (egress: patch) frames in place in the pinned slots (the default), or
        copy them through staging (lnx_rx_ring_set_zero_copy)."""
        _check(lib.lnx_rx_ring_set_zero_copy(self._h, int(bool(on))), "lnx_rx_ring_set_zero_copy")

    def set_filter(self, filt: RxFilter | None) -> None:
        """The ring's stack configuration (lnx_rx_ring_set_filter); None = accept-all."""
        _check(lib.lnx_rx_ring_set_filter(self._h, ctypes.byref(filt) if filt is not None else None),
               "lnx_rx_ring_set_filter")

    def ingress(self, first: int = 0, count: int | None = None, offset: int = 0, flags: int = 0):
        import numpy as np
        if count is None:
            count = self.nslots - first
        ok = np.zeros(max(count, 1), dtype=np.uint8)
        verdict = np.zeros(max(count, 1), dtype=np.uint8)
        _check(lib.lnx_rx_ring_ingress(self._h, first, count, offset, flags, ok.ctypes.data, verdict.ctypes.data),
               "lnx_rx_ring_ingress")
        return ok[:count], verdict[:count]

    def ingress_packets(self, bufs, offset: int = 0, flags: int = 0):
        import numpy as np
        if not isinstance(offset, int) or not 0 <= offset < 2**32:
            raise LnetoError("ingress_packets: offset must be an int in [0, 2**32)")
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray)
                else np.ascontiguousarray(b, dtype=np.uint8) for b in bufs]
        n = len(arrs)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = np.array([a.size for a in arrs] or [0], dtype=np.uint32)
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib.lnx_ingress_packets(self._h, ptrs, lens.ctypes.data, n, offset, flags, ok.ctypes.data,
                                       verdict.ctypes.data), "lnx_ingress_packets")
        return ok[:n], verdict[:n]

    def set_ports(self, ports: RxPorts | None) -> None:
        """The ring's StackPorts tables for its deliver entries (lnx_rx_ring_set_ports;
        a copy is kept); None = every port has a handler, the default."""
        _check(lib.lnx_rx_ring_set_ports(self._h, ctypes.byref(ports) if ports is not None else None),
               "lnx_rx_ring_set_ports")

    def ingress_deliver(self, first: int = 0, count: int | None = None, offset: int = 0, flags: int = 0,
                        group: bool = True):
        """ingress() plus each frame's delivery record from the same read
        (lnx_rx_ring_ingress_deliver): returns (fcs_ok, verdict, rec, order, count) —
        rec a DELIVERY_DTYPE array; with ``group`` order (uint32) lists the call's
        frames by ascending handler id in arrival order and count (H_COUNT + 1) the
        buckets' sizes, else both are None."""
        import numpy as np
        if count is None:
            count = self.nslots - first
        ok = np.zeros(max(count, 1), dtype=np.uint8)
        verdict = np.zeros(max(count, 1), dtype=np.uint8)
        rec = np.zeros(max(count, 1), dtype=DELIVERY_DTYPE)
        order = np.zeros(max(count, 1), dtype=np.uint32) if group else None
        cnt = np.zeros(H_COUNT + 1, dtype=np.uint32) if group else None
        _check(lib.lnx_rx_ring_ingress_deliver(self._h, first, count, offset, flags, ok.ctypes.data, verdict.ctypes.data,
                                               rec.ctypes.data, order.ctypes.data if group else None,
                                               cnt.ctypes.data if group else None), "lnx_rx_ring_ingress_deliver")
        return ok[:count], verdict[:count], rec[:count], (order[:count] if group else None), cnt

    def ingress_packets_deliver(self, bufs, offset: int = 0, flags: int = 0, group: bool = True):
        """ingress_packets() plus the delivery records (lnx_ingress_packets_deliver):
        returns (fcs_ok, verdict, rec, order, count) as ingress_deliver."""
        import numpy as np
        if not isinstance(offset, int) or not 0 <= offset < 2**32:
            raise LnetoError("ingress_packets_deliver: offset must be an int in [0, 2**32)")
        arrs = [np.frombuffer(bytes(b), dtype=np.uint8) if not isinstance(b, np.ndarray)
                else np.ascontiguousarray(b, dtype=np.uint8) for b in bufs]
        n = len(arrs)
        ptrs = (ctypes.c_void_p * max(n, 1))(*[a.ctypes.data if a.size else None for a in arrs])
        lens = np.array([a.size for a in arrs] or [0], dtype=np.uint32)
        ok = np.zeros(max(n, 1), dtype=np.uint8)
        verdict = np.zeros(max(n, 1), dtype=np.uint8)
        rec = np.zeros(max(n, 1), dtype=DELIVERY_DTYPE)
        order = np.zeros(max(n, 1), dtype=np.uint32) if group else None
        cnt = np.zeros(H_COUNT + 1, dtype=np.uint32) if group else None
        _check(lib.lnx_ingress_packets_deliver(self._h, ptrs, lens.ctypes.data, n, offset, flags, ok.ctypes.data,
                                               verdict.ctypes.data, rec.ctypes.data,
                                               order.ctypes.data if group else None,
                                               cnt.ctypes.data if group else None), "lnx_ingress_packets_deliver")
        return ok[:n], verdict[:n], rec[:n], (order[:n] if group else None), cnt

    def egress_packets(self, bufs, sizes, offset: int = 0, capacity: int | None = None,
                       flags: int = 3):
        """EgressPackets(bufs, sizes, offset) for the device's part of the transmit
        path (lnx_egress_packets): bufs are writable uint8 numpy arrays, frame k =
        bufs[k][offset : offset + sizes[k]]; flags TX_CHECKSUM | TX_FCS.  The frames
        are finished in place; returns (new sizes, status) as uint32 / uint8 arrays."""
        import numpy as np
        n = len(bufs)
        if not isinstance(offset, int) or not 0 <= offset < 2**32:
            raise LnetoError("egress_packets: offset must be an int in [0, 2**32)")
        if not isinstance(capacity, (int, type(None))) or (capacity is not None and not 0 <= capacity < 2**32):
            raise LnetoError("egress_packets: capacity must be an int in [0, 2**32)")
        for b in bufs:
            if not isinstance(b, np.ndarray) or b.dtype != np.uint8 or not b.flags.c_contiguous \
                    or not b.flags.writeable:
                raise LnetoError("egress_packets: bufs must be writable contiguous uint8 numpy arrays")
        if capacity is None:
            capacity = self.slot_cap
        sz = np.asarray(sizes)
        if sz.size and (sz.dtype.kind not in "iu" or sz.min() < 0 or sz.max() >= 2**32):
            raise LnetoError("egress_packets: sizes must be non-negative integers below 2**32")
        lens = np.ascontiguousarray(sz.astype(np.uint32)).copy()
        if len(lens) != n:
            raise LnetoError("egress_packets: one size per buffer")
        for b, l in zip(bufs, lens):  # the finished frame is written back at bufs[k][offset:]
            if b.size - offset < min(capacity, max(int(l), 60) + 4):
                raise LnetoError("egress_packets: each buffer needs room for its padded frame and FCS "
                                 "(min(capacity, max(size, 60) + 4) bytes from offset)")
        ptrs = (ctypes.c_void_p * max(n, 1))(*[b.ctypes.data for b in bufs])
        status = np.zeros(max(n, 1), dtype=np.uint8)
        _check(lib.lnx_egress_packets(self._h, ptrs, lens.ctypes.data, n, offset, capacity, flags,
                                      status.ctypes.data), "lnx_egress_packets")
        return lens[:n], status[:n]

    def close(self) -> None:
        if getattr(self, "_h", None):
            self.slots = self.lengths = None
            lib.lnx_rx_ring_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()


RESEARCH_LIB_PATH = os.path.join(HERE, "liblneto_amd_research.so")
_research = None


def research_lib():
    """The research library (liblneto_amd_research.so): the same C-ABI plus the
    losing kernel variants and the lnx__* profiling hooks of DESIGN.md §3-4.
    Only tools/ and the variant tests use it; the product path never does."""
    global _research
    if _research is None:
        if not os.path.exists(RESEARCH_LIB_PATH):
            raise ImportError(f"{RESEARCH_LIB_PATH} is not built (make -C lneto_amd/csrc)")
        _research = ctypes.CDLL(RESEARCH_LIB_PATH)
    return _research


def device_count() -> int:
    return lib.lnx_device_count()


def version() -> str:
    return lib.lnx_version().decode()


def _elf_section(path: str, name: str) -> bytes:
    """Bytes of section `name` of the ELF64 little-endian file at `path`."""
    import struct
    with open(path, "rb") as fh:
        blob = fh.read()
    if blob[:4] != b"\x7fELF" or blob[4] != 2 or blob[5] != 1:
        raise ValueError(f"{path}: not an ELF64 little-endian file")
    shoff, = struct.unpack_from("<Q", blob, 0x28)
    shentsize, shnum, shstrndx = struct.unpack_from("<HHH", blob, 0x3A)
    def sh(i):
        return struct.unpack_from("<IIQQQQIIQQ", blob, shoff + i * shentsize)
    stroff = sh(shstrndx)[4]
    for i in range(shnum):
        nm, _, _, _, off, size = sh(i)[:6]
        end = blob.index(b"\0", stroff + nm)
        if blob[stroff + nm:end].decode() == name:
            return blob[off:off + size]
    raise KeyError(f"{path}: no section {name}")


def build_id(path: str | None = None) -> str:
    """sha256 (16 hex digits) of the gfx950 code objects (.hip_fatbin) of the
    loaded library: the kernels' identity, unlike version(), a hand-written
    string.  bench.py records it beside every line and compares it with the
    one a committed PMC pass (profiles/counters_*.json) was taken on."""
    import hashlib
    return hashlib.sha256(_elf_section(path or LIB_PATH, ".hip_fatbin")).hexdigest()[:16]
