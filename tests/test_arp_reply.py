"""ARP on the host (no GPU): lnx_rx_arp_entry and lnx_arp_frame against the
line-cited restatement of tests/arp_ref.py and the reference's own TestHandler
as known answers, the frames through the library's receive code, the shared
header under sanitizers, and the batch entries' argument checks."""
import ctypes
import os
import struct
import subprocess
import zlib

import numpy as np
import pytest

import lneto_amd as L
from tests import arp_ref as A
from tests import deliver_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "arp_plan_host.cpp")
CFG = {fcs: L.RstCfg.make(mac=A.MAC, gw_mac=A.GW_MAC, ip4=A.IP4, fcs=fcs) for fcs in (False, True)}


def record_bytes(rec):
    return np.array([tuple(rec[k] for k in ("ip_end", "handler", "l4_off", "src_port", "dst_port", "verdict", "flags",
                                            "zero"))], dtype=L.DELIVERY_DTYPE).tobytes()


@pytest.fixture(scope="module")
def cases():
    """(label, frame, record) of the census under the stack's filter, then the self-made cases."""
    return [("census", f, rec) for f, rec in A.census_cases()] + A.self_made_cases()


# ------------------------------------------------------------ the reference's test as known answers
def test_handler_exchange():
    """TestHandler (arp/arp_test.go:11-104): c1 (de:ad:be:ef:00:00, 192.168.1.1) queries 192.168.1.2, c2
    (c0:ff:ee:c0:ff:ee) answers, and c1's CacheLookup(192.168.1.2) gives c2's hardware address."""
    hw1, ip1 = bytes.fromhex("deadbeef0000"), bytes([192, 168, 1, 1])
    hw2, ip2 = bytes.fromhex("c0ffeec0ffee"), bytes([192, 168, 1, 2])
    c1 = L.RstCfg.make(mac=hw1, gw_mac=bytes(6), ip4=ip1, fcs=False)
    c2 = L.RstCfg.make(mac=hw2, gw_mac=bytes(6), ip4=ip2, fcs=False)
    query = L.arp_frame(c1, L.ARP_REQUEST, dict(hw=bytes(6), ip=ip2))   # StartQuery leaves the hw zero
    assert len(query) == 60 and query[:6] == A.BROADCAST and query[6:12] == hw1
    assert query[14:42] == struct.pack(">HHBBH", 1, 0x0800, 6, 4, 1) + hw1 + ip1 + bytes(6) + ip2
    rec = L.rx_deliver(query, 0, None, None, None)
    assert rec["handler"] == D.H_ETH + 8 and rec["verdict"] == 0
    kind, e, v = L.rx_arp_entry(query, rec, c2)                          # c2.Demux: a pending response for c1
    assert (kind, v) == (1, 0) and e == dict(hw=hw1, ip=ip1)
    assert L.rx_arp_entry(query, rec, c1)[0] == 0                        # (not for c1 itself)
    answer = L.arp_frame(c2, L.ARP_REPLY, e)
    assert answer[:6] == hw1 and answer[6:12] == hw2
    kind, seen, v = L.rx_arp_entry(answer, L.rx_deliver(answer, 0, None, None, None), c1)   # c1.Demux
    assert (kind, v) == (2, 0) and seen == dict(hw=hw2, ip=ip2)          # the CacheLookup result the Go test expects


# ------------------------------------------------------------ entries and frames against the restatement
def test_entries_equal_restatement(cases):
    seen = {}
    for label, f, rec in cases:
        want = A.arp_demux(f, rec, A.IP4)
        assert L.rx_arp_entry(f, rec, CFG[True]) == want, (label, rec, f.hex())
        assert L.rx_arp_entry(f, record_bytes(rec), CFG[False]) == want, label
        if label != "census":
            assert label not in seen, label
            seen[label] = (want[0], want[2])
    assert seen == A.EXPECT, {k: (seen.get(k), A.EXPECT.get(k)) for k in set(seen) | set(A.EXPECT) if seen.get(k) != A.EXPECT.get(k)}
    # the census holds ARP frames of both kinds under the stack's filter
    kinds = [A.arp_demux(f, rec, A.IP4)[0] for label, f, rec in cases if label == "census"]
    assert len(kinds) > 500


def test_self_made_entries_by_hand():
    by_label = {label: (f, rec) for label, f, rec in A.self_made_cases()}
    sender = dict(hw=A.PEER_MAC, ip=A.PEER_IP)
    for label in ("request_padded", "request_unpadded", "p28", "forced_len42", "null_filter", "reply_for_us", "reply_for_other"):
        assert L.rx_arp_entry(*by_label[label], CFG[True])[1] == sender, label
    assert L.rx_arp_entry(*by_label["probe_sender_zero"], CFG[True])[1] == dict(hw=A.PEER_MAC, ip=bytes(4))
    assert L.rx_arp_entry(*by_label["sender_hw_broadcast"], CFG[True])[1]["hw"] == A.BROADCAST
    assert L.rx_arp_entry(*by_label["sender_hw_multicast"], CFG[True])[1]["hw"] == bytes.fromhex("01005e000001")
    # the records of the delivered cases name the filter's 0x0806 slot; the NULL filter's is H_ETH + 8
    assert by_label["request_padded"][1]["handler"] == D.H_ETH + 2 and by_label["null_filter"][1]["handler"] == D.H_ETH + 8
    # *verdict may be NULL, and *out is untouched when nothing is returned
    e = L.ArpEntry.make(hw=b"\xaa" * 6, ip=b"\xaa" * 4)
    f, rec = by_label["op_0x3"]
    assert L.lib.lnx_rx_arp_entry(f, len(f), record_bytes(rec), ctypes.byref(CFG[True]), ctypes.byref(e), None) == 0
    assert bytes(e.hw) == b"\xaa" * 6 and bytes(e.ip) == b"\xaa" * 4
    f, rec = by_label["request_padded"]
    assert L.lib.lnx_rx_arp_entry(f, len(f), record_bytes(rec), ctypes.byref(CFG[True]), ctypes.byref(e), None) == 1
    assert bytes(e.hw) == A.PEER_MAC and e.zero == 0


def test_frames_by_hand():
    e = dict(hw=bytes.fromhex("021122334455"), ip=bytes([10, 1, 2, 3]))
    reply = L.arp_frame(CFG[False], L.ARP_REPLY, e)
    want = (e["hw"] + A.MAC + bytes.fromhex("0806") + bytes.fromhex("0001080006040002") + A.MAC + A.IP4 + e["hw"] + e["ip"] +
            bytes(18))
    assert len(want) == 60 and reply == want
    query = L.arp_frame(CFG[False], L.ARP_REQUEST, dict(hw=bytes(6), ip=e["ip"]))
    want_q = (A.BROADCAST + A.MAC + bytes.fromhex("0806") + bytes.fromhex("0001080006040001") + A.MAC + A.IP4 + bytes(6) +
              e["ip"] + bytes(18))
    assert query == want_q
    # a query carries the entry's hw as it is (StartQuery leaves it zero; the batch form does not care)
    assert L.arp_frame(CFG[False], L.ARP_REQUEST, e)[32:38] == e["hw"]
    # the gateway MAC is nowhere in these frames
    assert A.GW_MAC not in reply and A.GW_MAC not in query


def test_frames_equal_restatement(cases):
    entries = [(label, e) for label, f, rec in cases for kind, e, _ in [A.arp_demux(f, rec, A.IP4)] if kind]
    entries += [("ones", dict(hw=b"\xff" * 6, ip=b"\xff" * 4)), ("zeros", dict(hw=bytes(6), ip=bytes(4)))]
    assert len(entries) >= 12
    for label, e in entries:
        for fcs in (False, True):
            for op in (1, 2):
                got = L.arp_frame(CFG[fcs], op, e)
                assert len(got) == (64 if fcs else 60)
                assert got == A.arp_frame(A.MAC, A.IP4, fcs, op, e), (label, e, fcs, op)
                if fcs:
                    assert got[60:] == struct.pack("<I", zlib.crc32(got[:60]))
                    assert L.crc32(got) == L.CRC32_RESIDUE
    # without the FCS the slot's last dword is zero
    out = (ctypes.c_uint8 * 64)(*([0xAA] * 64))
    n = ctypes.c_uint32(0)
    e = L.ArpEntry.make(**entries[0][1])
    assert L.lib.lnx_arp_frame(ctypes.byref(CFG[False]), 2, ctypes.byref(e), out, ctypes.byref(n)) == L.LNX_OK
    assert n.value == 60 and bytes(out[60:]) == bytes(4)
    # the entry's zero field is not looked at
    e.zero = 0xBEEF
    assert L.arp_frame(CFG[True], 2, e) == L.arp_frame(CFG[True], 2, entries[0][1])


def test_frames_through_the_librarys_own_code():
    """A reply is a frame the peer's stack accepts under a filter whose MAC is the entry's hw, its FCS verifies
    (fcs_verify's host form), and the peer's ARP handler learns us from it."""
    e = dict(hw=bytes.fromhex("021122334455"), ip=bytes([192, 168, 10, 7]))
    out = L.arp_frame(CFG[True], L.ARP_REPLY, e)
    peer = L.RxFilter.make(mac=e["hw"], ethertypes=(0x0800, 0x0806), ip4=e["ip"])
    assert L.lib.lnx_ingress_verdict(out[:60], 60, L.VERIFY_EVIL_BIT | L.VERIFY_ICMP, ctypes.byref(peer)) == 0
    assert L.crc32(out) == L.CRC32_RESIDUE   # (the device's fcs_verify_batch takes the replies in tests/test_arp_reply_gpu.py)
    rec = L.rx_deliver(out[:60], 0, peer, None, 1)
    assert rec["verdict"] == 0 and rec["handler"] == D.H_ETH + 1
    pcfg = L.RstCfg.make(mac=e["hw"], gw_mac=bytes(6), ip4=e["ip"])
    assert L.rx_arp_entry(out[:60], rec, pcfg) == (2, dict(hw=A.MAC, ip=A.IP4), 0)
    # a broadcast query passes the same filter, and the peer queues its answer to us
    q = L.arp_frame(CFG[True], L.ARP_REQUEST, dict(hw=bytes(6), ip=e["ip"]))
    assert L.lib.lnx_ingress_verdict(q[:60], 60, 0, ctypes.byref(peer)) == 0
    assert L.rx_arp_entry(q[:60], L.rx_deliver(q[:60], 0, peer, None, 1), pcfg) == (1, dict(hw=A.MAC, ip=A.IP4), 0)


# ------------------------------------------------------------ the shared header, stand-alone
@pytest.fixture(scope="module")
def program_input(cases, tmp_path_factory):
    path = tmp_path_factory.mktemp("arp_plan") / "input.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", 2) + bytes(CFG[False]) + bytes(CFG[True]))
        fh.write(struct.pack("<I", len(cases)))
        for _, f, rec in cases:
            fh.write(struct.pack("<I", len(f)) + record_bytes(rec) + f)
    return path


def _build(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plain_output(program_input, tmp_path_factory):
    r = subprocess.run([str(_build(tmp_path_factory, "arp_plan_host", "-O2")), str(program_input)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_standalone_program_equals_library(cases, plain_output):
    """g++'s build of arp_plan.hpp + arp_host.cpp + table_images.cpp gives the library's kinds, verdicts, entries and frames."""
    lines = plain_output.splitlines()
    assert len(lines) == 2 * len(cases)
    some = 0
    for k, (label, f, rec) in enumerate(cases):
        for j, fcs in enumerate((False, True)):
            kind, e, v = L.rx_arp_entry(f, rec, CFG[fcs])
            want = [str(kind), str(v)]
            if kind:
                some += 1
                want.append(bytes(L.ArpEntry.make(**e)).hex())
                for op in (2, 1):
                    out = L.arp_frame(CFG[fcs], op, e)
                    want += [(out + bytes(64 - len(out))).hex(), str(len(out))]
            assert lines[2 * k + j].split() == want, (label, fcs)
    assert some >= 20


def test_standalone_program_under_sanitizers(program_input, plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan, run directly: no field
    read leaves a frame's exact-size block (the cases hold frames that end at
    the last byte a rule reads), and the output is the plain build's."""
    exe = _build(tmp_path_factory, "arp_plan_host_san", "-O1", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    r = subprocess.run([str(exe), str(program_input)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == plain_output


# ------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device():
    frame, rec = bytes(60), bytes(16)
    e, v = L.ArpEntry(), ctypes.c_uint8(0)
    cfg = ctypes.byref(CFG[True])
    entry_of = L.lib.lnx_rx_arp_entry
    assert entry_of(frame, 60, None, cfg, ctypes.byref(e), ctypes.byref(v)) == L.LNX_EINVAL
    assert entry_of(frame, 60, rec, None, ctypes.byref(e), ctypes.byref(v)) == L.LNX_EINVAL
    assert entry_of(frame, 60, rec, cfg, None, ctypes.byref(v)) == L.LNX_EINVAL
    assert entry_of(None, 60, rec, cfg, ctypes.byref(e), ctypes.byref(v)) == L.LNX_EINVAL
    assert entry_of(None, 0, rec, cfg, ctypes.byref(e), ctypes.byref(v)) == 0
    assert entry_of(frame, 60, rec, cfg, ctypes.byref(e), None) == 0
    out, n = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    frame_of = L.lib.lnx_arp_frame
    assert frame_of(None, 2, ctypes.byref(e), out, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, 2, None, out, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, 2, ctypes.byref(e), None, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, 2, ctypes.byref(e), out, None) == L.LNX_EINVAL
    for op in (0, 3, 0x0100, 0x0200, 0xFFFF):
        assert frame_of(cfg, op, ctypes.byref(e), out, ctypes.byref(n)) == L.LNX_EINVAL, op
    bad = L.RstCfg.make(mac=A.MAC, gw_mac=A.GW_MAC, ip4=A.IP4)
    bad.flags = 3   # LNX_TX_CHECKSUM is not a flag of this entry
    assert frame_of(ctypes.byref(bad), 2, ctypes.byref(e), out, ctypes.byref(n)) == L.LNX_EINVAL
    with pytest.raises(L.LnetoError):
        L.ArpEntry.make(hw=bytes(6), ip=bytes(16))
    with pytest.raises(L.LnetoError):
        L.arp_frame(CFG[True], 3, dict(hw=bytes(6), ip=bytes(4)))

    # the batch entries: pointers that are never followed (the checks come before any device call)
    p, badcfg = 0x1000, ctypes.byref(bad)
    batch = L.lib.lnx_rx_arp_batch

    def call(d_bytes=p, d_off=p, n=4, flags=0, d_rec=p, c=cfg, cap=4, cap_seen=4, d_reply=p, d_src=p, d_seen=p, d_n=p, d_ws=p):
        return batch(d_bytes, d_off, n, flags, d_rec, c, cap, cap_seen, d_reply, d_src, d_seen, d_n, d_ws, None)

    assert call(n=1 << 32) == L.LNX_EINVAL
    assert call(n=(1 << 64) - 1) == L.LNX_EINVAL
    assert call(flags=8) == L.LNX_EINVAL                    # an unknown flag
    assert call(flags=L.VERIFY_ICMP) == L.LNX_EINVAL        # a receive-check flag
    assert call(c=badcfg) == L.LNX_EINVAL                   # ... on the other word
    assert call(d_reply=p + 32) == L.LNX_EINVAL             # d_reply: 64-byte aligned
    assert call(d_rec=p + 8) == L.LNX_EINVAL                # d_rec, d_seen: 16
    assert call(d_seen=p + 8) == L.LNX_EINVAL
    for name in ("d_src", "d_n", "d_ws"):                   # the rest: 4
        assert call(**{name: p + 2}) == L.LNX_EINVAL, name
    for name in ("d_bytes", "d_off", "d_rec", "c", "d_reply", "d_src", "d_seen", "d_n", "d_ws"):   # a NULL pointer with work to do
        assert call(**{name: None}) == L.LNX_EINVAL, name
    assert call(cap=0, cap_seen=0, d_reply=None, d_src=None, d_seen=None, d_n=None) == L.LNX_EINVAL   # both caps 0 still count
    assert call(cap=4, cap_seen=0, d_seen=None, d_n=None) == L.LNX_EINVAL                             # (d_seen may be NULL here)
    assert batch(None, None, 0, 0, None, None, 0, 0, None, None, None, None, None, None) == L.LNX_OK   # nothing to do
    assert batch(None, None, 0, 0, None, None, 4, 4, None, None, None, None, None, None) == L.LNX_OK
    assert batch(None, None, 0, 8, None, None, 0, 0, None, None, None, None, None, None) == L.LNX_EINVAL

    frames = L.lib.lnx_arp_frames_batch
    assert frames(None, None, None, 0, None, None) == L.LNX_OK
    assert frames(badcfg, None, None, 0, None, None) == L.LNX_EINVAL
    assert frames(badcfg, p, p, 4, p, None) == L.LNX_EINVAL
    assert frames(cfg, p, p, 4, p + 16, None) == L.LNX_EINVAL   # d_reply: 64-byte aligned
    assert frames(cfg, p + 2, p, 4, p, None) == L.LNX_EINVAL    # d_entry: 4
    assert frames(cfg, p, p + 1, 4, p, None) == L.LNX_EINVAL    # d_op: 2
    for hole in range(4):
        a = [cfg, p, p, p]
        a[hole] = None
        assert frames(a[0], a[1], a[2], 4, a[3], None) == L.LNX_EINVAL, hole


def test_workspace_size():
    """Two words per workgroup of the count / build launches (at most 512)."""
    assert L.rx_arp_ws_bytes(0) == 8 and L.rx_arp_ws_bytes(256) == 8 and L.rx_arp_ws_bytes(257) == 16
    assert L.rx_arp_ws_bytes(1 << 20) == 8 * 512


def test_cpp_mirror_compiles_and_runs(tmp_path):
    """include/lneto_amd.hpp's arp::EntryOf / Frame against the built library."""
    exe = tmp_path / "test_arp_api"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_arp_api.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(L.LIB_PATH), "-llneto_amd", f"-Wl,-rpath,{os.path.dirname(L.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
