"""RST replies for SYNs to closed ports on the host (no GPU): lnx_rx_rst_entry,
lnx_tcp_rst_frame and lnx_ip4_id_chain against the line-cited restatement of
tests/reply_ref.py and the reference's own tests as known answers, the replies
through the library's receive and transmit code, the shared header under
sanitizers, and the batch entries' argument checks."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import lneto_amd as L
from oracle import oracle as O
from tests import deliver_ref as D
from tests import reply_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "reply_plan_host.cpp")
CFG = {fcs: L.RstCfg.make(mac=R.MAC, gw_mac=R.GW_MAC, ip4=R.IP4, fcs=fcs) for fcs in (False, True)}


def record_bytes(rec):
    return np.array([tuple(rec[k] for k in ("ip_end", "handler", "l4_off", "src_port", "dst_port", "verdict", "flags",
                                            "zero"))], dtype=L.DELIVERY_DTYPE).tobytes()


@pytest.fixture(scope="module")
def cases():
    """(label, frame, record) of the census under one setting, then the self-made edges."""
    census, _, _ = R.census_cases()
    return [("census", f, rec) for f, rec in census] + R.self_made_cases()


@pytest.fixture(scope="module")
def entries(cases):
    """(label, entry) of every case that queues, by the restatement."""
    return [(label, e) for label, f, rec in cases for e in [R.rst_entry(f, rec)] if e is not None]


# ------------------------------------------------------------ the reference's tests as known answers
def _unknown_port_syn(flags):
    # TestStackPorts_RSTOnUnknownPort (internet/tcplistener_test.go:458-527): 10.0.0.1:5000 -> 10.0.0.2:443, seq 700
    ip = bytearray(40)
    ip[0], ip[9] = 0x45, 6
    ip[3] = 40   # (the test hands rawBuf[:40] to StackPorts itself; here demux4's total length says so)
    ip[12:16], ip[16:20] = bytes([10, 0, 0, 1]), bytes([10, 0, 0, 2])
    ip[20:34] = struct.pack(">HHIIBB", 5000, 443, 700, 0, 0x50, flags)
    return bytes(14) + bytes(ip)


@pytest.mark.parametrize("flags", [0x02, 0x02 | 0x40 | 0x80], ids=["syn", "syn_ece_cwr"])
def test_rst_on_unknown_port(flags):
    """SYN (and SYN|ECE|CWR, :562-607) 5000 -> 443 with seq 700: source 443, destination 5000, seq 0, ack 701, RST|ACK."""
    f = _unknown_port_syn(flags)
    f = f[:12] + b"\x08\x00" + f[14:]
    rec = L.rx_deliver(f, 0, None, L.RxPorts.make(tcp=[80]))
    assert rec["verdict"] == O.ERR_PACKET_DROP and rec["flags"] == D.DLV_RST
    want = dict(remote_addr=bytes([10, 0, 0, 1]), remote_port=5000, local_port=443, seq=0, ack=701, flags=0x14)
    assert R.rst_entry(f, rec) == want
    assert L.rx_rst_entry(f, rec) == want
    cfg = L.RstCfg.make(mac=R.MAC, gw_mac=R.GW_MAC, ip4=bytes([10, 0, 0, 2]), fcs=False)
    out = L.tcp_rst_frame(cfg, want, 0x1234)
    assert len(out) == 60
    assert struct.unpack(">HHIIH", out[34:48]) == (443, 5000, 0, 701, 0x5014)
    assert out[26:34] == bytes([10, 0, 0, 2, 10, 0, 0, 1])


def test_queue_and_drain():
    """TestRSTQueue_QueueAndDrain (tcp/rst_test.go:11-59): Queue(10.0.0.1, 8080, 1234, 100, 200, RST|ACK)."""
    e = dict(remote_addr=bytes([10, 0, 0, 1]), remote_port=8080, local_port=1234, seq=100, ack=200, flags=0x14)
    for fcs in (False, True):
        out = L.tcp_rst_frame(CFG[fcs], e, 7)
        assert out == R.rst_frame(R.MAC, R.GW_MAC, R.IP4, fcs, e, 7)
        assert struct.unpack(">HHIIH", out[34:48]) == (1234, 8080, 100, 200, 0x5014)
        assert struct.unpack(">HH", out[48:50] + out[52:54]) == (0, 0)     # window, urgent pointer


def test_non_ipv4_dropped():
    """TestRSTQueue_NonIPv4Dropped (tcp/rst_test.go:103-110): a 16-byte source queues nothing."""
    by_label = {label: (f, rec) for label, f, rec in R.self_made_cases()}
    f, rec = by_label["ip6_nib6"]
    assert rec["flags"] & D.DLV_RST and L.rx_rst_entry(f, rec) is None and R.rst_entry(f, rec) is None
    f, rec = by_label["ip6_nib4"]   # demux6 never looks at the nibble: the IPv4 offsets of an IPv6 packet
    assert L.rx_rst_entry(f, rec)["remote_addr"] == f[26:30]
    with pytest.raises(L.LnetoError):
        L.TcpRst.make(remote_addr=bytes(16), remote_port=80, local_port=1234, seq=0, ack=0, flags=4)


# ------------------------------------------------------------ entries and frames against the restatement
def test_census_holds_queueing_frames(cases):
    queueing = [f for label, f, rec in cases if label == "census" and R.rst_entry(f, rec) is not None]
    flagged = [f for label, f, rec in cases if label == "census" and rec["flags"] & D.DLV_RST]
    assert len(queueing) > 20
    assert len(flagged) > len(queueing)   # IPv6 SYNs: flagged, and no reply


def test_entries_equal_restatement(cases):
    seen = set()
    for label, f, rec in cases:
        want = R.rst_entry(f, rec)
        assert L.rx_rst_entry(f, rec) == want, (label, rec, f.hex())
        assert L.rx_rst_entry(f, record_bytes(rec)) == want, label
        seen.add((label, want is not None))
    made = {label: q for label, q in seen if label != "census"}
    assert all(made[f"ihl{i}"] for i in range(5, 16)) and made["ack_wrap"] and made["ip6_nib4"]
    assert made["l4_ends_frame"] and made["len30"] and made["len30_l4_22"]
    for label in ("ip6_nib6", "nib0_forced", "nib5_forced", "nib15_forced", "l4_past_frame", "l4_far", "len29", "len0",
                  "unflagged"):
        assert not made[label], label


def test_self_made_entries_by_hand():
    by_label = {label: (f, rec) for label, f, rec in R.self_made_cases()}
    assert L.rx_rst_entry(*by_label["ack_wrap"])["ack"] == 0
    for ihl in range(5, 16):
        e = L.rx_rst_entry(*by_label[f"ihl{ihl}"])
        assert (e["ack"], e["remote_port"], e["local_port"], e["seq"], e["flags"]) == (1001 + ihl, 5000, 443, 0, 0x14)
        assert e["remote_addr"] == bytes([192, 168, 10, 1])
    f, rec = by_label["len30"]
    assert L.rx_rst_entry(f, rec)["ack"] == (int.from_bytes(f[18:22], "big") + 1) & 0xFFFFFFFF


def test_frames_equal_restatement(entries):
    assert len(entries) > 30
    for k, (label, e) in enumerate(entries):
        ip_id = (0x9E37 * (k + 1)) & 0xFFFF
        for fcs in (False, True):
            got = L.tcp_rst_frame(CFG[fcs], e, ip_id)
            assert len(got) == (64 if fcs else 60)
            assert got == R.rst_frame(R.MAC, R.GW_MAC, R.IP4, fcs, e, ip_id), (label, e, fcs)
    # without the FCS the slot's last dword is zero
    out = (ctypes.c_uint8 * 64)(*([0xAA] * 64))
    n = ctypes.c_uint32(0)
    e = L.TcpRst.make(**entries[0][1])
    assert L.lib.lnx_tcp_rst_frame(ctypes.byref(CFG[False]), ctypes.byref(e), 1, out, ctypes.byref(n)) == L.LNX_OK
    assert n.value == 60 and bytes(out[60:]) == bytes(4)
    # every flag bit above 0x1ff is masked (SetOffsetAndFlags)
    hi = dict(entries[0][1], flags=0xFE14)
    assert L.tcp_rst_frame(CFG[True], hi, 1) == L.tcp_rst_frame(CFG[True], dict(hi, flags=0x14), 1)


def test_replies_through_the_librarys_own_code(entries):
    """Every reply is a frame the peer's stack accepts, its FCS verifies, and the
    transmit path's checksum and FCS steps reproduce it from the bare headers."""
    for k, (label, e) in enumerate(entries):
        out = L.tcp_rst_frame(CFG[True], e, 0x0100 + k)
        peer = L.RxFilter.make(mac=R.GW_MAC, ip4=e["remote_addr"])
        assert L.lib.lnx_ingress_verdict(out[:60], 60, L.VERIFY_EVIL_BIT | L.VERIFY_ICMP, ctypes.byref(peer)) == 0, label
        assert L.crc32(out) == L.CRC32_RESIDUE
        bare = bytearray(out[:54])
        bare[24:26] = bare[50:52] = b"\0\0"
        bare[16:18] = b"\0\0"   # the total length too: the checksum step writes it
        buf = (ctypes.c_uint8 * 64).from_buffer_copy(bytes(bare) + bytes([0xAA] * 10))
        assert L.lib.lnx_tx_checksum(ctypes.addressof(buf), 54) == 0
        n = ctypes.c_uint32(54)
        assert L.lib.lnx_fcs_append(ctypes.addressof(buf), ctypes.byref(n), 64) == 0
        assert n.value == 64 and bytes(buf) == out, label


def test_id_chain():
    for first in range(256):
        for seed in (0, 1, 0x1234, 0xFFFE, 0xFFFF):
            assert L.ip4_id_chain(first, seed, 9) == R.id_chain(first, seed, 9)
    assert L.ip4_id_chain(192, 7, 0) == []
    assert R.prand16(1) == 0x8181 and R.id_chain(0, 0, 1) == [0x8181]   # 1 -> 0x0081 -> 0x0081 -> 0x8181
    L.lib.lnx_ip4_id_chain(1, 2, 5, None)                                # a NULL out: nothing written


# ------------------------------------------------------------ the shared header, stand-alone
@pytest.fixture(scope="module")
def program_input(cases, tmp_path_factory):
    path = tmp_path_factory.mktemp("reply_plan") / "input.bin"
    chains = [(first, seed, n) for first in (0, 10, 192, 255) for seed in (0, 0xFFFF, 0x1234) for n in (0, 1, 33)]
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", 2) + bytes(CFG[False]) + bytes(CFG[True]))
        fh.write(struct.pack("<I", len(cases)))
        for k, (_, f, rec) in enumerate(cases):
            fh.write(struct.pack("<IH", len(f), (0x9E37 * (k + 1)) & 0xFFFF) + record_bytes(rec) + f)
        fh.write(struct.pack("<I", len(chains)))
        for first, seed, n in chains:
            fh.write(struct.pack("<BHI", first, seed, n))
    return path, chains


def _build(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plain_output(program_input, tmp_path_factory):
    r = subprocess.run([str(_build(tmp_path_factory, "reply_plan_host", "-O2")), str(program_input[0])],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_standalone_program_equals_library(cases, program_input, plain_output):
    """g++'s build of reply_plan.hpp + reply_host.cpp + table_images.cpp gives the library's entries and frames."""
    _, chains = program_input
    lines = plain_output.splitlines()
    assert len(lines) == len(cases) + len(chains)
    queued = 0
    for k, ((label, f, rec), line) in enumerate(zip(cases, lines)):
        e = L.rx_rst_entry(f, rec)
        if e is None:
            assert line == "-", label
            continue
        queued += 1
        ip_id = (0x9E37 * (k + 1)) & 0xFFFF
        want = [bytes(L.TcpRst.make(**e)).hex()]
        for fcs in (False, True):
            out = L.tcp_rst_frame(CFG[fcs], e, ip_id)
            want += [(out + bytes(64 - len(out))).hex(), str(len(out))]
        assert line.split() == want, label
    assert queued > 30
    for (first, seed, n), line in zip(chains, lines[len(cases):]):
        assert line == np.array(R.id_chain(first, seed, n), dtype="<u2").tobytes().hex()


def test_standalone_program_under_sanitizers(program_input, plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan, run directly: no field
    read leaves a frame's exact-size block (the cases hold frames that end at
    the last byte a rule reads), and the output is the plain build's."""
    exe = _build(tmp_path_factory, "reply_plan_host_san", "-O1", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    r = subprocess.run([str(exe), str(program_input[0])], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == plain_output


# ------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device():
    frame, rec = bytes(60), bytes(16)
    e = L.TcpRst()
    assert L.lib.lnx_rx_rst_entry(frame, 60, None, ctypes.byref(e)) == L.LNX_EINVAL
    assert L.lib.lnx_rx_rst_entry(frame, 60, rec, None) == L.LNX_EINVAL
    assert L.lib.lnx_rx_rst_entry(None, 60, rec, ctypes.byref(e)) == L.LNX_EINVAL
    assert L.lib.lnx_rx_rst_entry(None, 0, rec, ctypes.byref(e)) == 0
    out, n = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    frame_of = L.lib.lnx_tcp_rst_frame
    assert frame_of(None, ctypes.byref(e), 1, out, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(ctypes.byref(CFG[True]), None, 1, out, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(ctypes.byref(CFG[True]), ctypes.byref(e), 1, None, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(ctypes.byref(CFG[True]), ctypes.byref(e), 1, out, None) == L.LNX_EINVAL
    bad = L.RstCfg.make(mac=R.MAC, gw_mac=R.GW_MAC, ip4=R.IP4)
    bad.flags = 3   # LNX_TX_CHECKSUM is not a flag of this entry
    assert frame_of(ctypes.byref(bad), ctypes.byref(e), 1, out, ctypes.byref(n)) == L.LNX_EINVAL
    with pytest.raises(L.LnetoError):
        L.RstCfg.make(mac=R.MAC, gw_mac=R.GW_MAC, ip4=bytes(16))

    # the batch entries: pointers that are never followed (the checks come before any device call)
    p, cfg, badcfg = 0x1000, ctypes.byref(CFG[True]), ctypes.byref(bad)
    batch = L.lib.lnx_rx_rst_reply_batch
    assert batch(p, p, 1 << 32, 0, p, cfg, p, 4, p, p, p, p, None) == L.LNX_EINVAL
    assert batch(p, p, (1 << 64) - 1, 0, p, cfg, p, 4, p, p, p, p, None) == L.LNX_EINVAL
    assert batch(p, p, 4, 8, p, cfg, p, 4, p, p, p, p, None) == L.LNX_EINVAL                 # an unknown flag
    assert batch(p, p, 4, L.VERIFY_ICMP, p, cfg, p, 4, p, p, p, p, None) == L.LNX_EINVAL     # a receive-check flag
    assert batch(p, p, 4, 0, p, badcfg, p, 4, p, p, p, p, None) == L.LNX_EINVAL              # ... on the other word
    assert batch(p, p, 4, 0, p, cfg, p, 4, p + 32, p, p, p, None) == L.LNX_EINVAL            # d_reply: 64-byte aligned
    assert batch(p, p, 4, 0, p, cfg, p, 4, p + 4, p, p, p, None) == L.LNX_EINVAL
    for hole in range(9):   # a NULL pointer with work to do
        a = [p, p, p, cfg, p, p, p, p, p]
        a[hole] = None
        assert batch(a[0], a[1], 4, 0, a[2], a[3], a[4], 4, a[5], a[6], a[7], a[8], None) == L.LNX_EINVAL, hole
    assert batch(None, None, 0, 0, None, None, None, 0, None, None, None, None, None) == L.LNX_OK   # nothing to do
    assert batch(None, None, 0, 0, None, None, None, 4, None, None, None, None, None) == L.LNX_OK
    assert batch(None, None, 0, 8, None, None, None, 0, None, None, None, None, None) == L.LNX_EINVAL
    assert batch(None, None, 4, 0, None, None, None, 0, None, None, None, None, None) == L.LNX_EINVAL  # cap 0 still counts

    frames = L.lib.lnx_tcp_rst_frames_batch
    assert frames(None, None, 0, None, None, None) == L.LNX_OK
    assert frames(badcfg, None, 0, None, None, None) == L.LNX_EINVAL
    assert frames(badcfg, p, 4, p, p, None) == L.LNX_EINVAL
    assert frames(cfg, p, 4, p, p + 16, None) == L.LNX_EINVAL                                # d_reply: 64-byte aligned
    for hole in range(4):
        a = [cfg, p, p, p]
        a[hole] = None
        assert frames(a[0], a[1], 4, a[2], a[3], None) == L.LNX_EINVAL, hole


def test_workspace_size():
    """One word per workgroup of the count / build launches (at most 512)."""
    assert L.rx_rst_ws_bytes(0) == 4 and L.rx_rst_ws_bytes(256) == 4 and L.rx_rst_ws_bytes(257) == 8
    assert L.rx_rst_ws_bytes(1 << 20) == 4 * 512


def test_cpp_mirror_compiles_and_runs(tmp_path):
    """include/lneto_amd.hpp's RSTEntry / RSTFrame / IPIDChain against the built library."""
    exe = tmp_path / "test_reply_api"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_reply_api.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(L.LIB_PATH), "-llneto_amd", f"-Wl,-rpath,{os.path.dirname(L.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr
