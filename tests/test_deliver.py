"""Receive delivery on the host (no GPU): lnx_rx_deliver against the line-cited
restatement of tests/deliver_ref.py, the census of the branches the frames
reach, the shared header under sanitizers, and the batch entry's argument
checks."""
import collections
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import lneto_amd as L
from oracle import oracle as O
from tests import deliver_ref as R
from tests import framegen as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "deliver_plan_host.cpp")
FIELDS = ("ip_end", "handler", "l4_off", "src_port", "dst_port", "verdict", "flags", "zero")


def cfilter(on):
    return L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW) if on else None


def cports(ports):
    return None if ports is None else L.RxPorts.make(tcp=ports[0], udp=ports[1])


def ethertypes(on):
    return R.FILTER_KW["ethertypes"] if on else None


def pack(rec):
    return np.array([tuple(rec[k] for k in FIELDS)], dtype=L.DELIVERY_DTYPE).tobytes()


@pytest.fixture(scope="module")
def census():
    """Every (frame, setting) of the census set: label, frame, setting index,
    receive verdict, FCS result, the restatement's record and outcome tag."""
    frames = R.census_frames()
    assert len(frames) <= 5000
    ofilt = {on: R.ofilter(on) for on in (False, True)}
    v = {on: [O.ingress_verdict(f, R.VERIFY_FLAGS, ofilt[on]) for _, f in frames] for on in (False, True)}
    cases = []
    for j, (_, on, ports) in enumerate(R.SETTINGS):
        for i, (label, f) in enumerate(frames):
            fcs = R.fcs_choice(i, j)
            rec, tag = R.deliver(f, v[on][i], ethertypes(on), ports, fcs)
            cases.append((label, f, j, v[on][i], fcs, rec, tag))
    return cases


# ------------------------------------------------------------ hand-worked cases
def test_restatement_on_hand_worked_frames():
    """Records written out by hand from the reference's lines, for the restatement and the host function."""
    ports = ([22, 80, 80], [53])
    syn = G.ether(0x0800, G.ipv4(6, R.tcp_seg(40000, 80, 0x002)))          # 14 + 20 + 20 bytes
    closed = G.ether(0x0800, G.ipv4(6, R.tcp_seg(40000, 81, 0x002)))
    closed_ack = G.ether(0x0800, G.ipv4(6, R.tcp_seg(40000, 81, 0x012)))
    closed_fin = G.ether(0x0800, G.ipv4(6, R.tcp_seg(40000, 81, 0x001)))   # no SYN, no RST, no ACK
    closed_null6 = G.ether(0x86DD, G.ipv6(6, R.tcp_seg(40000, 81, 0x000)))
    dns6 = G.ether(0x86DD, G.ipv6(17, R.udp_dgram(40001, 53, b"q")))       # 14 + 40 + 9 bytes
    arp = G.ether(0x0806, bytes(28))
    want = [
        # nodeByPort: 80 sits at indices 1 and 2, the first wins
        (syn, 0, None, dict(ip_end=54, handler=R.H_TCP + 1, l4_off=34, src_port=40000, dst_port=80, verdict=0, flags=0)),
        # no node on 81: ErrPacketDrop, and a SYN alone queues a RST (stack-ports.go:70-82)
        (closed, 0, None, dict(ip_end=54, handler=R.H_NONE, l4_off=34, src_port=40000, dst_port=81, verdict=2,
                               flags=R.DLV_RST)),
        (closed_ack, 0, None, dict(ip_end=54, handler=R.H_NONE, l4_off=34, src_port=40000, dst_port=81, verdict=2, flags=0)),
        # flags&flagSYN == 0 (stack-ports.go:74): a FIN or a null segment to a closed port is dropped without a RST
        (closed_fin, 0, None, dict(ip_end=54, handler=R.H_NONE, l4_off=34, src_port=40000, dst_port=81, verdict=2, flags=0)),
        (closed_null6, 0, None, dict(ip_end=74, handler=R.H_NONE, l4_off=54, src_port=40000, dst_port=81, verdict=2,
                                     flags=R.DLV_IP6)),
        (dns6, 0, None, dict(ip_end=63, handler=R.H_UDP + 0, l4_off=54, src_port=40001, dst_port=53, verdict=0,
                             flags=R.DLV_IP6)),
        (arp, 0, None, dict(ip_end=0, handler=R.H_ETH + 2, l4_off=0, src_port=0, dst_port=0, verdict=0, flags=0)),
        # a receive verdict passes through; a bad FCS goes before it
        (syn, 3, None, dict(ip_end=0, handler=R.H_NONE, l4_off=0, src_port=0, dst_port=0, verdict=3, flags=0)),
        (syn, 15, 0, dict(ip_end=0, handler=R.H_NONE, l4_off=0, src_port=0, dst_port=0, verdict=3, flags=R.DLV_FCS)),
        # the packet would end past the frame: a verdict that is not this frame's
        (syn[:50], 0, 1, dict(ip_end=0, handler=R.H_NONE, l4_off=0, src_port=0, dst_port=0, verdict=18, flags=0)),
    ]
    for f, v_in, fcs, rec in want:
        rec = dict(rec, zero=0)
        assert R.deliver(f, v_in, R.FILTER_KW["ethertypes"], ports, fcs)[0] == rec, f.hex()
        assert L.rx_deliver(f, v_in, cfilter(True), cports(ports), fcs) == rec, f.hex()
    # without tables every port has a handler; without a filter every EtherType has one
    assert L.rx_deliver(closed, 0)["handler"] == R.H_TCP + 256
    assert L.rx_deliver(dns6, 0)["handler"] == R.H_UDP + 256
    assert L.rx_deliver(arp, 0)["handler"] == R.H_ETH + 8
    icmp = G.ether(0x0800, G.ipv4(1, G.icmp(8, b"ping")))
    assert L.rx_deliver(icmp, 0, cfilter(True), cports(ports))["handler"] == R.H_IP4 + 1


# ------------------------------------------------------------ census
def _port(label):
    return label.rsplit("/", 1)[1]


def test_census_reaches_every_branch(census):
    """Asserted on the restatement's outcomes before anything is compared: each
    rule outcome at least 8 times, for both IP versions where it exists."""
    c = collections.Counter()
    for label, f, j, v_in, fcs, rec, tag in census:
        name = R.SETTINGS[j][0]
        kind, var, port = label.split("/")
        ver = kind[-1] if kind[-1] in "46" else "-"
        c[tag, ver] += 1
        c["setting", name, tag] += 1
        if tag == "fcs":
            c["fcs_over", "zero" if v_in == 0 else "nonzero"] += 1
        if tag == "eth_slot":
            c["eth_slot", rec["handler"] - R.H_ETH] += 1
        if tag == "ip_other":
            c["ip_other", ver, rec["handler"] - (R.H_IP4 if ver == "4" else R.H_IP6)] += 1
        if tag == "hit":
            base = R.H_TCP if kind.startswith("tcp") else R.H_UDP
            c["hit", name, kind[:3], ver, rec["handler"] - base] += 1
        if tag in ("miss", "miss_rst"):
            c[tag, kind, var] += 1
        if tag == "short":
            c["short", ver, rec["ip_end"] - rec["l4_off"]] += 1
    need = []
    for ver in "46":
        need += [(t, ver) for t in ("ip_other", "short", "hit", "hit_any", "miss", "miss_rst", "vin", "fcs")]
        need += [("ip_other", ver, 1 if ver == "4" else 58), ("ip_other", ver, 47)]
        need += [("short", ver, p) for p in range(4)]           # P = 0..3 / pl = 0..3
        for l4 in ("tcp", "udp"):
            need += [("hit", "filt_full", l4, ver, k) for k in (0, 100, 255)]
            need += [("hit", "filt_dup", l4, ver, 1 if l4 == "tcp" else 0)]    # the first of the duplicates
            need += [("hit", "null_port0", l4, ver, 1 if l4 == "tcp" else 0)]  # port 0
        # the RST condition, and each term negated once
        need += [("miss_rst", f"tcp{ver}", v) for v in ("syn", "syn8", "p14")]
        need += [("miss", f"tcp{ver}", v) for v in ("synack", "synrst", "ack", "psh", "p13")]
        need += [("miss", f"tcp{ver}", v) for v in R.NO_SYN_ALONE]   # SYN clear with RST and ACK clear too
        need += [("miss", f"udp{ver}", "dgram")]
    need += [("miss_rst", "tcp6", "nib4"), ("miss_rst", "tcp6", "nib6"), ("miss", "tcp6", "nib5")]
    need += [("eth_any", "-"), ("eth_slot", "-"), ("eth_slot", 2), ("eth_slot", 3)]
    need += [("fcs_over", "zero"), ("fcs_over", "nonzero")]
    need += [("setting", name, "hit_any") for name in ("null_null", "filt_null")]
    need += [("setting", "null_empty", "miss"), ("setting", "null_empty", "miss_rst")]
    short = {k: c[k] for k in need if c[k] < 8}
    assert not short, short


def test_each_term_of_the_rst_condition_is_negated_alone(census):
    """The flag words of the closed-port TCP frames that reach the RST test
    (zero verdict, FCS not bad, P >= 14): every term of `SYN and not (RST or
    ACK)` is false in some frame in which the other terms would let the RST
    through, so no term can be dropped from the condition unnoticed."""
    words = collections.Counter()
    for label, f, j, v_in, fcs, rec, tag in census:
        if tag in ("miss", "miss_rst") and label.startswith("tcp") and rec["ip_end"] - rec["l4_off"] >= 14:
            fl = ((f[rec["l4_off"] + 12] << 8) | f[rec["l4_off"] + 13]) & 0x1FF
            words[label[3], fl & 0x16, tag] += 1
            assert (tag == "miss_rst") == (fl & 0x16 == 0x02 and f[14] >> 4 in (4, 6)), (label, hex(fl))
    for ver in "46":
        assert words[ver, 0x02, "miss_rst"] >= 8      # SYN alone
        assert words[ver, 0x00, "miss"] >= 8          # SYN clear, RST and ACK clear
        assert words[ver, 0x12, "miss"] >= 8          # SYN with ACK
        assert words[ver, 0x06, "miss"] >= 8          # SYN with RST


def test_short_buffer_frames_verify_first(census):
    """The frames that end in io.ErrShortBuffer carry no checksum field, yet their
    TCP sums verify (the builder solved an address word): verdict 0 from the
    oracle under both filters, then 6 from the port stage."""
    seen = 0
    for label, f, j, v_in, fcs, rec, tag in census:
        if "/short" in label:
            assert O.ingress_verdict(f, R.VERIFY_FLAGS, None) == 0 and O.ingress_verdict(f, R.VERIFY_FLAGS, R.ofilter(True)) == 0
            if fcs != 0:
                assert (rec["verdict"], tag) == (R.ERR_SHORT_BUFFER, "short")
                seen += 1
    assert seen >= 64


def test_host_equals_restatement(census):
    filt = {on: cfilter(on) for on in (False, True)}
    ports = [cports(p) for _, _, p in R.SETTINGS]
    for label, f, j, v_in, fcs, rec, tag in census:
        got = L.rx_deliver(f, v_in, filt[R.SETTINGS[j][1]], ports[j], fcs)
        assert got == rec, (label, R.SETTINGS[j][0], v_in, fcs, tag, f.hex())


def test_truncated_frames_with_a_zero_verdict():
    """Rule 6: every cut of a valid frame below 75 bytes, claimed good, is ErrTruncatedFrame and nothing else."""
    sweep = R.truncation_sweep()
    assert len(sweep) == 4 * 75
    blank = dict(ip_end=0, handler=R.H_NONE, l4_off=0, src_port=0, dst_port=0, verdict=18, flags=0, zero=0)
    for _, on, ports in R.SETTINGS:
        for label, f in sweep:
            assert R.deliver(f, 0, ethertypes(on), ports)[0] == blank, label
            assert L.rx_deliver(f, 0, cfilter(on), cports(ports)) == blank, label
    for name, whole in R.truncation_wholes():
        assert len(whole) > 74 and O.ingress_verdict(whole, R.VERIFY_FLAGS, R.ofilter(True)) == 0, name
        assert L.rx_deliver(whole, 0, cfilter(True), cports((R.TCP_FULL, R.UDP_FULL)))["verdict"] == 0, name


# ------------------------------------------------------------ the shared header, stand-alone
@pytest.fixture(scope="module")
def program_input(census, tmp_path_factory):
    """The truncation sweep with a zero verdict, then the census frames of one
    setting with their own verdicts and FCS results."""
    items = [(f, 0, -1) for _, f in R.truncation_sweep()]
    items += [(f, v_in, -1 if fcs is None else fcs) for label, f, j, v_in, fcs, rec, tag in census if j == 3]
    path = tmp_path_factory.mktemp("deliver_plan") / "input.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", len(R.SETTINGS)))
        for _, on, ports in R.SETTINGS:
            fh.write(bytes([on]) + bytes(cfilter(on) or L.RxFilter()))
            fh.write(bytes([ports is not None]) + bytes(cports(ports) or L.RxPorts()))
        fh.write(struct.pack("<I", len(items)))
        for f, v_in, fcs in items:
            fh.write(struct.pack("<IBb", len(f), v_in, fcs) + f)
    return path, items


def _build(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plain_output(program_input, tmp_path_factory):
    r = subprocess.run([str(_build(tmp_path_factory, "deliver_plan_host", "-O2")), str(program_input[0])],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_standalone_program_equals_library(program_input, plain_output):
    """g++'s build of deliver_plan.hpp + deliver_host.cpp gives the library's records."""
    _, items = program_input
    lines = plain_output.splitlines()
    assert len(lines) == len(items)
    filt = {on: cfilter(on) for on in (False, True)}
    ports = [cports(p) for _, _, p in R.SETTINGS]
    for (f, v_in, fcs), line in zip(items, lines):
        want = [pack(L.rx_deliver(f, v_in, filt[on], ports[j], None if fcs < 0 else fcs)).hex()
                for j, (_, on, _) in enumerate(R.SETTINGS)]
        assert line.split() == want, f.hex()
    # the sweep comes first: verdict 18 (byte 12 of the record) under every setting
    for line in lines[:4 * 75]:
        assert all(rec[24:26] == "12" for rec in line.split())


def test_standalone_program_under_sanitizers(program_input, plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan, run directly: no field
    read leaves a frame's exact-size block, and the output is the plain build's."""
    exe = _build(tmp_path_factory, "deliver_plan_host_san", "-O1", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    r = subprocess.run([str(exe), str(program_input[0])], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == plain_output


# ------------------------------------------------------------ argument errors
def test_argument_errors_need_no_device():
    out = (ctypes.c_uint8 * 16)()
    frame = bytes(60)
    bad = L.RxPorts()
    bad.n_tcp = 257
    assert L.lib.lnx_rx_deliver(frame, 60, None, ctypes.byref(bad), -1, 0, ctypes.addressof(out)) == L.LNX_EINVAL
    bad.n_tcp, bad.n_udp = 256, 257
    assert L.lib.lnx_rx_deliver(frame, 60, None, ctypes.byref(bad), -1, 0, ctypes.addressof(out)) == L.LNX_EINVAL
    bad.n_udp = 256
    assert L.lib.lnx_rx_deliver(frame, 60, None, ctypes.byref(bad), -1, 0, ctypes.addressof(out)) == L.LNX_OK
    assert L.lib.lnx_rx_deliver(frame, 60, None, None, -1, 0, None) == L.LNX_EINVAL
    assert L.lib.lnx_rx_deliver(None, 60, None, None, -1, 0, ctypes.addressof(out)) == L.LNX_EINVAL
    with pytest.raises(L.LnetoError):
        L.RxPorts.make(tcp=range(257))

    # the batch entry: pointers that are never followed (the checks come before any device call)
    p = 0x1000
    batch = L.lib.lnx_rx_deliver_batch
    bad.n_tcp, bad.n_udp = 257, 0
    assert batch(p, p, 4, 0, None, ctypes.byref(bad), None, p, p, p, p, p, None) == L.LNX_EINVAL
    assert batch(p, p, 4, 0, None, None, None, p, p, p, None, p, None) == L.LNX_EINVAL    # d_count alone NULL
    assert batch(p, p, 4, 0, None, None, None, p, p, None, p, p, None) == L.LNX_EINVAL    # d_order alone NULL
    assert batch(p, p, 1 << 32, 0, None, None, None, p, p, p, p, p, None) == L.LNX_EINVAL
    assert batch(p, p, (1 << 64) - 1, 0, None, None, None, p, p, None, None, None, None) == L.LNX_EINVAL
    assert batch(p, p, 4, 8, None, None, None, p, p, None, None, None, None) == L.LNX_EINVAL  # an unknown flag
    assert batch(p, p, 4, 0, None, None, None, p, p + 4, None, None, None, None) == L.LNX_EINVAL  # records: 16-byte aligned
    assert batch(None, None, 4, 0, None, None, None, None, None, None, None, None, None) == L.LNX_EINVAL
    assert batch(None, None, 0, 0, None, None, None, None, None, None, None, None, None) == L.LNX_OK  # nothing to do
    nine = L.RxFilter()
    nine.n_ethertypes = 9
    assert batch(p, p, 4, 0, ctypes.byref(nine), None, None, p, p, None, None, None, None) == L.LNX_EINVAL


def test_cpp_mirror_compiles_and_runs(tmp_path):
    """include/lneto_amd.hpp's Deliver / DeliverBatch / StackPortTables against the built library."""
    exe = tmp_path / "test_deliver_api"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_deliver_api.cpp"), "-o", str(exe),
                    "-L", os.path.dirname(L.LIB_PATH), "-llneto_amd", f"-Wl,-rpath,{os.path.dirname(L.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0 and "ok" in r.stdout, r.stdout + r.stderr


def test_workspace_size_grows_with_the_batch():
    """Keys (2 bytes a frame) and one histogram per workgroup of the grouping launches (at most 512)."""
    hist = 4 * (R.H_COUNT + 1)
    assert L.rx_deliver_ws_bytes(0) == hist
    assert L.rx_deliver_ws_bytes(1) == hist + 2
    assert L.rx_deliver_ws_bytes(257) == 2 * hist + 2 * 257
    assert L.rx_deliver_ws_bytes(1 << 20) == 512 * hist + 2 * (1 << 20)
