"""The kernels' frame parse, run on the host (no GPU).

lneto_amd/csrc/frame_plan.hpp holds the receive demux rules that the ingress
and receive-check kernels inline (rx_plan, rx_verdict, conv).
tests/cpp/frame_plan_host.cpp compiles the same header with g++, reads every
field through accessors over a heap copy of exactly the frame's bytes and takes
the sums bytewise, in the kernels' little-endian half-word form at both address
parities.  Here its receive verdicts must equal oracle.ingress_verdict on
lneto's fuzz corpus (raw and fixed) and on every frame generator of the suite,
under all four flag sets, without a filter, with two filters of
tests/test_rx_filter.py and three of tests/test_rx_filter_edges.py.  The
program is built a second time with AddressSanitizer and UBSan and run on the same input: an accessor called
outside its guard reads past the exact-size buffer."""
import json
import os
import struct
import subprocess

import pytest

import lneto_amd as L
from oracle import oracle as O
from tests import framegen as G
from tests.test_rx_filter_edges import FILTER_EDGES, frame_plan_subset

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "frame_plan_host.cpp")
FLAGS = [0, O.VERIFY_EVIL_BIT, O.VERIFY_ICMP, O.VERIFY_EVIL_BIT | O.VERIFY_ICMP]
assert FLAGS == [0, 1, 2, 3]  # the program's flag loop
# None = accept-all; "plain" is test_rx_filter._f(), "few_handlers" reaches the handler masks' zero bits
FILTERS = [None,
           dict(ip4=G.IP4_DST, ip6=G.IP6_DST),
           dict(ip4=G.IP4_DST, ip6=G.IP6_DST, ethertypes=(0x0800, 0x88CC), ip4_protocols=(17, 47), ip6_protocols=(58,))]
# ... and three of tests/test_rx_filter_edges.py: handlers in every mask word, all eight EtherType slots, a stack
# address whose only non-zero byte is the last
FILTERS += [FILTER_EDGES[name] for name in ("wide_handlers", "eight_types", "ip6_byte15")]


def _spread(items, cap):
    """At most cap of the (name, frame) items, evenly spaced (the generators order their cases by kind)."""
    items = [x[1] for x in items]
    step = max(1, -(-len(items) // cap))
    return items[::step]


@pytest.fixture(scope="module")
def frames():
    d = json.load(open(os.path.join(ROOT, "tests", "golden", "fuzz_frames.json")))
    raw = [bytes.fromhex(f["hex"]) for f in d["frames"]]
    assert len(raw) == 208
    out = raw + [O.fix_ip_tcp_crcs(f)[0] for f in raw]
    out += G.frames(count=400) + G.icmp_frames(count=300) + G.trailing_frames(count=300) + G.filter_frames(count=400)
    out += _spread(G.ip4_option_frames(), 400) + _spread(G.limit_frames(), 40)
    # every guard of the accessors: one UDP frame of each family cut at every length through its headers
    for whole in (G.ether(0x0800, G.ipv4(17, G.udp(b"guards"), opts=bytes(8))), G.ether(0x86DD, G.ipv6(17, G.udp(b"guards")))):
        out += [whole[:n] for n in range(len(whole))]
    # near-miss destinations and the protocols at the mask words' edges (tests/framegen.py filter_edge_frames)
    out += [f for _, f in frame_plan_subset(600)]
    return out


@pytest.fixture(scope="module")
def input_file(frames, tmp_path_factory):
    path = tmp_path_factory.mktemp("frame_plan") / "input.bin"
    with open(path, "wb") as f:
        f.write(struct.pack("<I", len(FILTERS)))
        for kw in FILTERS:
            c = L.RxFilter() if kw is None else L.RxFilter.make(mac=G.MAC_US, **kw)
            f.write(bytes([kw is not None]) + bytes(c))
        f.write(struct.pack("<I", len(frames)))
        for fr in frames:
            f.write(struct.pack("<I", len(fr)) + fr)
    return path


def _build(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plain_output(input_file, tmp_path_factory):
    r = subprocess.run([str(_build(tmp_path_factory, "frame_plan_host", "-O2")), str(input_file)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_host_parse_matches_the_oracle(frames, plain_output):
    lines = plain_output.splitlines()
    assert len(lines) == len(frames)
    ofilts = [None if kw is None else O.StackFilter(mac=G.MAC_US, **kw) for kw in FILTERS]
    codes = set()
    for i, (fr, line) in enumerate(zip(frames, lines)):
        idx, rx = line.split(" ")
        assert int(idx) == i
        want_rx = "".join(f"{O.ingress_verdict(fr, fl, of):02x}" * 2 for of in ofilts for fl in FLAGS)
        assert rx == want_rx, (i, fr.hex())
        codes.update(int(want_rx[k:k + 2], 16) for k in range(0, len(want_rx), 2))
    assert codes >= {0, O.ERR_PACKET_DROP, O.ERR_BAD_CRC, O.ERR_INVALID_FIELD, O.ERR_INVALID_LENGTH_FIELD,
                     O.ERR_TRUNCATED_FRAME}


def test_host_parse_under_sanitizers(input_file, plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan: no accessor leaves the
    frame's exact-size buffer, and the output is the unsanitized build's."""
    exe = _build(tmp_path_factory, "frame_plan_host_san", "-O1", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    r = subprocess.run([str(exe), str(input_file)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == plain_output

