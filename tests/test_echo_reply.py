"""Echo replies for ICMPv4 echo requests on the host (no GPU): lnx_rx_echo_entry
and lnx_icmp_echo_reply_frame against the line-cited restatement of
tests/echo_ref.py, every reply through the library's own receive checks, the
shared header under sanitizers, and the batch entry's argument checks."""
import ctypes
import os
import struct
import subprocess

import numpy as np
import pytest

import lneto_amd as L
from oracle import oracle as O
from tests import echo_ref as E
from tests import reply_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "echo_plan_host.cpp")
CFG = {fcs: L.RstCfg.make(mac=E.MAC, gw_mac=E.GW_MAC, ip4=E.IP4, fcs=fcs) for fcs in (False, True)}


def record_bytes(rec):
    return np.array([tuple(rec[k] for k in ("ip_end", "handler", "l4_off", "src_port", "dst_port", "verdict", "flags",
                                            "zero"))], dtype=L.DELIVERY_DTYPE).tobytes()


def ip_id_of(k):
    return (0x9E37 * (k + 1)) & 0xFFFF


@pytest.fixture(scope="module")
def cases():
    """(label, frame, record) of the census under the stack's setting, then the self-made edges."""
    census, _, _ = R.census_cases(E.CENSUS_SETTING)
    return [("census", f, rec) for f, rec in census] + E.self_made_cases()


@pytest.fixture(scope="module")
def replies(cases):
    """(label, frame, entry, data, k) of every case that queues, by the restatement."""
    out = []
    for k, (label, f, rec) in enumerate(cases):
        e = E.echo_entry(f, rec)
        if e is not None:
            out.append((label, f, e, f[e["data_off"]:e["data_off"] + e["data_len"]], k))
    return out


def test_entries_equal_the_restatement(cases):
    queued = {}
    for label, f, rec in cases:
        want = E.echo_entry(f, rec)
        assert L.rx_echo_entry(f, rec) == want, label
        assert L.rx_echo_entry(f, record_bytes(rec)) == want, label
        queued[label] = queued.get(label, 0) + (want is not None)
    assert queued["census"] >= 8                      # echo requests of the census, options among them
    for label in [f"ihl{i}" for i in range(5, 16)] + [f"data{d}" for d in E.EDGE_LENGTHS + (E.MAX_DATA,)] + \
            ["all_zero", "all_zero_odd", "code7", "one_byte_of_data", "end_is_len", "trailer", "data_at_total_length"]:
        assert queued[label] == 1, label
    for label in ("type0", "type3", "no_data", "truncated_icmp", "end_past_len", "l4_33", "l4_far", "nibble6_forced",
                  "handler_igmp", "verdict2", "len0", "data_past_total_length"):
        assert queued[label] == 0, label


def test_census_requests_are_what_the_verdict_let_through(cases):
    """Under VERIFY_ICMP a census frame queues iff it is an IPv4 echo request with data that the receive check
    accepted: handler H_IP4 + 1 holds echo replies and other types too, and those queue nothing."""
    seen = set()
    for label, f, rec in cases:
        if label != "census" or rec["handler"] != E.H_ICMP4 or rec["verdict"] != 0:
            continue
        typ = f[rec["l4_off"]]
        seen.add(typ)
        has_data = rec["ip_end"] > rec["l4_off"] + 8
        assert (L.rx_echo_entry(f, rec) is not None) == (typ == 8 and has_data)
    assert {0, 8} <= seen


def test_frames_equal_the_restatement(replies):
    for label, f, e, data, k in replies:
        for fcs in (False, True):
            want = E.echo_frame(E.MAC, E.GW_MAC, E.IP4, fcs, e, data, ip_id_of(k))
            got = L.icmp_echo_reply_frame(CFG[fcs], e, data, ip_id_of(k))
            assert got == want, (label, fcs)
            assert len(got) == max(60, 42 + len(data)) + (4 if fcs else 0)
    by = {label: (e, data, k) for label, _, e, data, k in replies}
    e, data, k = by["all_zero"]
    assert L.icmp_echo_reply_frame(CFG[False], e, data, 1)[36:38] == b"\xff\xff"   # not RFC 1624's 0x0000
    e, data, k = by["code7"]
    assert L.icmp_echo_reply_frame(CFG[False], e, data, 1)[34:36] == b"\0\0"       # type 0, the request's code dropped
    e, data, k = by[f"data{E.MAX_DATA}"]
    big = L.icmp_echo_reply_frame(CFG[True], e, data, 1)
    assert big[16:18] == b"\xff\xff" and len(big) == 14 + 65535 + 4
    assert {len(L.icmp_echo_reply_frame(CFG[True], by[f"data{d}"][0], by[f"data{d}"][1], 1)) for d in (17, 18, 19)} == {64, 65}


def test_replies_pass_the_library_checks(replies):
    """Under the peer's filter the receive verdict of every reply is 0 (ICMP and evil-bit checks on), pcap's
    checksum re-verification is clean, the FCS residue holds, and a reply fed back as a request queues nothing."""
    peer = L.RxFilter.make(mac=E.GW_MAC)
    for label, f, e, data, k in replies:
        out = L.icmp_echo_reply_frame(CFG[True], e, data, ip_id_of(k))
        bare = out[:-4]
        assert L.lib.lnx_ingress_verdict(bare, len(bare), L.VERIFY_EVIL_BIT | L.VERIFY_ICMP, ctypes.byref(peer)) == 0, label
        assert L.pcap_checksums(bare) == 0, label
        assert L.crc32(out) == L.CRC32_RESIDUE, label
        assert out[26:30] == E.IP4 and out[30:34] == e["remote_addr"] and out[:6] == E.GW_MAC and out[6:12] == E.MAC
        rec = E.record_of(bare)
        assert L.rx_echo_entry(bare, rec) is None and E.echo_entry(bare, rec) is None, label


def test_short_buffer_and_argument_errors():
    f = E.echo_request(E.pattern(30))
    e = L.IcmpEcho.make(**L.rx_echo_entry(f, E.record_of(f)))
    data = f[42:]
    for fcs, need in ((False, 72), (True, 76)):
        out = (ctypes.c_uint8 * 80)(*([0xAA] * 80))
        n = ctypes.c_uint32(77)
        rc = L.lib.lnx_icmp_echo_reply_frame(ctypes.byref(CFG[fcs]), ctypes.byref(e), data, 5, out, need - 1, ctypes.byref(n))
        assert rc == 6 and bytes(out) == b"\xaa" * 80 and n.value == 77          # ErrShortBuffer, nothing written
        rc = L.lib.lnx_icmp_echo_reply_frame(ctypes.byref(CFG[fcs]), ctypes.byref(e), data, 5, out, need, ctypes.byref(n))
        assert rc == 0 and n.value == need and bytes(out[need:]) == b"\xaa" * (80 - need)   # exactly *len bytes
        with pytest.raises(L.LnetoError):
            L.icmp_echo_reply_frame(CFG[fcs], e, data, 5, out_cap=need - 1)
    out, n = (ctypes.c_uint8 * 80)(), ctypes.c_uint32(0)
    frame_of = L.lib.lnx_icmp_echo_reply_frame
    cfg = ctypes.byref(CFG[True])
    assert frame_of(None, ctypes.byref(e), data, 1, out, 80, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, None, data, 1, out, 80, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, ctypes.byref(e), None, 1, out, 80, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, ctypes.byref(e), data, 1, None, 80, ctypes.byref(n)) == L.LNX_EINVAL
    assert frame_of(cfg, ctypes.byref(e), data, 1, out, 80, None) == L.LNX_EINVAL
    bad = L.RstCfg.make(mac=E.MAC, gw_mac=E.GW_MAC, ip4=E.IP4)
    bad.flags = 3   # LNX_TX_CHECKSUM is not a flag of this entry
    assert frame_of(ctypes.byref(bad), ctypes.byref(e), data, 1, out, 80, ctypes.byref(n)) == L.LNX_EINVAL
    for d in (0, E.MAX_DATA + 1):
        e2 = L.IcmpEcho.make(bytes(4), 1, 1, 42, d)
        assert frame_of(cfg, ctypes.byref(e2), data, 1, out, 80, ctypes.byref(n)) == L.LNX_EINVAL

    rec = bytes(16)
    assert L.lib.lnx_rx_echo_entry(f, len(f), None, ctypes.byref(e)) == L.LNX_EINVAL
    assert L.lib.lnx_rx_echo_entry(f, len(f), rec, None) == L.LNX_EINVAL
    assert L.lib.lnx_rx_echo_entry(None, 60, rec, ctypes.byref(e)) == L.LNX_EINVAL
    assert L.lib.lnx_rx_echo_entry(None, 0, record_bytes(E.record_of(f)), ctypes.byref(e)) == 0

    # the batch entry: pointers that are never followed (the checks come before any device call)
    p, badcfg = 0x1000, ctypes.byref(bad)
    batch = L.lib.lnx_rx_echo_reply_batch
    assert batch(p, p, 1 << 32, 0, p, cfg, p, 4, 4, p, p, p, p, p, p, None) == L.LNX_EINVAL
    assert batch(p, p, 4, 8, p, cfg, p, 4, 4, p, p, p, p, p, p, None) == L.LNX_EINVAL                 # an unknown flag
    assert batch(p, p, 4, L.VERIFY_ICMP, p, cfg, p, 4, 4, p, p, p, p, p, p, None) == L.LNX_EINVAL     # a receive-check flag
    assert batch(p, p, 4, 0, p, badcfg, p, 4, 4, p, p, p, p, p, p, None) == L.LNX_EINVAL              # ... on the other word
    assert batch(p, p, 4, 0, p, cfg, p, 4, 4, p + 32, p, p, p, p, p, None) == L.LNX_EINVAL            # d_reply: 64-byte aligned
    for hole in range(11):   # a NULL pointer with work to do
        a = [p, p, p, cfg, p, p, p, p, p, p, p]
        a[hole] = None
        assert batch(a[0], a[1], 4, 0, a[2], a[3], a[4], 4, 4, a[5], a[6], a[7], a[8], a[9], a[10], None) == L.LNX_EINVAL, hole
    none = [None] * 6
    assert batch(None, None, 0, 0, None, None, None, 0, 0, *none, None) == L.LNX_OK   # nothing to do
    assert batch(None, None, 0, 0, None, None, None, 4, 4, *none, None) == L.LNX_OK
    assert batch(None, None, 0, 8, None, None, None, 0, 0, *none, None) == L.LNX_EINVAL
    assert batch(None, None, 4, 0, None, None, None, 0, 0, *none, None) == L.LNX_EINVAL   # cap 0 still counts


def test_workspace_size():
    """A qword and a word per workgroup of the count / build launches (at most 1024), and one more of each: the totals."""
    assert L.rx_echo_ws_bytes(0) == 24 and L.rx_echo_ws_bytes(256) == 24 and L.rx_echo_ws_bytes(257) == 36
    assert L.rx_echo_ws_bytes(1 << 20) == 12 * 1025


# ------------------------------------------------------------ the shared header, stand-alone
@pytest.fixture(scope="module")
def program_input(cases, tmp_path_factory):
    path = tmp_path_factory.mktemp("echo_plan") / "input.bin"
    with open(path, "wb") as fh:
        fh.write(struct.pack("<I", 2) + bytes(CFG[False]) + bytes(CFG[True]))
        fh.write(struct.pack("<I", len(cases)))
        for k, (_, f, rec) in enumerate(cases):
            fh.write(struct.pack("<IH", len(f), ip_id_of(k)) + record_bytes(rec) + f)
    return path


def _build(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, SRC, "-o", str(exe)], check=True)
    return exe


@pytest.fixture(scope="module")
def plain_output(program_input, tmp_path_factory):
    r = subprocess.run([str(_build(tmp_path_factory, "echo_plan_host", "-O2")), str(program_input)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-2000:]
    return r.stdout


def test_standalone_program_equals_library(cases, plain_output):
    """g++'s build of echo_plan.hpp + echo_host.cpp gives the library's entries and frames (a CRC-32 of each frame,
    its length and its first 64 bytes stand for it), and refuses a buffer one byte short."""
    lines = plain_output.splitlines()
    assert len(lines) == len(cases)
    queued = 0
    for k, ((label, f, rec), line) in enumerate(zip(cases, lines)):
        e = L.rx_echo_entry(f, rec)
        if e is None:
            assert line == "-", label
            continue
        queued += 1
        want = [bytes(L.IcmpEcho.make(**e)).hex()]
        for fcs in (False, True):
            out = L.icmp_echo_reply_frame(CFG[fcs], e, f[e["data_off"]:e["data_off"] + e["data_len"]], ip_id_of(k))
            want += [out[:64].hex(), f"{O.crc32(out):08x}", str(len(out)), "6"]
        assert line.split() == want, label
    assert queued > 40


def test_standalone_program_under_sanitizers(program_input, plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan, run directly: every frame and every output buffer sits in a
    heap block of exactly its length, so no field read leaves a frame (the cases hold frames that end at the last
    byte the copy reads) and no write leaves *len; the output is the plain build's."""
    exe = _build(tmp_path_factory, "echo_plan_host_san", "-O1", "-g", "-fsanitize=address,undefined",
                 "-fno-sanitize-recover=all")
    r = subprocess.run([str(exe), str(program_input)], capture_output=True, text=True)
    assert r.returncode == 0, r.stderr[-4000:]
    assert r.stdout == plain_output
