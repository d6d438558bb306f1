"""ARP replies and learn records against the receive call on the same batch
(DESIGN.md §3.22), HIP-event timed on the launch stream: 3 warm-ups, then as many
calls between two events as fill a window of 20 ms (at least 10; the count per
call is in the JSON line), the four calls alternated over --rounds windows in
one process and on one library build; medians, with the spread of the receive
call's own windows beside them.

  count      lnx_rx_arp_batch with both caps 0: the count and scan launches alone
  arp        the whole call, cap = cap_seen = n (count, scan, build)
  receive    lnx_rx_verify_deliver_batch with grouping on the same batch, whose records the two above consume
  tx_finish  lnx_tx_finish_batch(LNX_TX_FCS) over as many prebuilt 60-byte frames as there are replies, at
             capacity 64: what the library could do for these frames before, once a host had built them.  It
             patches lengths in place, so every call is preceded by a device copy of the 60s (4 bytes a frame),
             inside the timed window.

  sweep   1 Mi ARP requests of 64 bytes on the wire, all for our address
  zipf8   1 Mi frames of Zipf lengths 64-1500 on the wire, one ARP frame in eight (half of them requests for us,
          half replies), the rest UDP to open ports

The buffers are allocated once; the C entries are called directly.  One shape
per process; one JSON line per shape (--out appends it to a file), the first
replies and learn records checked against lnx_rx_arp_entry / lnx_arp_frame
first.  The traffic model beside the times: 16 B of record a frame, 16 B of
offsets and the one or two 64-byte lines that hold bytes 12..41 of each
candidate in, 64 B + 4 B a reply and 16 B a learn record out.  Not part of the
product."""
import argparse
import ctypes
import json
import os
import struct
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
import lneto_amd as L  # noqa: E402
from lneto_amd import synth  # noqa: E402
from tests import arp_ref as A  # noqa: E402
from tests import deliver_ref as R  # noqa: E402
from tests import framegen as G  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, MIN_CALLS, WINDOW_MS = 3, 10, 20.0
BANK = 4096   # distinct frames, tiled to the batch
FILT = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
PORTS = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)
CFG = L.RstCfg.make(mac=A.MAC, gw_mac=A.GW_MAC, ip4=A.IP4, fcs=True)


def fcs(f: bytes) -> bytes:
    return f + struct.pack("<I", L.crc32(f))


def arp(k: int, op: int) -> bytes:
    sha = bytes([0x02, 0x11, 0x22, (k >> 8) & 255, k & 255, 0x5A])
    return fcs(A.arp_eth(A.arp_body(op, sha=sha, spa=bytes([10, 9, (k >> 8) & 255, k & 255]), tha=A.MAC if op == 2 else bytes(6))))


def udp(k: int, wire_len: int) -> bytes:
    l4 = R.udp_dgram(10000 + (k & 0xFFF), R.UDP_FULL[(91 * k) & 255], bytes((k + i) & 255 for i in range(wire_len - 4 - 42)))
    return fcs(G.ether(0x0800, G.ipv4(17, l4)))


def window(fn, calls):
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(calls):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / calls


def calls_for(fn):
    """Warm up, then the number of calls that fills a window of WINDOW_MS."""
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    per = window(fn, MIN_CALLS)
    return int(min(max(MIN_CALLS, WINDOW_MS / max(per, 1e-4)), 5000))


def timeit(fn, calls):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    return window(fn, calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["sweep", "zipf8"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    ap.add_argument("--out", help="append the JSON line to this file")
    ap.add_argument("--dry", action="store_true", help="build the batch and its host expectations, then stop (no device)")
    a = ap.parse_args()
    n = max(int((1 << 20) * a.scale) // BANK * BANK, BANK)
    if a.shape == "sweep":
        bank = [arp(k, 1) for k in range(BANK)]
    else:
        lens = synth.zipf_lengths(BANK).astype(np.int64)
        bank = [arp(k, 1 + ((k >> 3) & 1)) if k % 8 == 7 else udp(k, max(int(lens[k]), 64)) for k in range(BANK)]
    lens = np.array([len(f) for f in bank], dtype=np.int64)
    want_replies = sum(1 for k in range(BANK) if a.shape == "sweep" or (k % 8 == 7 and not (k >> 3) & 1)) * (n // BANK)
    want_seen = (0 if a.shape == "sweep" else BANK // 16) * (n // BANK)
    flat = np.frombuffer(b"".join(bank), dtype=np.uint8)
    reps = n // BANK
    h_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.tile(lens, reps), out=h_off[1:])
    if a.dry:
        print(json.dumps({"shape": a.shape, "frames": n, "bytes": int(h_off[-1]), "replies": want_replies, "seen": want_seen}))
        return
    d = torch.from_numpy(flat.copy()).to(dev).repeat(reps).contiguous()
    d_off = torch.from_numpy(h_off).to(dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    v = torch.empty(n, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(R.H_COUNT + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.rx_deliver_ws_bytes(n), dtype=torch.uint8, device=dev)
    reply = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    seen = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    d_n = torch.empty(4, dtype=torch.int32, device=dev)
    aws = torch.empty(L.rx_arp_ws_bytes(n), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pf, pp, pc = ctypes.byref(FILT), ctypes.byref(PORTS), ctypes.byref(CFG)

    def receive():
        assert L.lib.lnx_rx_verify_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, L.VERIFY_ICMP, pf, pp, ok.data_ptr(),
                                                 v.data_ptr(), rec.data_ptr(), order.data_ptr(), count.data_ptr(),
                                                 ws.data_ptr(), s) == 0

    def arp_call(cap):
        assert L.lib.lnx_rx_arp_batch(d.data_ptr(), d_off.data_ptr(), n, 0, rec.data_ptr(), pc, cap, cap, reply.data_ptr(),
                                      src.data_ptr(), seen.data_ptr(), d_n.data_ptr(), aws.data_ptr(), s) == 0

    receive()
    arp_call(n)
    torch.cuda.synchronize()
    counts = [int(x) for x in d_n.cpu().numpy().view(np.uint32)]
    assert counts == [want_replies, want_replies, want_seen, want_seen], counts
    assert int((v.cpu().numpy() != 0).sum()) == 0 and int((ok.cpu().numpy() != 1).sum()) == 0
    # the first replies and learn records against the host functions
    written, nseen = counts[0], counts[2]
    h_reply, h_src, h_seen = reply[:64].cpu().numpy(), src[:64].cpu().numpy(), seen[:64].cpu().numpy().view(L.ARP_SEEN_DTYPE).reshape(-1)
    e, slot, ln = L.ArpEntry(), (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)

    def host_entry(i):
        f = d[int(h_off[i]):int(h_off[i + 1]) - 4].cpu().numpy().tobytes()
        r = rec[i].cpu().numpy().tobytes()
        return L.lib.lnx_rx_arp_entry(f, len(f), r, pc, ctypes.byref(e), None)

    for k in range(min(64, written)):
        assert host_entry(int(h_src[k])) == 1
        assert L.lib.lnx_arp_frame(pc, 2, ctypes.byref(e), slot, ctypes.byref(ln)) == 0
        assert bytes(h_reply[k]) == bytes(slot), k
    for k in range(min(64, nseen)):
        assert host_entry(int(h_seen["src"][k])) == 2
        assert bytes(h_seen["hw"][k]) == bytes(e.hw) and bytes(h_seen["ip"][k]) == bytes(e.ip), k
    # as many bare 60-byte frames as replies, 64 bytes apart, the FCS room filled with something else
    m = written
    bare = reply[:m].clone()
    bare[:, 60:] = 0xAA
    t_start = torch.arange(m, dtype=torch.int64, device=dev) * 64
    t_len0 = torch.full((m,), 60, dtype=torch.int32, device=dev)
    t_len = t_len0.clone()
    t_st = torch.empty(m, dtype=torch.uint8, device=dev)

    def tx_finish():
        t_len.copy_(t_len0)
        assert L.lib.lnx_tx_finish_batch(bare.data_ptr(), t_start.data_ptr(), t_len.data_ptr(), m, 64, L.TX_FCS, t_st.data_ptr(), s) == 0

    tx_finish()
    torch.cuda.synchronize()
    assert torch.equal(bare, reply[:m]) and int(t_st.sum()) == 0 and int((t_len != 64).sum()) == 0

    calls = {"receive": receive, "count": lambda: arp_call(0), "arp": lambda: arp_call(n), "tx_finish": tx_finish}
    per_window = {name: calls_for(fn) for name, fn in calls.items()}
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn, per_window[name]))
    receive()
    torch.cuda.synchronize()
    med = {name: float(np.median(x)) for name, x in ms.items()}
    line = {"shape": a.shape, "scale": a.scale, "frames": n, "bytes": int(h_off[-1]), "replies": written, "seen": nseen,
            "warmup": WARMUP, "calls": per_window, "windows": a.rounds}
    for name, x in ms.items():
        line[name + "_ms"] = [round(t, 4) for t in x]
    line["median_ms"] = {name: round(t, 4) for name, t in med.items()}
    line["range_ms"] = {name: [round(min(x), 4), round(max(x), 4)] for name, x in ms.items()}
    line["receive_spread_ms"] = round(max(ms["receive"]) - min(ms["receive"]), 4)
    line["build_ms"] = round(med["arp"] - med["count"], 4)
    line["arp_over_receive"] = round(med["arp"] / med["receive"], 4)
    line["arp_over_tx_finish"] = round(med["arp"] / med["tx_finish"], 4)
    line["arp_ns_per_reply"] = round(med["arp"] * 1e6 / max(written, 1), 3)
    # the traffic model: records, offsets and the candidates' lines in (twice: count and build), slots, sources and learn records out
    cand = written + nseen
    model = 2 * (16 * n + 16 * n + 64 * cand) + 68 * written + 16 * nseen
    line["model_bytes"] = model
    line["model_gbps"] = round(model / (med["arp"] * 1e-3) / 1e9, 1)
    line["build_id"] = L.build_id()
    line["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(line)
    print(text, flush=True)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a") as fh:
            fh.write(text + "\n")


if __name__ == "__main__":
    main()
