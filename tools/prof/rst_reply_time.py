"""RST replies against the receive call on the same batch,
HIP-event timed on the launch stream: 3 warm-ups, then 20 calls between two
events, the four calls alternated over --rounds windows in one process and on
one library build; medians, with the spread of the receive call's own windows
beside them.

  count      lnx_rx_rst_reply_batch with cap = 0: the count and scan launches alone
  reply      the whole call, cap = n (count, scan, build)
  receive    lnx_rx_verify_deliver_batch with grouping on the same batch, whose records the two above consume
  tx_finish  lnx_tx_finish_batch(LNX_TX_CHECKSUM | LNX_TX_FCS) over as many prebuilt 54-byte frames as there are
             replies, at capacity 64: what the library could do for these frames once a host had built the
             headers.  It patches lengths in place, so every call is preceded by a device copy of the 54s
             (4 bytes a frame), inside the timed window.

  syn64   1 Mi SYNs of 64 bytes on the wire, all to closed ports
  mtu8    1 Mi frames of 1500 bytes on the wire, one SYN to a closed port in eight

Frames: IPv4, 64 templates.  The buffers are allocated once; the C entries are
called directly.  One shape per process; one JSON line per shape (--out appends
it to a file), the first replies checked against lnx_rx_rst_entry /
lnx_tcp_rst_frame first.  The traffic model beside the times: 16 B of record a
frame and the one or two 128-byte header lines of each queueing frame in, 64 B
+ 4 B a reply out.  Not part of the product."""
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
from tests import deliver_ref as R  # noqa: E402
from tests import framegen as G  # noqa: E402
from tests import reply_ref as P  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, REPS = 3, 20
FILT = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
PORTS = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)
CFG = L.RstCfg.make(mac=P.MAC, gw_mac=P.GW_MAC, ip4=P.IP4, fcs=True)


def fcs(f: bytes) -> bytes:
    return f + struct.pack("<I", L.crc32(f))


def template(shape: str, k: int) -> bytes:
    if shape == "syn64":
        return fcs(P.syn_frame(0x10000000 * (k % 16) + 977 * k, sport=10000 + k, dport=9, payload=bytes(6)))
    closed = k % 8 == 7
    if k & 1:
        l4 = R.tcp_seg(10000 + k, 9 if closed else R.TCP_FULL[(37 * k) & 255], 0x002 if closed else 0x018,
                       bytes((k + i) & 255 for i in range(1500 - 4 - 54)))
        return fcs(G.ether(0x0800, G.ipv4(6, l4)))
    l4 = R.udp_dgram(10000 + k, R.UDP_FULL[(91 * k) & 255], bytes((k + i) & 255 for i in range(1500 - 4 - 42)))
    return fcs(G.ether(0x0800, G.ipv4(17, l4)))


def timeit(fn):
    for _ in range(WARMUP):
        fn()
    torch.cuda.synchronize()
    s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(REPS):
        fn()
    e.record()
    torch.cuda.synchronize()
    return s.elapsed_time(e) / REPS


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["syn64", "mtu8"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    n = max(int((1 << 20) * a.scale) // 64 * 64, 64)
    wl = 64 if a.shape == "syn64" else 1500
    bank = np.stack([np.frombuffer(template(a.shape, k), dtype=np.uint8) for k in range(64)])
    assert bank.shape == (64, wl)
    d = torch.from_numpy(bank).to(dev).repeat(n // 64, 1).reshape(-1).contiguous()
    d_off = torch.arange(n + 1, dtype=torch.int64, device=dev) * wl
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    v = torch.empty(n, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(R.H_COUNT + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.rx_deliver_ws_bytes(n), dtype=torch.uint8, device=dev)
    ids = np.array(L.ip4_id_chain(P.IP4[0], 0x0BAD, n), dtype=np.uint16)
    d_ids = torch.from_numpy(ids.view(np.int16)).to(dev)
    reply = torch.empty((n, 64), dtype=torch.uint8, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    d_n = torch.empty(2, dtype=torch.int32, device=dev)
    rws = torch.empty(L.rx_rst_ws_bytes(n), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pf, pp, pc = ctypes.byref(FILT), ctypes.byref(PORTS), ctypes.byref(CFG)

    def receive():
        assert L.lib.lnx_rx_verify_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, L.VERIFY_ICMP, pf, pp, ok.data_ptr(),
                                                 v.data_ptr(), rec.data_ptr(), order.data_ptr(), count.data_ptr(),
                                                 ws.data_ptr(), s) == 0

    def rst(cap):
        assert L.lib.lnx_rx_rst_reply_batch(d.data_ptr(), d_off.data_ptr(), n, 0, rec.data_ptr(), pc, d_ids.data_ptr(), cap,
                                            reply.data_ptr(), src.data_ptr(), d_n.data_ptr(), rws.data_ptr(), s) == 0

    receive()
    rst(n)
    torch.cuda.synchronize()
    written, wanted = (int(x) for x in d_n.cpu().numpy().view(np.uint32))
    assert written == wanted == (n if a.shape == "syn64" else n // 8), (written, wanted)
    assert int((v.cpu().numpy() != 0).sum()) == 0 and int((ok.cpu().numpy() != 1).sum()) == 0
    # the first replies against the host functions
    h_rec, h_reply, h_src = rec.cpu().numpy(), reply[:64].cpu().numpy(), src[:64].cpu().numpy()
    e, slot, ln = L.TcpRst(), (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    for k in range(min(64, written)):
        i = int(h_src[k])
        f = d[i * wl:(i + 1) * wl - 4].cpu().numpy().tobytes()
        assert L.lib.lnx_rx_rst_entry(f, len(f), h_rec[i].ctypes.data, ctypes.byref(e)) == 1
        assert L.lib.lnx_tcp_rst_frame(pc, ctypes.byref(e), int(ids[k]), slot, ctypes.byref(ln)) == 0
        assert bytes(h_reply[k]) == bytes(slot), k
    # as many bare 54-byte headers as replies, their three generated fields zeroed, 64 bytes apart
    m = written
    bare = reply[:m].clone()
    bare[:, 16:18] = 0
    bare[:, 24:26] = 0
    bare[:, 50:52] = 0
    bare[:, 54:] = 0xAA
    t_start = torch.arange(m, dtype=torch.int64, device=dev) * 64
    t_len0 = torch.full((m,), 54, dtype=torch.int32, device=dev)
    t_len = t_len0.clone()
    t_st = torch.empty(m, dtype=torch.uint8, device=dev)

    def tx_finish():
        t_len.copy_(t_len0)
        assert L.lib.lnx_tx_finish_batch(bare.data_ptr(), t_start.data_ptr(), t_len.data_ptr(), m, 64, 3, t_st.data_ptr(), s) == 0

    tx_finish()
    torch.cuda.synchronize()
    assert torch.equal(bare, reply[:m]) and int(t_st.sum()) == 0 and int((t_len != 64).sum()) == 0

    calls = {"receive": receive, "count": lambda: rst(0), "reply": lambda: rst(n), "tx_finish": tx_finish}
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn))
    receive()
    torch.cuda.synchronize()
    med = {name: float(np.median(x)) for name, x in ms.items()}
    line = {"shape": a.shape, "scale": a.scale, "frames": n, "bytes": n * wl, "replies": written, "warmup": WARMUP,
            "calls": REPS, "windows": a.rounds}
    for name, x in ms.items():
        line[name + "_ms"] = [round(t, 4) for t in x]
    line["median_ms"] = {name: round(t, 4) for name, t in med.items()}
    line["receive_spread_ms"] = round(max(ms["receive"]) - min(ms["receive"]), 4)
    line["build_ms"] = round(med["reply"] - med["count"], 4)
    line["reply_over_receive"] = round(med["reply"] / med["receive"], 4)
    line["reply_over_tx_finish"] = round(med["reply"] / med["tx_finish"], 4)
    line["reply_ns_per_reply"] = round(med["reply"] * 1e6 / max(written, 1), 3)
    # the traffic model: records and header lines in, slots and sources out
    lines_in = 1 if wl % 128 == 0 or wl == 64 else 2
    model = 16 * n + 128 * lines_in * written + 68 * written
    line["model_bytes"] = model
    line["model_gbps"] = round(model / (med["reply"] * 1e-3) / 1e9, 1)
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
