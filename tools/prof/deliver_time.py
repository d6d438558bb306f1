"""Receive delivery against the receive check on the same batch (DESIGN.md
§3.17), HIP-event timed on the launch stream: 3 warm-ups, then 20 calls between
two events, the three calls alternated over --rounds windows in one process;
medians, with the spread of rx_verify_batch's own windows beside them.

  records   lnx_rx_deliver_batch without grouping (one launch)
  grouped   the same with d_order / d_count (four launches)
  verify    lnx_rx_verify_batch, whose fcs_ok / verdict the two above consume

  mtu    1 Mi valid TCP / UDP frames of 1500 bytes on the wire
  zipf   1 Mi valid TCP / UDP frames, lengths the Zipf 64-1500 B mix (synth.zipf_lengths)

Frames: IPv4, alternately TCP and UDP, one template per length (zipf) or 64
templates (mtu), destination ports spread over full 256-entry tables with one
template in eight to a closed port, every eleventh frame's FCS flipped on the
device.  The buffers are allocated once; the C entry is called directly.  One
shape per process; one JSON line per shape (--out appends it to a file), a
sample of records checked against lnx_rx_deliver first.  Not part of the
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
from tests import deliver_ref as R  # noqa: E402
from tests import framegen as G  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, REPS = 3, 20
FILT = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
PORTS = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)


def template(wire_len: int, k: int) -> bytes:
    """A valid frame of wire_len bytes with its FCS; k picks the protocol and the port."""
    closed = k % 8 == 7
    if k & 1:
        l4 = R.tcp_seg(10000 + k, 9 if closed else R.TCP_FULL[(37 * k) & 255], 0x002 if closed else 0x018,
                       bytes((k + i) & 255 for i in range(wire_len - 4 - 54)))
        f = G.ether(0x0800, G.ipv4(6, l4))
    else:
        l4 = R.udp_dgram(10000 + k, 9 if closed else R.UDP_FULL[(91 * k) & 255], bytes((k + i) & 255 for i in range(wire_len - 4 - 42)))
        f = G.ether(0x0800, G.ipv4(17, l4))
    assert len(f) + 4 == wire_len
    return f + struct.pack("<I", L.crc32(f))


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
    ap.add_argument("--shape", choices=["mtu", "zipf"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    n = max(int((1 << 20) * a.scale), 64)
    if a.shape == "mtu":
        lens = np.full(n, 1500, dtype=np.int64)
        tlen = [1500] * 64
    else:
        lens = synth.zipf_lengths(n).astype(np.int64)
        tlen = list(range(64, 1501))
    bank = np.zeros((len(tlen), 1504), dtype=np.uint8)
    for k, wl in enumerate(tlen):
        bank[k, :wl] = np.frombuffer(template(wl, k), dtype=np.uint8)
    tid = (np.arange(n) % 64) if a.shape == "mtu" else (lens - 64)
    off = synth.offsets_from_lengths(lens).astype(np.int64)
    d_off = torch.from_numpy(off).to(dev)
    d_len, d_tid = torch.from_numpy(lens).to(dev), torch.from_numpy(tid.astype(np.int64)).to(dev)
    if a.shape == "mtu":
        d = torch.from_numpy(bank).to(dev)[d_tid, :1500].reshape(-1).contiguous()
    else:
        fid = torch.repeat_interleave(torch.arange(n, device=dev), d_len)
        pos = torch.arange(int(off[-1]), device=dev) - d_off[fid]
        d = torch.from_numpy(bank).to(dev)[d_tid[fid], pos].contiguous()
        del fid, pos
    flip = torch.arange(0, n, 11, device=dev)
    d[d_off[flip + 1] - 1] ^= 0x40  # the FCS's last byte of every eleventh frame
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    v = torch.empty(n, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(R.H_COUNT + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.rx_deliver_ws_bytes(n), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pf, pp = ctypes.byref(FILT), ctypes.byref(PORTS)

    def verify():
        assert L.lib.lnx_rx_verify_batch(d.data_ptr(), d_off.data_ptr(), n, 0, pf, ok.data_ptr(), v.data_ptr(), s) == 0

    def deliver(group):
        assert L.lib.lnx_rx_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, 0, pf, pp, ok.data_ptr(), v.data_ptr(),
                                          rec.data_ptr(), order.data_ptr() if group else None,
                                          count.data_ptr() if group else None, ws.data_ptr() if group else None, s) == 0

    calls = {"verify": verify, "records": lambda: deliver(False), "grouped": lambda: deliver(True)}
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    # a sample against the host function, and the grouping's invariants
    h_ok, h_v, h_rec = ok.cpu().numpy(), v.cpu().numpy(), rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    assert int((h_ok == 0).sum()) == len(flip) and int((h_v != 0).sum()) == 0
    for i in list(range(0, n, max(n // 500, 1))) + [n - 1]:
        f = d[int(off[i]):int(off[i + 1]) - 4].cpu().numpy().tobytes()
        want = L.rx_deliver(f, int(h_v[i]), FILT, PORTS, int(h_ok[i]))
        assert {k: int(h_rec[i][k]) for k in want} == want, i
    key = np.where(h_rec["handler"] == R.H_NONE, R.H_COUNT, h_rec["handler"]).astype(np.int64)
    assert np.array_equal(count.cpu().numpy(), np.bincount(key, minlength=R.H_COUNT + 1))
    assert np.array_equal(order.cpu().numpy(), np.argsort(key, kind="stable"))
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn))
    med = {name: float(np.median(x)) for name, x in ms.items()}
    line = {"shape": a.shape, "scale": a.scale, "frames": n, "bytes": int(off[-1]), "warmup": WARMUP, "calls": REPS,
            "windows": a.rounds, "delivered": int((h_rec["verdict"] == 0).sum()), "buckets": int(len(set(key.tolist())))}
    for name, x in ms.items():
        line[name + "_ms"] = [round(t, 4) for t in x]
    line["median_ms"] = {name: round(t, 4) for name, t in med.items()}
    line["verify_spread_ms"] = round(max(ms["verify"]) - min(ms["verify"]), 4)
    line["grouping_ms"] = round(med["grouped"] - med["records"], 4)
    line["grouped_over_verify"] = round(med["grouped"] / med["verify"], 4)
    line["records_ns_per_frame"] = round(med["records"] * 1e6 / n, 3)
    line["grouped_ns_per_frame"] = round(med["grouped"] * 1e6 / n, 3)
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
