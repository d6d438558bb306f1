"""The fused receive check + delivery (lnx_rx_verify_deliver_batch, DESIGN.md
§3.18) against the two calls it replaces, HIP-event timed on the launch stream:
3 warm-ups, then 20 calls between two events, the calls alternated over --rounds
windows in one process; medians, with the spread of the two-call form's own
windows beside them.

  two_calls      lnx_rx_verify_batch, then lnx_rx_deliver_batch with d_order / d_count,
                 both from --parent: the library of the commit before the fused kernel
  fused          lnx_rx_verify_deliver_batch with d_order / d_count, 256-entry port tables
  fused_records  the same without grouping (one launch)
  fused_ports4   the grouped call with 4-entry port tables (the lookup's cost: most ports then miss)
  verify_parent  lnx_rx_verify_batch of --parent
  verify_head    lnx_rx_verify_batch of this build: the same kernel source through the shared
                 body (the A/B of DESIGN.md §3.18 "the eight instantiations")

  mtu    1 Mi valid TCP / UDP frames of 1500 bytes on the wire
  zipf   1 Mi valid TCP / UDP frames, lengths the Zipf 64-1500 B mix (synth.zipf_lengths)
  ring   the zipf frames in a ring's pinned slots (1536 B each), host clock:
         lnx_ingress_packets_deliver against lnx_ingress_packets on the slot buffers, GiB/s

The frames are tools/prof/deliver_time.py's.  The fused call's five outputs are
compared with the two-call form's before anything is timed.  One shape per
process; one JSON line per shape (--out appends it to a file).  Not part of the
product."""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import lneto_amd as L  # noqa: E402
from lneto_amd import synth  # noqa: E402
from tests import deliver_ref as R  # noqa: E402
from deliver_time import FILT, PORTS, REPS, WARMUP, template, timeit  # noqa: E402

dev = torch.device("cuda:0")
PORTS4 = L.RxPorts.make(tcp=R.TCP_FULL[:4], udp=R.UDP_FULL[:4])
_vp = ctypes.c_void_p


def parent_lib(path):
    """The parent commit's library beside this build's, with the two entries the comparison needs."""
    lib = ctypes.CDLL(os.path.abspath(path))
    lib.lnx_rx_verify_batch.restype = ctypes.c_int
    lib.lnx_rx_verify_batch.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(L.RxFilter), _vp, _vp, _vp]
    lib.lnx_rx_deliver_batch.restype = ctypes.c_int
    lib.lnx_rx_deliver_batch.argtypes = [_vp, _vp, ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(L.RxFilter),
                                         ctypes.POINTER(L.RxPorts), _vp, _vp, _vp, _vp, _vp, _vp, _vp]
    assert not hasattr(lib, "lnx_rx_verify_deliver_batch"), "--parent must be the library before the fused kernel"
    return lib


def frames(shape, n):
    lens = np.full(n, 1500, dtype=np.int64) if shape == "mtu" else synth.zipf_lengths(n).astype(np.int64)
    tlen = [1500] * 64 if shape == "mtu" else list(range(64, 1501))
    bank = np.zeros((len(tlen), 1504), dtype=np.uint8)
    for k, wl in enumerate(tlen):
        bank[k, :wl] = np.frombuffer(template(wl, k), dtype=np.uint8)
    tid = (np.arange(n) % 64) if shape == "mtu" else (lens - 64)
    return lens, bank, tid


def emit(line, out):
    line["build_id"] = L.build_id()
    line["device"] = torch.cuda.get_device_name(0)
    text = json.dumps(line)
    print(text, flush=True)
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, "a") as fh:
            fh.write(text + "\n")


def batch(a, P):
    n = max(int((1 << 20) * a.scale), 64)
    lens, bank, tid = frames(a.shape, n)
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
    u8 = lambda m: torch.empty(m, dtype=torch.uint8, device=dev)  # noqa: E731
    i32 = lambda m: torch.empty(m, dtype=torch.int32, device=dev)  # noqa: E731
    two = dict(ok=u8(n), v=u8(n), rec=u8(16 * n), order=i32(n), count=i32(R.H_COUNT + 1))
    one = dict(ok=u8(n), v=u8(n), rec=u8(16 * n), order=i32(n), count=i32(R.H_COUNT + 1))
    ws = u8(L.rx_deliver_ws_bytes(n))
    s = torch.cuda.current_stream(dev).cuda_stream
    pf = ctypes.byref(FILT)

    def verify(lib, o):
        assert lib.lnx_rx_verify_batch(d.data_ptr(), d_off.data_ptr(), n, 0, pf, o["ok"].data_ptr(), o["v"].data_ptr(), s) == 0

    def two_calls():
        verify(P, two)
        assert P.lnx_rx_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, 0, pf, ctypes.byref(PORTS), two["ok"].data_ptr(),
                                      two["v"].data_ptr(), two["rec"].data_ptr(), two["order"].data_ptr(),
                                      two["count"].data_ptr(), ws.data_ptr(), s) == 0

    def fused(ports, group):
        assert L.lib.lnx_rx_verify_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, 0, pf, ctypes.byref(ports),
                                                 one["ok"].data_ptr(), one["v"].data_ptr(), one["rec"].data_ptr(),
                                                 one["order"].data_ptr() if group else None,
                                                 one["count"].data_ptr() if group else None,
                                                 ws.data_ptr() if group else None, s) == 0

    calls = {"two_calls": two_calls, "fused": lambda: fused(PORTS, True), "fused_records": lambda: fused(PORTS, False),
             "fused_ports4": lambda: fused(PORTS4, True), "verify_parent": lambda: verify(P, two),
             "verify_head": lambda: verify(L.lib, one)}
    two_calls()
    fused(PORTS, True)
    torch.cuda.synchronize()
    for k in two:
        assert torch.equal(two[k], one[k]), k
    h_rec = one["rec"].cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    assert int((one["ok"] == 0).sum()) == len(flip) and int((h_rec["verdict"] == 0).sum()) > n // 2
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn))
    med = {name: float(np.median(x)) for name, x in ms.items()}
    spread = lambda name: round(max(ms[name]) - min(ms[name]), 4)  # noqa: E731
    line = {"shape": a.shape, "scale": a.scale, "frames": n, "bytes": int(off[-1]), "warmup": WARMUP, "calls": REPS,
            "windows": a.rounds, "delivered": int((h_rec["verdict"] == 0).sum())}
    for name, x in ms.items():
        line[name + "_ms"] = [round(t, 4) for t in x]
    line["median_ms"] = {name: round(t, 4) for name, t in med.items()}
    line["two_calls_spread_ms"] = spread("two_calls")
    line["fused_gain_ms"] = round(med["two_calls"] - med["fused"], 4)
    line["fused_over_two_calls"] = round(med["fused"] / med["two_calls"], 4)
    line["gain_exceeds_spread"] = bool(med["two_calls"] - med["fused"] > max(ms["two_calls"]) - min(ms["two_calls"]))
    line["lookup_256_minus_4_ms"] = round(med["fused"] - med["fused_ports4"], 4)
    line["verify_parent_spread_ms"] = spread("verify_parent")
    line["verify_head_minus_parent_ms"] = round(med["verify_head"] - med["verify_parent"], 4)
    line["parent_build_id"] = L.build_id(os.path.abspath(a.parent))
    emit(line, a.out)


def ring(a):
    n, cap = max(int((1 << 20) * a.scale), 64), 1536
    lens, bank, tid = frames("zipf", n)
    r = L.RxRing(n, slot_cap=cap, batch_slots=min(65536, n), depth=3, host_threshold=0)
    try:
        r.set_ports(PORTS)
        r.set_filter(FILT)
        for a0 in range(0, n, 65536):
            r.slots[a0:a0 + 65536, :1504] = bank[tid[a0:a0 + 65536]]
        r.slots[np.arange(0, n, 11), lens[::11] - 1] ^= 0x40
        ptrs = (r.slots.ctypes.data + cap * np.arange(n, dtype=np.uint64)).astype(np.uint64)
        ln = lens.astype(np.uint32)
        ok, v = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        ok2, v2 = np.zeros(n, np.uint8), np.zeros(n, np.uint8)
        rec = np.zeros(n, dtype=L.DELIVERY_DTYPE)
        order, count = np.zeros(n, np.uint32), np.zeros(R.H_COUNT + 1, np.uint32)

        def plain():
            assert L.lib.lnx_ingress_packets(r._h, ptrs.ctypes.data, ln.ctypes.data, n, 0, 0, ok.ctypes.data, v.ctypes.data) == 0

        def deliver(group):
            assert L.lib.lnx_ingress_packets_deliver(r._h, ptrs.ctypes.data, ln.ctypes.data, n, 0, 0, ok2.ctypes.data,
                                                     v2.ctypes.data, rec.ctypes.data, order.ctypes.data if group else None,
                                                     count.ctypes.data if group else None) == 0

        calls = {"ingress_packets": plain, "deliver_records": lambda: deliver(False), "deliver_grouped": lambda: deliver(True)}
        z0 = r.stats()["zero_copy_frames"]
        for fn in calls.values():
            fn()
        assert r.stats()["zero_copy_frames"] - z0 == 3 * n, "the slot buffers were not read in place"
        assert np.array_equal(ok, ok2) and np.array_equal(v, v2) and int((ok == 0).sum()) == len(range(0, n, 11))
        key = np.where(rec["handler"] == R.H_NONE, R.H_COUNT, rec["handler"]).astype(np.int64)
        assert np.array_equal(count, np.bincount(key, minlength=R.H_COUNT + 1))
        assert np.array_equal(order, np.argsort(key, kind="stable"))
        sec = {name: [] for name in calls}
        for _ in range(a.rounds):
            for name, fn in calls.items():
                fn()
                t0 = time.perf_counter()
                for _ in range(3):
                    fn()
                sec[name].append((time.perf_counter() - t0) / 3)
    finally:
        r.close()
    nbytes = int(lens.sum())
    gib = {name: [round(nbytes / t / 2**30, 2) for t in x] for name, x in sec.items()}
    line = {"shape": "ring", "scale": a.scale, "frames": n, "bytes": nbytes, "slot_cap": cap, "windows": a.rounds,
            "calls": 3, "clock": "host", "delivered": int((rec["verdict"] == 0).sum())}
    for name, x in gib.items():
        line[name + "_gibs"] = x
    line["median_gibs"] = {name: float(np.median(x)) for name, x in gib.items()}
    line["median_ms"] = {name: round(float(np.median(x)) * 1e3, 3) for name, x in sec.items()}
    line["ingress_packets_spread_gibs"] = round(max(gib["ingress_packets"]) - min(gib["ingress_packets"]), 2)
    emit(line, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["mtu", "zipf", "ring"], required=True)
    ap.add_argument("--parent", help="the parent commit's liblneto_amd.so (mtu, zipf)")
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    if a.shape == "ring":
        return ring(a)
    if not a.parent:
        ap.error("--parent is required for mtu and zipf")
    batch(a, parent_lib(a.parent))


if __name__ == "__main__":
    main()
