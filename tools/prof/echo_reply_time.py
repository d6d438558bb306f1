"""Echo replies against the receive call on the same batch and against the work
they replace, HIP-event timed on the launch stream: 3
warm-ups, then a window of calls between two events, as many calls as fill about
20 ms (at least 10; the count per call is in the JSON line), the calls
alternated over --rounds windows in one process and on one library build;
medians, with the spread of the receive call's own windows beside them.  On
the zipf8 shape the replies (30 MB) and the records stay in the last-level
cache from call to call, for the call and for its yardsticks alike.

  count      lnx_rx_echo_reply_batch with cap = 0: the count and scan launches alone
  reply      the whole call (count, scan, build; checksums, padding and FCS included)
  reply_nofcs  the same call with a configuration without LNX_TX_FCS: what the copy, the checksums and the padding
             cost without the FCS fold and its tables
  receive    lnx_rx_verify_deliver_batch with grouping on the same batch, whose records the two above consume
  copy       a device-to-device copy of as many bytes as the replies hold
  tx_finish  lnx_tx_finish_batch(LNX_TX_CHECKSUM | LNX_TX_FCS) over the same replies prebuilt without their FCS, in
             the same blocks: what the library could do for these frames once something else had copied the data and
             built the headers.  It patches lengths in place, so every call is preceded by a device copy of the
             lengths (4 bytes a reply), inside the timed window.
  copy + tx_finish is the yardstick "the work it replaces".

  ping1500  1 Mi echo requests of 1500 bytes on the wire: every frame queues
  zipf8     1 Mi frames of Zipf lengths 64-1500 on the wire, one echo request in eight, the rest UDP to open ports

The buffers are allocated once; the C entries are called directly.  One shape
per process; one JSON line per shape (--out appends it to a file), the first
replies checked against lnx_rx_echo_entry / lnx_icmp_echo_reply_frame first.
Not part of the product."""
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
from tests import echo_ref as E  # noqa: E402
from tests import framegen as G  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, MIN_CALLS, WINDOW_MS = 3, 10, 20.0
BANK = 4096   # distinct frames, tiled to the batch
FILT = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
PORTS = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)
CFG = L.RstCfg.make(mac=E.MAC, gw_mac=E.GW_MAC, ip4=E.IP4, fcs=True)
CFG_NOFCS = L.RstCfg.make(mac=E.MAC, gw_mac=E.GW_MAC, ip4=E.IP4, fcs=False)


def fcs(f: bytes) -> bytes:
    return f + struct.pack("<I", L.crc32(f))


def frame(k: int, wire_len: int, request: bool) -> bytes:
    """A frame of wire_len bytes with its FCS (at least 64)."""
    if request:
        return fcs(E.echo_request(E.pattern(wire_len - 4 - 42, k), k & 0xFFFF, (k >> 3) & 0xFFFF))
    l4 = R.udp_dgram(10000 + (k & 0xFFF), R.UDP_FULL[(91 * k) & 255], E.pattern(wire_len - 4 - 42, k))
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
    ap.add_argument("--shape", choices=["ping1500", "zipf8"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    ap.add_argument("--out", help="append the JSON line to this file")
    a = ap.parse_args()
    n = max(int((1 << 20) * a.scale) // BANK * BANK, BANK)
    if a.shape == "ping1500":
        lens = np.full(BANK, 1500, dtype=np.int64)
        bank = [frame(k, 1500, True) for k in range(BANK)]
    else:
        lens = synth.zipf_lengths(BANK).astype(np.int64)
        bank = [frame(k, int(lens[k]), k % 8 == 7) for k in range(BANK)]
    assert [len(f) for f in bank] == lens.tolist()
    flat = np.frombuffer(b"".join(bank), dtype=np.uint8)
    reps = n // BANK
    d = torch.from_numpy(flat.copy()).to(dev).repeat(reps).contiguous()
    h_off = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.tile(lens, reps), out=h_off[1:])
    d_off = torch.from_numpy(h_off).to(dev)
    ok = torch.empty(n, dtype=torch.uint8, device=dev)
    v = torch.empty(n, dtype=torch.uint8, device=dev)
    rec = torch.empty((n, 16), dtype=torch.uint8, device=dev)
    order = torch.empty(n, dtype=torch.int32, device=dev)
    count = torch.empty(R.H_COUNT + 1, dtype=torch.int32, device=dev)
    ws = torch.empty(L.rx_deliver_ws_bytes(n), dtype=torch.uint8, device=dev)
    ids = np.array(L.ip4_id_chain(E.IP4[0], 0x0BAD, n), dtype=np.uint16)
    d_ids = torch.from_numpy(ids.view(np.int16)).to(dev)
    cap_blocks = int(h_off[-1]) // 64 + 2 * n
    reply = torch.empty((cap_blocks, 64), dtype=torch.uint8, device=dev)
    start = torch.empty(n, dtype=torch.int64, device=dev)
    length = torch.empty(n, dtype=torch.int32, device=dev)
    src = torch.empty(n, dtype=torch.int32, device=dev)
    d_n = torch.empty(4, dtype=torch.int32, device=dev)
    ews = torch.empty(L.rx_echo_ws_bytes(n), dtype=torch.uint8, device=dev)
    s = torch.cuda.current_stream(dev).cuda_stream
    pf, pp, pc = ctypes.byref(FILT), ctypes.byref(PORTS), ctypes.byref(CFG)

    def receive():
        assert L.lib.lnx_rx_verify_deliver_batch(d.data_ptr(), d_off.data_ptr(), n, L.VERIFY_ICMP, pf, pp, ok.data_ptr(),
                                                 v.data_ptr(), rec.data_ptr(), order.data_ptr(), count.data_ptr(),
                                                 ws.data_ptr(), s) == 0

    def echo(cap, pc=pc):
        assert L.lib.lnx_rx_echo_reply_batch(d.data_ptr(), d_off.data_ptr(), n, 0, rec.data_ptr(), pc, d_ids.data_ptr(), cap,
                                             cap_blocks, reply.data_ptr(), start.data_ptr(), length.data_ptr(), src.data_ptr(),
                                             d_n.data_ptr(), ews.data_ptr(), s) == 0

    receive()
    echo(n)
    torch.cuda.synchronize()
    written, wanted, bwritten, bwanted = (int(x) for x in d_n.cpu().numpy().view(np.uint32))
    assert written == wanted == (n if a.shape == "ping1500" else n // 8) and bwritten == bwanted, (written, wanted)
    assert int((v.cpu().numpy() != 0).sum()) == 0 and int((ok.cpu().numpy() != 1).sum()) == 0
    # the first replies against the host functions
    h_rec, h_src = rec.cpu().numpy(), src[:64].cpu().numpy()
    h_start, h_len = start[:64].cpu().numpy(), length[:64].cpu().numpy()
    e, ln = L.IcmpEcho(), ctypes.c_uint32(0)
    for k in range(min(64, written)):
        i = int(h_src[k])
        f = d[h_off[i]:h_off[i + 1] - 4].cpu().numpy().tobytes()
        assert L.lib.lnx_rx_echo_entry(f, len(f), h_rec[i].ctypes.data, ctypes.byref(e)) == 1
        buf = (ctypes.c_uint8 * int(h_len[k]))()
        assert L.lib.lnx_icmp_echo_reply_frame(pc, ctypes.byref(e), f[e.data_off:e.data_off + e.data_len], int(ids[k]), buf,
                                               int(h_len[k]), ctypes.byref(ln)) == 0
        got = reply.view(-1)[int(h_start[k]):int(h_start[k]) + int(h_len[k])].cpu().numpy().tobytes()
        assert got == bytes(buf), k
    reply_bytes = int(length[:written].sum())

    # the yardstick: a copy of as many bytes, and tx_finish over the replies without their FCS in the same blocks
    m = written
    flat_reply = reply.view(-1)[:bwritten * 64]
    pre = flat_reply.clone()
    t_start = start[:m].clone()
    t_len0 = (length[:m] - 4).contiguous()
    t_len = t_len0.clone()
    t_st = torch.empty(m, dtype=torch.uint8, device=dev)
    capacity = int(((length[:m].max() + 63) // 64) * 64)
    cp_src = torch.empty(reply_bytes, dtype=torch.uint8, device=dev)
    cp_dst = torch.empty(reply_bytes, dtype=torch.uint8, device=dev)

    def copy():
        cp_dst.copy_(cp_src)

    def tx_finish():
        t_len.copy_(t_len0)
        assert L.lib.lnx_tx_finish_batch(pre.data_ptr(), t_start.data_ptr(), t_len.data_ptr(), m, capacity, 3, t_st.data_ptr(), s) == 0

    tx_finish()
    torch.cuda.synchronize()
    tx_same = bool(torch.equal(pre, flat_reply)) and int(t_st.sum()) == 0 and bool(torch.equal(t_len, length[:m]))

    pc0 = ctypes.byref(CFG_NOFCS)
    calls = {"receive": receive, "count": lambda: echo(0), "reply": lambda: echo(n), "reply_nofcs": lambda: echo(n, pc0),
             "copy": copy, "tx_finish": tx_finish}
    ms = {name: [] for name in calls}
    per_window = {name: calls_for(fn) for name, fn in calls.items()}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn, per_window[name]))
    receive()
    torch.cuda.synchronize()
    med = {name: float(np.median(x)) for name, x in ms.items()}
    line = {"shape": a.shape, "scale": a.scale, "frames": n, "bytes": int(h_off[-1]), "replies": written,
            "reply_bytes": reply_bytes, "reply_blocks": bwritten, "warmup": WARMUP, "calls": per_window, "windows": a.rounds,
            "tx_finish_reproduces_the_replies": tx_same}
    for name, x in ms.items():
        line[name + "_ms"] = [round(t, 4) for t in x]
    line["median_ms"] = {name: round(t, 4) for name, t in med.items()}
    line["receive_spread_ms"] = round(max(ms["receive"]) - min(ms["receive"]), 4)
    line["build_ms"] = round(med["reply"] - med["count"], 4)
    line["replaced_ms"] = round(med["copy"] + med["tx_finish"], 4)
    line["reply_over_receive"] = round(med["reply"] / med["receive"], 4)
    line["reply_over_replaced"] = round(med["reply"] / (med["copy"] + med["tx_finish"]), 4)
    # the traffic model: records in; the replies' bytes in, once for a reply of at most 32 blocks (kept in
    # registers) and twice for a longer one (checksum pass, copy pass); their blocks and start / len / src out
    lens_w = length[:written].to(torch.int64)
    twice = int(lens_w[(lens_w + 63) // 64 > 32].sum())
    model = 16 * n + reply_bytes + twice + 64 * bwritten + 16 * written
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
