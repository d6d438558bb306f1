"""Running internet checksums against lnx_sum16_batch over the same segments
(DESIGN.md §3.16), HIP-event timed on the launch stream: 3 warm-ups, then 20
launches between two events, the calls of a shape alternated over --rounds
windows in one process; medians, and the spread between sum16_batch's own
windows beside them.

  mtu     1 Mi segments x 1500 B: sum16_batch, sum_partial_batch (the same
          reads, a 4-byte result where the other has 2) and sum16_chain_batch
          with one segment per frame
  jumbo   256 Ki frames x 9000 B as 4 x 2048 + 808-byte segments: sum16_batch
          over the segments against sum16_chain_batch
  giant   one 1 GiB frame as 65 536 x 16 KiB segments: the same pair

One shape per process (python tools/prof/sum_chain_time.py --shape jumbo); one
JSON line per shape, a few results checked against the host functions first.
Under `rocprofv3 --kernel-trace --stats -- python tools/prof/sum_chain_time.py
...` the trace gives the fold kernel's own time.  Not part of the product."""
import argparse
import json
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
import lneto_amd as L  # noqa: E402
from lneto_amd import synth  # noqa: E402

dev = torch.device("cuda:0")
WARMUP, REPS = 3, 20


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
    ap.add_argument("--shape", choices=["jumbo", "mtu", "giant"], required=True)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    a = ap.parse_args()
    if a.shape == "mtu":
        nframes, seg_lens = max(int((1 << 20) * a.scale), 64), [1500]
    elif a.shape == "jumbo":
        nframes, seg_lens = max(int((1 << 18) * a.scale), 16), [2048, 2048, 2048, 2048, 808]
    else:
        nframes, seg_lens = 1, [16384] * max(int(65536 * a.scale), 512)
    per, flen = len(seg_lens), sum(seg_lens)
    nseg = nframes * per
    ln = torch.tensor(seg_lens, dtype=torch.int32, device=dev).repeat(nframes)
    st = torch.cumsum(ln.to(torch.int64), 0) - ln  # back to back: the frame's bytes in order
    first = torch.arange(nframes + 1, dtype=torch.int64, device=dev) * per
    d = synth.bytes_torch(nframes * flen, dev)
    seed = torch.from_numpy(np.random.default_rng(1).integers(0, 2**32, nseg, dtype=np.uint64).astype(np.uint32)
                            .view(np.int32)).to(dev)
    out16 = torch.empty(nseg, dtype=torch.int16, device=dev)
    out32 = torch.empty(nseg, dtype=torch.int32, device=dev)
    f16 = torch.empty(nframes, dtype=torch.int16, device=dev)
    ws = torch.empty(2 * nseg, dtype=torch.int32, device=dev)
    calls = {"sum16_batch": lambda: L.sum16_batch(d, st, ln, seed, out=out16)}
    if a.shape == "mtu":
        calls["sum_partial_batch"] = lambda: L.sum_partial_batch(d, st, ln, d_seed=seed, out=out32)
    calls["sum16_chain_batch"] = lambda: L.sum16_chain_batch(d, st, ln, first, d_seed=seed[:nframes], out16=f16,
                                                             sum32=False, seg_eo=ws)
    for fn in calls.values():
        fn()
    torch.cuda.synchronize()
    sd = seed.cpu().numpy().view(np.uint32)
    for f in ([0] if nframes == 1 else [0, 1, nframes - 1]):
        body = d[f * flen:(f + 1) * flen].cpu().numpy().tobytes()
        assert int(f16[f:f + 1].cpu().numpy().view(np.uint16)[0]) == L.payload_sum16(int(sd[f]), body), f
    for k in (0, nseg - 1):
        body = d[int(st[k]):int(st[k]) + int(ln[k])].cpu().numpy().tobytes()
        assert int(out16[k:k + 1].cpu().numpy().view(np.uint16)[0]) == L.payload_sum16(int(sd[k]), body), k
        if a.shape == "mtu":
            assert int(out32[k:k + 1].cpu().numpy().view(np.uint32)[0]) == L.sum_partial(int(sd[k]), body), k
    ms = {name: [] for name in calls}
    for _ in range(a.rounds):
        for name, fn in calls.items():
            ms[name].append(timeit(fn))
    med = {name: float(np.median(v)) for name, v in ms.items()}
    base = med["sum16_batch"]
    line = {"shape": a.shape, "scale": a.scale, "bytes": nframes * flen, "segments": nseg, "frames": nframes,
            "warmup": WARMUP, "launches": REPS, "windows": a.rounds}
    for name, v in ms.items():
        line[name + "_ms"] = [round(x, 4) for x in v]
    line["median_ms"] = {name: round(v, 4) for name, v in med.items()}
    line["sum16_batch_spread_ms"] = round(max(ms["sum16_batch"]) - min(ms["sum16_batch"]), 4)
    line["extra_ms"] = {name: round(v - base, 4) for name, v in med.items() if name != "sum16_batch"}
    line["ratio"] = {name: round(v / base, 4) for name, v in med.items() if name != "sum16_batch"}
    line["TBps_sum16_batch"] = round(nframes * flen / base / 1e9, 3)
    line["build_id"] = L.build_id()
    line["device"] = torch.cuda.get_device_name(0)
    print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
