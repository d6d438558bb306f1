"""Running-CRC entries against the calls they extend, HIP-event
timed on the launch stream: 3 warm-ups, then 20 launches between two events,
the two calls of a shape alternated over --rounds rounds in one process.

  jumbo   256 Ki frames x 9000 B as 4 x 2048 + 808-byte segments:
          crc32_chain_batch against crc32_segments on the same segments
  mtu     1 Mi frames x 1500 B: crc32_update_batch with random seeds against crc32_batch
  giant   one 1 GiB frame as 65 536 x 16 KiB segments: chain against segments

One shape per process (python tools/prof/chain_time.py --shape jumbo); one JSON
line per shape, a few frames checked against zlib first.  Not part of the product."""
import argparse
import json
import os
import sys
import zlib

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


def u32(t):
    return t.cpu().numpy().view(np.uint32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", choices=["jumbo", "mtu", "giant"], required=True)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--scale", type=float, default=1.0, help="fraction of the shape's frames (rehearsals)")
    a = ap.parse_args()
    if a.shape == "mtu":
        n = max(int((1 << 20) * a.scale), 64)
        d = synth.bytes_torch(n * 1500, dev)
        off = torch.arange(n + 1, dtype=torch.int64, device=dev) * 1500
        seed = torch.from_numpy(np.random.default_rng(1).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32).view(np.int32)).to(dev)
        out = torch.empty(n, dtype=torch.int32, device=dev)
        base_name, new_name = "crc32_batch", "crc32_update_batch"
        base = lambda: L.crc32_batch(d, off, out=out)                 # noqa: E731
        new = lambda: L.crc32_update_batch(d, off, seed, out=out)     # noqa: E731
        new()
        got, raw, sd = u32(out[:4]), d[:6000].cpu().numpy().tobytes(), u32(seed[:4])
        for i in range(4):
            assert got[i] == zlib.crc32(raw[1500 * i:1500 * (i + 1)], int(sd[i])), i
        nbytes = n * 1500
    else:
        if a.shape == "jumbo":
            nframes, seg_lens = max(int((1 << 18) * a.scale), 16), [2048, 2048, 2048, 2048, 808]
        else:
            nframes, seg_lens = 1, [16384] * max(int(65536 * a.scale), 512)
        per = len(seg_lens)
        flen = sum(seg_lens)
        ln = torch.tensor(seg_lens, dtype=torch.int32, device=dev).repeat(nframes)
        st = torch.cumsum(ln.to(torch.int64), 0) - ln  # back to back: the frame's bytes in order
        first = torch.arange(nframes + 1, dtype=torch.int64, device=dev) * per
        d = synth.bytes_torch(nframes * flen, dev)
        ws = torch.empty(nframes * per, dtype=torch.int32, device=dev)
        out = torch.empty(nframes, dtype=torch.int32, device=dev)
        base_name, new_name = "crc32_segments", "crc32_chain_batch"
        base = lambda: L.crc32_segments(d, st, ln, out=ws)                                  # noqa: E731
        new = lambda: L.crc32_chain_batch(d, st, ln, first, out=out, seg_crc=ws)            # noqa: E731
        new()
        for f in ([0] if nframes == 1 else [0, 1, nframes - 1]):
            assert u32(out[f:f + 1])[0] == zlib.crc32(d[f * flen:(f + 1) * flen].cpu().numpy().tobytes()), f
        nbytes = nframes * flen
    base_ms, new_ms = [], []
    for _ in range(a.rounds):
        base_ms.append(timeit(base))
        new_ms.append(timeit(new))
    bm, nm = float(np.median(base_ms)), float(np.median(new_ms))
    print(json.dumps({
        "shape": a.shape, "scale": a.scale, "bytes": nbytes, "warmup": WARMUP, "launches": REPS,
        base_name + "_ms": [round(x, 4) for x in base_ms], new_name + "_ms": [round(x, 4) for x in new_ms],
        "median_ms": [round(bm, 4), round(nm, 4)], "extra_ms": round(nm - bm, 4), "ratio": round(nm / bm, 4),
        "TBps_base": round(nbytes / bm / 1e9, 3), "build_id": L.build_id(),
        "device": torch.cuda.get_device_name(0)}), flush=True)


if __name__ == "__main__":
    main()
