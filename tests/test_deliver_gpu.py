"""Receive delivery on the MI355X: lnx_rx_deliver_batch against the per-frame
host function lnx_rx_deliver (itself pinned on the restatement by
tests/test_deliver.py), its order / count against numpy's stable argsort and
bincount of the bucket keys."""
import ctypes
import struct
import threading

import numpy as np
import pytest

import lneto_amd as L
from tests import deliver_ref as R
from tests import framegen as G

pytestmark = pytest.mark.gpu

GRID_CAP, CHUNK = 512, 256   # deliver_kernel.hip: kGrpGridCap workgroups, kGrpBlock frames a chunk
FILT = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
FULL = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)
DUP = L.RxPorts.make(tcp=[7, 80, 80, 443, 0], udp=[53, 53, 0])


def with_fcs(f: bytes, flip: bool = False) -> bytes:
    fcs = L.crc32(f) ^ (0x00010000 if flip else 0)
    return f + struct.pack("<I", fcs)


def packed(frames):
    lens = np.array([len(f) for f in frames], dtype=np.int64)
    off = np.zeros(len(frames) + 1, dtype=np.int64)
    np.cumsum(lens, out=off[1:])
    return np.frombuffer(b"".join(frames) or b"\0", dtype=np.uint8).copy(), off


def host_records(frames, verdict, fcs_ok, filt, ports):
    """lnx_rx_deliver in a loop; frames without their FCS."""
    out = np.zeros(len(frames), dtype=L.DELIVERY_DTYPE)
    pf = ctypes.byref(filt) if filt is not None else None
    pp = ctypes.byref(ports) if ports is not None else None
    base = out.ctypes.data
    for i, f in enumerate(frames):
        rc = L.lib.lnx_rx_deliver(f, len(f), pf, pp, -1 if fcs_ok is None else int(fcs_ok[i]), int(verdict[i]), base + 16 * i)
        assert rc == 0
    return out


def grouping(rec):
    key = np.where(rec["handler"] == R.H_NONE, R.H_COUNT, rec["handler"]).astype(np.int64)
    return np.argsort(key, kind="stable"), np.bincount(key, minlength=R.H_COUNT + 1)


def check(got, want_rec):
    rec, order, count = got
    rec = rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    bad = np.flatnonzero(rec != want_rec)
    assert bad.size == 0, (bad[:5], rec[bad[:5]], want_rec[bad[:5]])
    if order is not None:
        want_order, want_count = grouping(want_rec)
        assert np.array_equal(count.cpu().numpy(), want_count)
        assert np.array_equal(order.cpu().numpy(), want_order)


def dev(cuda, data, off):
    import torch
    return torch.from_numpy(data).to(cuda), torch.from_numpy(off).to(cuda)


@pytest.fixture(scope="module")
def census():
    """The census frames in a fixed shuffle (so that a short prefix is mixed), a third of their FCSs flipped."""
    frames = [f for _, f in R.census_frames()]
    perm = np.random.default_rng(5).permutation(len(frames))
    frames = [frames[i] for i in perm]
    return frames, [with_fcs(f, flip=i % 3 == 1) for i, f in enumerate(frames)]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, None])
def test_chain_behind_the_receive_check(cuda, census, n):
    bare, wire = census
    n = len(bare) if n is None else n
    for flags, frames in ((0, wire[:n]), (L.RX_NO_FCS, bare[:n])):
        d, o = dev(cuda, *packed(frames))
        ok, v = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP | flags, filter=FILT)
        got = L.rx_deliver_batch(d, o, v, ok, flags=flags, filter=FILT, ports=FULL)
        want = host_records(bare[:n], v.cpu().numpy(), ok.cpu().numpy(), FILT, FULL)
        check(got, want)
        if n == len(bare) and flags == 0:
            # the batch is mixed: a third of the FCSs are flipped, and frames are delivered, dropped and queued for RST
            assert ((want["flags"] & R.DLV_FCS) != 0).sum() > n // 4 and (want["verdict"] == 0).sum() > 100
            assert ((want["flags"] & R.DLV_RST) != 0).sum() > 20 and (want["verdict"] == R.ERR_SHORT_BUFFER).sum() > 20
            assert len(set(want["handler"].tolist())) >= 10
            # the other settings on the same batch, and no FCS results at all
            for filt, ports in ((None, None), (None, DUP), (FILT, L.RxPorts.make())):
                v2 = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=filt)[1]
                check(L.rx_deliver_batch(d, o, v2, None, filter=filt, ports=ports),
                      host_records(bare, v2.cpu().numpy(), None, filt, ports))


@pytest.fixture(scope="module")
def short_pool(census):
    """Census frames of 64-128 bytes on the wire, with their host records under FILT / DUP."""
    bare, wire = census
    keep = [i for i, f in enumerate(wire) if 64 <= len(f) <= 128][:509]   # (a prime: no period shared with the chunks)
    assert len(keep) == 509
    b, w = [bare[i] for i in keep], [wire[i] for i in keep]
    fcs_ok = np.array([i % 3 != 1 for i in keep], dtype=np.uint8)
    cf = ctypes.byref(FILT)
    v = np.array([L.lib.lnx_ingress_verdict(f, len(f), L.VERIFY_ICMP, cf) for f in b], dtype=np.uint8)
    return w, v, fcs_ok, host_records(b, v, fcs_ok, FILT, DUP)


@pytest.mark.parametrize("n", [GRID_CAP * CHUNK + 1, 3 * GRID_CAP * CHUNK + 77])
def test_capped_grids_past_one_pass(cuda, short_pool, n):
    """More chunks than workgroups: at cap x chunk + 1 the first 257 workgroups take two chunks (the last of them
    one frame) and the rest none; at 3 x that every workgroup takes four, the last ones fewer."""
    wire, v, fcs_ok, rec = short_pool
    data, off = packed(wire)
    reps = -(-n // len(wire))
    lens = np.tile(np.diff(off), reps)[:n]
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    bdata = np.tile(data, reps)[:boff[-1]]
    assert bdata.nbytes < 64 << 20
    d, o = dev(cuda, bdata, boff)
    ok, vd = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT)
    assert np.array_equal(vd.cpu().numpy(), np.tile(v, reps)[:n]) and np.array_equal(ok.cpu().numpy(), np.tile(fcs_ok, reps)[:n])
    check(L.rx_deliver_batch(d, o, vd, ok, filter=FILT, ports=DUP), np.tile(rec, reps)[:n])


def _plain(cuda, frames, filt, ports, **kw):
    """Valid frames without FCS and a zero verdict for each."""
    import torch
    d, o = dev(cuda, *packed(frames))
    v = torch.zeros(len(frames), dtype=torch.uint8, device=cuda)
    got = L.rx_deliver_batch(d, o, v, None, flags=L.RX_NO_FCS, filter=filt, ports=ports, **kw)
    return got, host_records(frames, np.zeros(len(frames), np.uint8), None, filt, ports)


def test_bucket_extremes(cuda):
    tcp = lambda port, i=0: G.ether(0x0800, G.ipv4(6, R.tcp_seg(30000 + i, port, 0x018, bytes([i & 255]) * (i % 7))))
    udp = lambda port, i=0: G.ether(0x86DD, G.ipv6(17, R.udp_dgram(30000 + i, port, bytes([i & 255]) * (i % 5))))
    # every frame in one bucket
    got, want = _plain(cuda, [tcp(1100, i) for i in range(1000)], FILT, FULL)
    assert set(want["handler"]) == {R.H_TCP + 100}
    check(got, want)
    assert np.array_equal(got[1].cpu().numpy(), np.arange(1000))
    # every frame undelivered
    got, want = _plain(cuda, [tcp(1100, i) if i & 1 else udp(2100, i) for i in range(1000)], FILT, L.RxPorts.make())
    assert set(want["handler"]) == {R.H_NONE} and set(want["verdict"]) == {2}
    check(got, want)
    assert int(got[2][R.H_COUNT]) == 1000 and np.array_equal(got[1].cpu().numpy(), np.arange(1000))
    # 256 TCP + 256 UDP ports, each hit exactly once (in a scrambled arrival order)
    perm = np.random.default_rng(9).permutation(512)
    frames = [tcp(R.TCP_FULL[j], int(j)) if j < 256 else udp(R.UDP_FULL[j - 256], int(j)) for j in perm]
    got, want = _plain(cuda, frames, None, FULL)
    check(got, want)
    count = got[2].cpu().numpy()
    assert (count[R.H_TCP:R.H_TCP + 256] == 1).all() and (count[R.H_UDP:R.H_UDP + 256] == 1).all() and count.sum() == 512
    # two buckets alternating frame by frame: arrival order inside each
    got, want = _plain(cuda, [tcp(1000, i) if i & 1 else udp(2000, i) for i in range(1001)], FILT, FULL)
    check(got, want)
    assert np.array_equal(got[1].cpu().numpy(), np.concatenate([np.arange(1, 1001, 2), np.arange(0, 1001, 2)]))


def test_offsets_in_any_order(cuda, census):
    import torch
    bare, wire = census
    wire = wire[:600]
    data, off = packed(wire)
    d = torch.from_numpy(data).to(cuda)
    rng = np.random.default_rng(11)
    shuffled = off.copy()
    rng.shuffle(shuffled)                      # arbitrary ranges: overlaps, ends below their starts, long frames
    near = off.copy()
    near[1::2] = np.maximum(near[1::2] - 30, 0)  # every other boundary 30 bytes early: frames that start in their neighbour
    for o_np in (off[::-1].copy(), shuffled, near):
        o = torch.from_numpy(o_np).to(cuda)
        ok, v = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT)
        frames = [data[o_np[i]:max(o_np[i + 1] - 4, o_np[i])].tobytes() for i in range(len(o_np) - 1)]
        check(L.rx_deliver_batch(d, o, v, ok, filter=FILT, ports=FULL),
              host_records(frames, v.cpu().numpy(), ok.cpu().numpy(), FILT, FULL))
    assert any(len(f) == 0 for f in frames) and any(len(f) > 0 for f in frames)


def test_verdicts_that_do_not_belong_to_the_bytes(cuda):
    """A zero verdict over truncated frames packed back to back: whatever lies
    next to a frame is another frame's bytes, so a read past a frame's end would
    decide something the host function (which sees the frame alone) does not."""
    import torch
    sweep = [f for _, f in R.truncation_sweep()]
    for flags in (L.RX_NO_FCS, 0):
        frames = sweep if flags else [f + b"\x08\x00\x45\x06" for f in sweep]   # four more bytes in the FCS's place
        data, off = packed(frames)
        buf = np.concatenate([np.full(61, 0xA5, np.uint8), data, np.full(64, 0x5A, np.uint8)])   # (61: odd alignments)
        d = torch.from_numpy(buf).to(cuda)
        o = torch.from_numpy(off + 61).to(cuda)
        v = torch.zeros(len(frames), dtype=torch.uint8, device=cuda)
        for filt, ports in ((None, None), (FILT, FULL)):
            got = L.rx_deliver_batch(d, o, v, None, flags=flags, filter=filt, ports=ports)
            want = host_records(sweep, np.zeros(len(sweep), np.uint8), None, filt, ports)
            assert set(want["verdict"]) == {18}
            check(got, want)


def test_records_alone(cuda, census):
    import torch
    bare, wire = census
    d, o = dev(cuda, *packed(wire[:700]))
    ok, v = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT)
    rec, order, count = L.rx_deliver_batch(d, o, v, ok, filter=FILT, ports=FULL, group=False)
    assert order is None and count is None
    check((rec, None, None), host_records(bare[:700], v.cpu().numpy(), ok.cpu().numpy(), FILT, FULL))
    assert torch.equal(rec, L.rx_deliver_batch(d, o, v, ok, filter=FILT, ports=FULL)[0])


def test_two_streams_two_threads(cuda, census):
    """Each call brings its own workspace: calls on two streams from two host threads do not meet."""
    import torch
    bare, wire = census
    halves = [(bare[:800], wire[:800]), (bare[800:1600], wire[800:1600])]
    results, errors = [None, None], []

    def work(t):
        try:
            s = torch.cuda.Stream(device=cuda)
            d, o = dev(cuda, *packed(halves[t][1]))
            torch.cuda.synchronize(cuda)
            out = []
            with torch.cuda.stream(s):
                for _ in range(6):
                    ok, v = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, stream=s)
                    out.append((ok, v) + L.rx_deliver_batch(d, o, v, ok, filter=FILT, ports=FULL, stream=s))
            s.synchronize()
            results[t] = out
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        ok, v = results[t][0][:2]
        want = host_records(halves[t][0], v.cpu().numpy(), ok.cpu().numpy(), FILT, FULL)
        for out in results[t]:
            check(out[2:], want)
