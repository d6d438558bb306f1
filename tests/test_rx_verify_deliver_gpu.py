"""The receive check and the delivery records from one read of each frame
(lnx_rx_verify_deliver_batch) on the MI355X.  Expected values
come from the two calls it replaces: L.rx_verify_batch, then lnx_rx_deliver per
frame (host_records of tests/test_deliver_gpu.py) with numpy's stable argsort /
bincount for the groups.  All five outputs must be equal, byte for byte."""
import threading

import numpy as np
import pytest

import lneto_amd as L
from tests import deliver_ref as R
from tests import framegen as G
from tests.test_deliver_gpu import DUP, FILT, FULL, dev, grouping, host_records, packed, with_fcs

pytestmark = pytest.mark.gpu

GROUP, WAVES = 56, 16            # rx_verify_kernel.hip: kRvGroup frames a wave and group, kRvBlock / 64 waves
EMPTY = L.RxPorts.make()
# 256 + 256 entries with duplicates and port 0: the first 128 of each full table, port 0, then the table again
# (a hit in the second copy would be a wrong index) and a tail that appears nowhere else
TCP_DUPFULL = R.TCP_FULL[:128] + [0] + R.TCP_FULL[:64] + R.TCP_FULL[128:191]
UDP_DUPFULL = R.UDP_FULL[:128] + [0] + R.UDP_FULL[:64] + R.UDP_FULL[128:191]
DUPFULL = L.RxPorts.make(tcp=TCP_DUPFULL, udp=UDP_DUPFULL)
assert len(TCP_DUPFULL) == 256 and len(UDP_DUPFULL) == 256


def ihl15_frames():
    """IPv4 TCP SYN frames with 40 bytes of options (IHL 15: the ports at offsets 74 / 76, the flags at 86),
    to open and to closed ports, and a few UDP ones."""
    out = []
    for i, port in enumerate((1000, 1100, 1255, 1128, 80, 0, 9, 1063, 1190, 7) * 3):
        flags = (0x002, 0x012, 0x018)[i % 3] if i >= 10 else 0x002
        out.append(G.ether(0x0800, G.ipv4(6, R.tcp_seg(20000 + i, port, flags, bytes([i]) * (i % 9)), opts=bytes(40))))
    for i, port in enumerate((2000, 2255, 53, 0, 9)):
        out.append(G.ether(0x0800, G.ipv4(17, R.udp_dgram(21000 + i, port, bytes([i]) * (3 + i)), opts=bytes(40))))
    return out


def long_frames():
    """TCP / UDP frames with 200-1460-byte payloads: the 16-lane rows of phase A (the short ones take the 8-lane rows)."""
    rng = np.random.default_rng(77)
    out = []
    for i, size in enumerate((200, 513, 1024, 1153, 1460, 1459, 700, 1281) * 3):
        pay = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
        port = (1000, 1255, 9, 0)[i % 4]
        if i % 2:
            out.append(G.ether(0x0800, G.ipv4(6, R.tcp_seg(22000 + i, port, 0x018 if i % 3 else 0x002, pay),
                                              opts=bytes(4 * (i % 3)))))
        else:
            out.append(G.ether(0x86DD, G.ipv6(17, R.udp_dgram(22000 + i, port + 1000, pay))))
    return out


@pytest.fixture(scope="module")
def frames():
    """The census frames with the IHL-15 and the long frames mixed in, in a fixed shuffle; a third of the FCSs flipped."""
    bare = [f for _, f in R.census_frames()] + ihl15_frames() * 4 + long_frames() * 2
    perm = np.random.default_rng(5).permutation(len(bare))
    bare = [bare[i] for i in perm]
    return bare, [with_fcs(f, flip=i % 3 == 1) for i, f in enumerate(bare)]


def two_calls(d, o, flags, filt, ports, group=True):
    """What the fused call must give: rx_verify_batch, then rx_deliver_batch behind it."""
    ok, v = L.rx_verify_batch(d, o, flags=flags, filter=filt)
    rec, order, count = L.rx_deliver_batch(d, o, v, ok, flags=flags & L.RX_NO_FCS, filter=filt, ports=ports, group=group)
    return ok, v, rec, order, count


def same(got, want):
    import torch
    for name, g, w in zip(("ok", "verdict", "rec", "order", "count"), got, want):
        assert (g is None) == (w is None), name
        if g is not None:
            assert g.shape == w.shape and torch.equal(g, w), (name, (g != w).nonzero()[:5].tolist())


def check_host(got, bare, filt, ports):
    """The records against lnx_rx_deliver per frame, the groups against numpy."""
    ok, v, rec, order, count = got
    want = host_records(bare, v.cpu().numpy(), ok.cpu().numpy(), filt, ports)
    rec = rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    bad = np.flatnonzero(rec != want)
    assert bad.size == 0, (bad[:5], rec[bad[:5]], want[bad[:5]])
    if order is not None:
        want_order, want_count = grouping(want)
        assert np.array_equal(count.cpu().numpy(), want_count)
        assert np.array_equal(order.cpu().numpy(), want_order)
    return want


SIZES = [0, 1, 3, 4, 5, GROUP - 1, GROUP, GROUP + 1, WAVES * GROUP - 1, WAVES * GROUP, WAVES * GROUP + 1, None]


@pytest.mark.parametrize("n", SIZES)
def test_equals_the_two_calls(cuda, frames, n):
    bare, wire = frames
    n = len(bare) if n is None else n
    assert n <= len(bare)
    for flags, batch in ((0, wire[:n]), (L.RX_NO_FCS, bare[:n])):
        d, o = dev(cuda, *packed(batch))
        for filt in (None, FILT):
            for ports in (None, DUPFULL, EMPTY):
                vf = L.VERIFY_ICMP | flags
                got = L.rx_verify_deliver_batch(d, o, flags=vf, filter=filt, ports=ports)
                same(got, two_calls(d, o, vf, filt, ports))
                want = check_host(got, bare[:n], filt, ports)
                alone = L.rx_verify_deliver_batch(d, o, flags=vf, filter=filt, ports=ports, group=False)
                assert alone[3] is None and alone[4] is None
                same(alone[:3], got[:3])
                if n == len(bare) and flags == 0 and filt is FILT and ports is DUPFULL:
                    # the batch is mixed: bad FCSs, delivered frames, RSTs, misses, and hits past the duplicates
                    assert ((want["flags"] & R.DLV_FCS) != 0).sum() > n // 4 and (want["verdict"] == 0).sum() > 100
                    assert ((want["flags"] & R.DLV_RST) != 0).sum() > 20 and len(set(want["handler"].tolist())) >= 10
                    assert (want["l4_off"] == 74).sum() > 40 and ((want["l4_off"] == 74) & (want["verdict"] == 0)).sum() > 10
                    assert R.H_TCP + 128 in want["handler"] and R.H_TCP + 255 in want["handler"]


@pytest.mark.parametrize("pad", range(8))
def test_ip4_options_at_every_misalignment(cuda, pad):
    """The IHL-15 frames' ports and flags lie past the staged bytes for every start misalignment but the smallest:
    the packed buffer shifted by 0..7 bytes between guard bytes that no frame owns."""
    import torch
    bare = ihl15_frames()
    assert all(len(f) >= 88 for f in bare if f[23] == 6)
    wire = [with_fcs(f, flip=i % 5 == 4) for i, f in enumerate(bare)]
    data, off = packed(wire)
    head = 64 + pad
    buf = np.concatenate([np.full(head, 0xA5, np.uint8), data, np.full(72 - pad, 0x5A, np.uint8)])
    d = torch.from_numpy(buf).to(cuda)
    o = torch.from_numpy(off + head).to(cuda)
    for filt, ports in ((None, None), (FILT, DUPFULL), (FILT, DUP)):
        got = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=filt, ports=ports)
        same(got, two_calls(d, o, L.VERIFY_ICMP, filt, ports))
        want = check_host(got, bare, filt, ports)
        assert (want["l4_off"] == 74).sum() >= 20
        if ports is DUPFULL:
            assert ((want["flags"] & R.DLV_RST) != 0).sum() >= 2 and (want["handler"] == R.H_TCP + 255).sum() >= 1
    assert torch.equal(d.cpu(), torch.from_numpy(buf))


def test_offsets_in_any_order(cuda, frames):
    import torch
    bare, wire = frames
    wire = wire[:600]
    data, off = packed(wire)
    d = torch.from_numpy(data).to(cuda)
    rng = np.random.default_rng(11)
    shuffled = off.copy()
    rng.shuffle(shuffled)                        # arbitrary ranges: overlaps, ends below their starts, long frames
    near = off.copy()
    near[1::2] = np.maximum(near[1::2] - 30, 0)  # every other boundary 30 bytes early: frames that start in their neighbour
    for o_np in (off[::-1].copy(), shuffled, near):
        o = torch.from_numpy(o_np).to(cuda)
        got = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=FULL)
        same(got, two_calls(d, o, L.VERIFY_ICMP, FILT, FULL))
        cut = [data[o_np[i]:max(o_np[i + 1] - 4, o_np[i])].tobytes() for i in range(len(o_np) - 1)]
        check_host(got, cut, FILT, FULL)
    assert any(len(f) == 0 for f in cut) and any(len(f) > 0 for f in cut)


def test_capped_grid_past_one_pass(cuda, frames):
    """256 CUs x 16 waves x 56 frames + 1: more groups than the capped grid's waves take in one pass."""
    import torch
    bare, wire = frames
    keep = [i for i, f in enumerate(wire) if 64 <= len(f) <= 128][:509]   # (a prime: no period shared with the groups)
    assert len(keep) == 509
    b, w = [bare[i] for i in keep], [wire[i] for i in keep]
    n = torch.cuda.get_device_properties(cuda).multi_processor_count * WAVES * GROUP + 1
    data, off = packed(w)
    reps = -(-n // len(w))
    lens = np.tile(np.diff(off), reps)[:n]
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    bdata = np.tile(data, reps)[:boff[-1]]
    assert bdata.nbytes < 64 << 20
    d, o = dev(cuda, bdata, boff)
    got = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=DUP)
    # the pool's results once, tiled
    dp, op = dev(cuda, data, off)
    okp, vp = L.rx_verify_batch(dp, op, flags=L.VERIFY_ICMP, filter=FILT)
    okp, vp = okp.cpu().numpy(), vp.cpu().numpy()
    recp = host_records(b, vp, okp, FILT, DUP)
    assert np.array_equal(got[0].cpu().numpy(), np.tile(okp, reps)[:n])
    assert np.array_equal(got[1].cpu().numpy(), np.tile(vp, reps)[:n])
    want = np.tile(recp, reps)[:n]
    rec = got[2].cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    assert np.array_equal(rec, want)
    want_order, want_count = grouping(want)
    assert np.array_equal(got[4].cpu().numpy(), want_count) and np.array_equal(got[3].cpu().numpy(), want_order)


def test_two_streams_two_threads(cuda, frames):
    """Each call brings its own workspace: calls on two streams from two host threads do not meet."""
    import torch
    bare, wire = frames
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
                    out.append(L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=FULL, stream=s))
            s.synchronize()
            results[t] = (out, two_calls(d, o, L.VERIFY_ICMP, FILT, FULL))
        except Exception as e:  # noqa: BLE001
            errors.append(e)

    threads = [threading.Thread(target=work, args=(t,)) for t in range(2)]
    for th in threads:
        th.start()
    for th in threads:
        th.join()
    assert not errors, errors
    for t in range(2):
        out, want = results[t]
        check_host(want, halves[t][0], FILT, FULL)
        for got in out:
            same(got, want)


def test_argument_refusals(cuda, frames):
    import ctypes
    import torch
    bare, wire = frames
    d, o = dev(cuda, *packed(wire[:8]))
    buf = lambda nbytes: torch.zeros(nbytes, dtype=torch.uint8, device=cuda)  # noqa: E731
    ok, v, rec, order, count, ws = buf(8), buf(8), buf(8 * 16), buf(8 * 4), buf(4 * (R.H_COUNT + 1)), buf(L.rx_deliver_ws_bytes(8))
    call = lambda n, flags, filt, ports, *p: L.lib.lnx_rx_verify_deliver_batch(  # noqa: E731
        d.data_ptr(), o.data_ptr(), n, flags, filt, ports, *p, None)
    ptrs = [t.data_ptr() for t in (ok, v, rec, order, count, ws)]
    assert call(8, 0, None, None, *ptrs) == 0
    assert call(8, 0, None, None, ptrs[0], ptrs[1], ptrs[2], ptrs[3], None, ptrs[5]) == L.LNX_EINVAL
    assert call(8, 0, None, None, ptrs[0], ptrs[1], ptrs[2], None, ptrs[4], ptrs[5]) == L.LNX_EINVAL
    assert call(8, 0, None, None, ptrs[0], ptrs[1], None, ptrs[3], ptrs[4], ptrs[5]) == L.LNX_EINVAL
    assert call(1 << 32, 0, None, None, *ptrs) == L.LNX_EINVAL
    assert call(8, 8, None, None, *ptrs) == L.LNX_EINVAL
    big = L.RxPorts.make()
    big.n_tcp = 257
    assert call(8, 0, None, ctypes.byref(big), *ptrs) == L.LNX_EINVAL
    bad = L.RxFilter.make(mac=G.MAC_US, **R.FILTER_KW)
    bad.n_ethertypes = 9
    assert call(8, 0, ctypes.byref(bad), None, *ptrs) == L.LNX_EINVAL
    # records alone: the workspace is not touched (there is none); n = 0: the counts zeroed
    assert call(8, 0, None, None, ptrs[0], ptrs[1], ptrs[2], None, None, None) == 0
    count.fill_(7)
    assert call(0, 0, None, None, *ptrs) == 0
    torch.cuda.synchronize(cuda)
    assert int(count.view(torch.int32).abs().sum()) == 0
