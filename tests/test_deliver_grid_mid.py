"""Receive delivery's grouping between the grid sizes the other files reach.

The histogram and scatter launches take G = min(ceil(n / 256), 512) workgroups,
one contiguous slice each, and deliver_scan_kernel turns the workgroups' bucket
counts into bases: its wave w owns the workgroups [w seg, (w + 1) seg),
seg = ceil(G / 16).  tests/test_deliver_gpu.py runs G = 1, 2, 4, 8 and 512; here
every shape of the scan in between runs: seg = 1 with most waves busy, ragged
segments with idle waves behind them, the step to seg = 32, and the same launches
behind the ring's deliver entries, whose internal batches lay one workspace out
for two different G.

Expected values never come from the device: the records from lnx_rx_deliver,
once per pool frame (verdicts from lnx_ingress_verdict, FCS results by
construction; through the ring the oracle's), addressed n times by index; order
and count from numpy's stable argsort / bincount of the bucket keys.

Three frames whose handler no other frame has are planted in the first, the
middle and the last workgroup's slice, so that a workgroup the scan drops or
takes twice moves a whole bucket instead of hiding inside a large one."""
import numpy as np
import pytest

import lneto_amd as L
from tests import deliver_ref as R
from tests import framegen as G
from tests.test_deliver_gpu import DUP, FILT, check, dev, grouping, host_records, packed, with_fcs
from tests.test_deliver_gpu import census, short_pool  # noqa: F401  (fixtures)

pytestmark = pytest.mark.gpu

CHUNK = 256        # deliver_kernel.hip kGrpBlock: frames per chunk
GRID_CAP = 512     # deliver_kernel.hip kGrpGridCap: workgroups of the histogram / scatter launches
SCAN_WAVES = 16    # deliver_kernel.hip kScanWaves: waves of deliver_scan_kernel
POOL = 509         # short_pool's frames (a prime: no period shared with the chunks)
FULL = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)


def grid(n):
    """slice_walk.hpp slice_grid under deliver_kernel.hip's kGrpBlock / kGrpGridCap, restated."""
    return min(max(-(-n // CHUNK), 1), GRID_CAP)


def seg(g):
    """deliver_scan_kernel: the workgroups a wave owns."""
    return -(-g // SCAN_WAVES)


def keys_of(rec):
    return np.where(rec["handler"] == R.H_NONE, R.H_COUNT, rec["handler"]).astype(np.int64)


def gather(data, off, idx):
    """The packed batch whose frame i is pool frame idx[i]: (bytes, off)."""
    lens = np.diff(off)[idx]
    boff = np.zeros(len(idx) + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    src = np.repeat(off[:-1][idx] - boff[:-1], lens) + np.arange(boff[-1], dtype=np.int64)
    out = data[src] if len(src) else np.zeros(1, np.uint8)
    assert out.nbytes < 64 << 20
    return out, boff


# ------------------------------------------------------------------ every scan shape
RARE = [G.ether(0x0800, G.ipv4(6, R.tcp_seg(40001, 7, 0x018, b"rare: tcp 7"))),       # DUP's tcp[0]
        G.ether(0x86DD, G.ipv6(6, R.tcp_seg(40002, 443, 0x018, b"rare: tcp 443"))),   # DUP's tcp[3]
        G.ether(0x88CC, b"rare: an LLDP frame of sixty bytes".ljust(46, b"."))]       # FILT's fourth EtherType


@pytest.fixture(scope="module")
def pool(short_pool):
    """short_pool's 509 frames, then the three rare ones: (bytes, off, verdict, fcs_ok, records) under FILT / DUP."""
    import ctypes
    wire, v, fcs_ok, rec = short_pool
    assert len(wire) == POOL and all(64 <= len(f) <= 128 for f in wire)
    cf = ctypes.byref(FILT)
    rv = np.array([L.lib.lnx_ingress_verdict(f, len(f), L.VERIFY_ICMP, cf) for f in RARE], dtype=np.uint8)
    rok = np.ones(len(RARE), dtype=np.uint8)
    rrec = host_records(RARE, rv, rok, FILT, DUP)
    assert rv.tolist() == [0, 0, 0]
    assert rrec["handler"].tolist() == [R.H_TCP + 0, R.H_TCP + 3, R.H_ETH + 3]
    assert not np.isin(rrec["handler"], rec["handler"]).any()   # no pool frame has one of these handlers
    data, off = packed(wire + [with_fcs(f) for f in RARE])
    return data, off, np.concatenate([v, rv]), np.concatenate([fcs_ok, rok]), np.concatenate([rec, rrec])


def planted(g, r):
    """An index in workgroup 0's slice, one in workgroup g // 2's, one in the last non-empty slice's (per = 1)."""
    return [131, (g // 2) * CHUNK + 200, (g - 1) * CHUNK + (r - 1) // 2]


def host_conditions(rec, n, g, plant):
    """What a case must be for its comparison to mean something; numpy only."""
    key = keys_of(rec)
    count = np.bincount(key, minlength=R.H_COUNT + 1)
    assert (count > 0).sum() >= 8
    big = int(np.argmax(count))
    per_slice = np.add.reduceat((key == big).astype(np.int64), np.arange(0, n, CHUNK))
    assert len(per_slice) == g
    whole = per_slice[:n // CHUNK]                     # the slices of 256 frames
    assert whole.min() != whole.max()                  # the largest bucket's share differs between whole slices
    assert len(set(per_slice.tolist())) > 1
    # every slice holds frames of the largest bucket.  (A last slice of ONE frame holds the planted frame and
    # nothing else: r = 1 asks for both, and the planted frame is what pins that workgroup's bases.)
    lone = n % CHUNK == 1 and plant[2] == n - 1
    assert (per_slice[:g - 1] > 0).all() and (per_slice[g - 1] > 0 or lone)
    assert [int(count[key[i]]) for i in plant] == [1, 1, 1]
    assert len({int(key[i]) for i in plant}) == 3
    assert [i // CHUNK for i in plant] == [0, g // 2, g - 1]


# seg = 1 with 9 and with 16 busy waves; seg = 2, wave 8 with one workgroup and waves 9..15 with none; seg = 3,
# ragged; seg = 7, wave 14 short; seg = 16, one workgroup short of full; seg 31 -> 32; seg = 32, wave 15 short by one
SHAPES = [(9, 77), (16, 256), (17, 1), (17, 77), (17, 256), (33, 1), (100, 1), (100, 77), (100, 256), (255, 77),
          (496, 256), (497, 1), (511, 77)]
SEGS = {9: 1, 16: 1, 17: 2, 33: 3, 100: 7, 255: 16, 496: 31, 497: 32, 511: 32}


assert {g for g, _ in SHAPES} == set(SEGS) and all({(g, r) for r in (1, 77, 256)} <= set(SHAPES) for g in (17, 100))


@pytest.mark.parametrize("g,r", SHAPES)
def test_every_scan_shape(cuda, pool, g, r):
    import torch
    data, off, v, fcs_ok, rec = pool
    n = (g - 1) * CHUNK + r
    assert grid(n) == g and seg(g) == SEGS[g] and -(-n // CHUNK) == g   # one chunk a workgroup
    plant = planted(g, r)
    idx = np.arange(n) % POOL
    idx[plant] = POOL + np.arange(3)
    want = rec[idx]
    host_conditions(want, n, g, plant)
    want_order, want_count = grouping(want)
    d, o = dev(cuda, *gather(data, off, idx))
    # the records launch behind the receive check
    ok, vd = L.rx_verify_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT)
    assert np.array_equal(vd.cpu().numpy(), v[idx]) and np.array_equal(ok.cpu().numpy(), fcs_ok[idx])
    two = L.rx_deliver_batch(d, o, vd, ok, filter=FILT, ports=DUP)
    check(two, want)
    # the check that writes records and keys itself
    ok1, v1, rec1, order1, count1 = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=DUP)
    assert torch.equal(ok1, ok) and torch.equal(v1, vd)
    check((rec1, order1, count1), want)
    assert torch.equal(order1, two[1]) and torch.equal(count1, two[2])
    # the planted frames stand where numpy puts them
    got_order = order1.cpu().numpy()
    for i in plant:
        assert got_order[np.flatnonzero(want_order == i)[0]] == i


# ------------------------------------------------------------------ bucket occupancy at a mid-range size
def _tcp(port, i):
    return G.ether(0x0800, G.ipv4(6, R.tcp_seg(30000 + i, port, 0x018, bytes([i & 255]) * (i % 7))))


def _udp(port, i):
    return G.ether(0x86DD, G.ipv6(17, R.udp_dgram(30000 + i, port, bytes([i & 255]) * (i % 5))))


def _plain_tiled(cuda, frames, n):
    """n valid frames without FCS cycling through `frames`, a zero verdict for each: (got, expected records)."""
    import torch
    rec = host_records(frames, np.zeros(len(frames), np.uint8), None, FILT, FULL)
    idx = np.arange(n) % len(frames)
    d, o = dev(cuda, *gather(*packed(frames), idx))
    v = torch.zeros(n, dtype=torch.uint8, device=cuda)
    return L.rx_deliver_batch(d, o, v, None, flags=L.RX_NO_FCS, filter=FILT, ports=FULL), rec[idx]


def test_bucket_extremes_at_a_ragged_scan(cuda):
    """G = 100 (seg = 7, wave 14 short, wave 15 idle): one bucket; two buckets alternating frame by frame."""
    n = 99 * CHUNK + 77
    assert grid(n) == 100 and seg(100) == 7
    # every frame in one bucket
    got, want = _plain_tiled(cuda, [_tcp(1100, i) for i in range(POOL)], n)
    assert set(want["handler"]) == {R.H_TCP + 100}
    check(got, want)
    assert np.array_equal(got[1].cpu().numpy(), np.arange(n))
    assert int(got[2][R.H_TCP + 100]) == n
    # two buckets alternating frame by frame (a pool of 2 x 509, so that the parity survives the wrap)
    got, want = _plain_tiled(cuda, [_tcp(1000, i) if i & 1 else _udp(2000, i) for i in range(2 * POOL)], n)
    assert np.array_equal(want["handler"], np.where(np.arange(n) & 1, R.H_TCP, R.H_UDP))
    check(got, want)
    assert np.array_equal(got[1].cpu().numpy(), np.concatenate([np.arange(1, n, 2), np.arange(0, n, 2)]))


# ------------------------------------------------------------------ through the ring
RING_BATCH = 17 * CHUNK             # an internal batch of G = 17
RING_N = 2 * RING_BATCH + 300       # G = 17, 17 and 2 on one workspace
RING_CAP = 512


@pytest.mark.parametrize("route", ["slots_direct", "packed"])
def test_through_the_ring(cuda, short_pool, route):
    """lnx_rx_ring_ingress_deliver over 2 x 4352 + 300 slots: the ring sizes a stage's workspace for 4352 frames and
    puts the keys behind slice_grid(n) histograms, so the last batch (G = 2) lays the same workspace out differently
    from the two full ones (G = 17).  Frames short in their slots are read in place (zero copy) or packed on the
    host; the route is told by the counters."""
    from tests.test_rx_ring import _expect
    from tests.test_rx_ring_deliver import _equal, _raw_slots_deliver
    from tests.test_rx_ring_routes import _delta
    wire = short_pool[0]
    assert [grid(b) for b in (RING_BATCH, RING_BATCH, RING_N - 2 * RING_BATCH)] == [17, 17, 2] and seg(17) == 2
    ok, v = _expect(wire)                                                   # the oracle, once per pool frame
    rec = host_records([f[:-4] for f in wire], v, ok, None, DUP)
    idx = np.arange(RING_N) % POOL
    want_rec = rec[idx]
    order, count = grouping(want_rec)                                       # over the WHOLE call
    assert (count > 0).sum() >= 8 and (ok == 0).sum() > 100
    # every internal batch holds frames of the call's largest buckets, and not the same number
    key = keys_of(want_rec)
    big = int(np.argmax(count))
    per_batch = np.add.reduceat((key == big).astype(np.int64), [0, RING_BATCH, 2 * RING_BATCH])
    assert (per_batch > 0).all() and len(set(per_batch.tolist())) == 3
    want = (ok[idx], v[idx], want_rec, order.astype(np.uint32), count.astype(np.uint32))
    offset = 2
    slots = np.full((POOL, RING_CAP), 0xA5, dtype=np.uint8)
    for j, f in enumerate(wire):
        slots[j, offset:offset + len(f)] = np.frombuffer(f, np.uint8)
    lens = np.array([offset + len(f) for f in wire], dtype=np.uint32)
    ring = L.RxRing(RING_N, slot_cap=RING_CAP, batch_slots=RING_BATCH, depth=2, host_threshold=0)
    try:
        ring.set_zero_copy(route == "slots_direct")
        ring.set_ports(DUP)
        ring.slots[:] = slots[idx]
        ring.lengths[:] = lens[idx]
        for rep in range(2):
            s0 = ring.stats()
            got = _raw_slots_deliver(ring, 0, RING_N, offset)
            assert _delta(ring, s0) == {"host_frames": 0, "device_frames": RING_N, "device_batches": 3,
                                        "zero_copy_frames": RING_N if route == "slots_direct" else 0}, (route, rep)
            _equal(got, want)
    finally:
        ring.close()
