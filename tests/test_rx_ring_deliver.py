"""Receive delivery through the ring (lnx_rx_ring_set_ports,
lnx_rx_ring_ingress_deliver, lnx_ingress_packets_deliver) on
every route an internal batch can take, and on the host path.

Expected FCS results and verdicts come from the oracle (zlib's CRC,
O.ingress_verdict), the records from lnx_rx_deliver per frame on those, the
groups from numpy's stable argsort / bincount over the WHOLE call (the ring
groups each internal batch on the device and merges them on the host).  The
calls go through ctypes with their outputs pre-filled with 0xEE, and the route
is told by exact deltas of ring.stats(), as tests/test_rx_ring_routes.py does."""
import ctypes
import functools

import numpy as np
import pytest

import lneto_amd as L
from tests import deliver_ref as R
from tests import framegen as G
from tests.test_deliver_gpu import grouping, host_records
from tests.test_rx_ring import _expect, _with_fcs
from tests.test_rx_ring_routes import _delta, _ee, _ptr, _raw_ingress, _raw_slots

pytestmark = pytest.mark.gpu

EE, EE32 = 0xEE, 0xEEEEEEEE
BATCH = 64
N = 3 * BATCH + 17
LNX_OK, LNX_EINVAL = 0, -1
FULL = L.RxPorts.make(tcp=R.TCP_FULL, udp=R.UDP_FULL)
DUP = L.RxPorts.make(tcp=[7, 80, 80, 443, 0], udp=[53, 53, 0])
SPARSE_CAP, DENSE_CAP = 512, 1536


@functools.lru_cache(maxsize=None)
def _sparse():
    """N census frames of at most 300 bytes with their FCS, a quarter of the FCSs flipped."""
    frames = [f for _, f in R.census_frames() if len(f) <= 300]
    perm = np.random.default_rng(8).permutation(len(frames))[:N]
    out = []
    for i, j in enumerate(perm):
        w = bytearray(_with_fcs(frames[j]))
        if i % 4 == 2:
            w[-2] ^= 0x10
        out.append(bytes(w))
    return out


@functools.lru_cache(maxsize=None)
def _dense():
    """N frames of 1500 bytes on the wire (TCP / UDP over IPv4 / IPv6, open and closed ports): they fill their slots."""
    rng = np.random.default_rng(9)
    out = []
    for i in range(N):
        port = (1000, 1255, 9, 0, 1100)[i % 5]
        if i % 2:
            pay = rng.integers(0, 256, 1500 - 4 - 54, dtype=np.uint8).tobytes()
            f = G.ether(0x0800, G.ipv4(6, R.tcp_seg(3000 + i, port, 0x002 if i % 3 else 0x018, pay)))
        else:
            pay = rng.integers(0, 256, 1500 - 4 - 62, dtype=np.uint8).tobytes()
            f = G.ether(0x86DD, G.ipv6(17, R.udp_dgram(3000 + i, port + 1000, pay)))
        w = bytearray(_with_fcs(f))
        assert len(w) == 1500
        if i % 6 == 1:
            w[700] ^= 0x01
        out.append(bytes(w))
    return out


@functools.lru_cache(maxsize=None)
def _want(kind, ports_name):
    """(ok, verdict, rec, order, count) for the whole call."""
    wire = _sparse() if kind == "sparse" else _dense()
    ports = {"none": None, "full": FULL, "dup": DUP}[ports_name]
    ok, v = _expect(wire)
    rec = host_records([f[:-4] if len(f) >= 4 else b"" for f in wire], v, ok, None, ports)
    order, count = grouping(rec)
    # a call's frames end up in several buckets, delivered and not, good and bad FCSs
    assert (ok == 0).sum() >= 20 and (rec["verdict"] == 0).sum() >= 10 and (count > 0).sum() >= 2
    return ok, v, rec, order.astype(np.uint32), count.astype(np.uint32)


def _outs(n, ok=True, verdict=True, group=True):
    rec = np.full(16 * max(n, 1), EE, dtype=np.uint8)
    order = np.full(max(n, 1), EE32, dtype=np.uint32) if group else None
    count = np.full(R.H_COUNT + 1, EE32, dtype=np.uint32) if group else None
    return (_ee(n) if ok else None), (_ee(n) if verdict else None), rec, order, count


def _raw_slots_deliver(ring, first, count, offset, flags=0, **kw):
    o, v, rec, order, cnt = _outs(count, **kw)
    rc = L.lib.lnx_rx_ring_ingress_deliver(ring._h, first, count, offset, flags, _ptr(o), _ptr(v), _ptr(rec), _ptr(order),
                                           _ptr(cnt))
    return rc, o, v, rec.view(L.DELIVERY_DTYPE)[:count], order, cnt


def _raw_packets_deliver(ring, ptrs, lens, offset, flags=0, **kw):
    n = len(ptrs)
    arr = (ctypes.c_void_p * max(n, 1))(*ptrs)
    ln = np.array(list(lens) or [0], dtype=np.uint32)
    o, v, rec, order, cnt = _outs(n, **kw)
    rc = L.lib.lnx_ingress_packets_deliver(ring._h, arr, ln.ctypes.data, n, offset, flags, _ptr(o), _ptr(v), _ptr(rec),
                                           _ptr(order), _ptr(cnt))
    return rc, o, v, rec.view(L.DELIVERY_DTYPE)[:n], order, cnt


def _equal(got, want):
    rc, ok, v, rec, order, cnt = got
    assert rc == LNX_OK
    w_ok, w_v, w_rec, w_order, w_count = want
    assert ok is None or np.array_equal(ok, w_ok), np.flatnonzero(ok != w_ok)[:10]
    assert v is None or np.array_equal(v, w_v), np.flatnonzero(v != w_v)[:10]
    bad = np.flatnonzero(rec != w_rec)
    assert bad.size == 0, (bad[:5], rec[bad[:5]], w_rec[bad[:5]])
    if order is not None:
        assert np.array_equal(cnt, w_count), np.flatnonzero(cnt != w_count)[:10]
        assert np.array_equal(order, w_order), np.flatnonzero(order != w_order)[:10]


def _fill(ring, wire, first, offset):
    ring.slots[:] = 0xA5
    for i, f in enumerate(wire):
        ring.slots[first + i, offset:offset + len(f)] = np.frombuffer(f, np.uint8)
        ring.lengths[first + i] = offset + len(f)


ROUTES = {  # name: (frames, zero copy, host threshold, zero-copy frames of a call)
    "slots_direct": ("sparse", True, 0, N),
    "packed": ("sparse", False, 0, 0),
    "slots_copy": ("dense", True, 0, 0),
    "host": ("sparse", True, N + 1, 0),
}


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_slot_range_routes(cuda, route):
    kind, zero_copy, threshold, zc = ROUTES[route]
    wire = _sparse() if kind == "sparse" else _dense()
    first, offset = 3, 2
    ring = L.RxRing(first + N + 2, slot_cap=SPARSE_CAP if kind == "sparse" else DENSE_CAP, batch_slots=BATCH, depth=2,
                    host_threshold=threshold)
    try:
        ring.set_zero_copy(zero_copy)
        ring.set_ports(FULL)
        _fill(ring, wire, first, offset)
        host = route == "host"
        for rep in range(2):
            s0 = ring.stats()
            got = _raw_slots_deliver(ring, first, N, offset)
            assert _delta(ring, s0) == {"host_frames": N if host else 0, "device_frames": 0 if host else N,
                                        "device_batches": 0 if host else 4, "zero_copy_frames": zc}, (route, rep)
            _equal(got, _want(kind, "full"))
        # records alone; NULL fcs_ok / verdict
        got = _raw_slots_deliver(ring, first, N, offset, ok=False, verdict=False, group=False)
        _equal(got, _want(kind, "full"))
        # the ports changed between two calls change the handlers; NULL: every port has a handler
        ring.set_ports(DUP)
        _equal(_raw_slots_deliver(ring, first, N, offset), _want(kind, "dup"))
        ring.set_ports(None)
        _equal(_raw_slots_deliver(ring, first, N, offset), _want(kind, "none"))
        assert not np.array_equal(_want(kind, "dup")[2]["handler"], _want(kind, "full")[2]["handler"])
        assert not np.array_equal(_want(kind, "none")[2]["handler"], _want(kind, "full")[2]["handler"])
        # afterwards the old entry on the same ring returns what it did before
        rc, ok, v = _raw_slots(ring, first, N, offset)
        assert rc == LNX_OK and np.array_equal(ok, _want(kind, "full")[0]) and np.array_equal(v, _want(kind, "full")[1])
    finally:
        ring.close()


def _slot_ptrs(ring, idx):
    base = ring.slots.ctypes.data
    return [base + int(i) * ring.slot_cap for i in idx]


@pytest.mark.parametrize("route", ["seg_direct", "mixed", "host"])
def test_packets_routes(cuda, route):
    """Caller-owned buffers: all of them the ring's slots (kSegDirect), internal batches that alternate between
    slots and buffers elsewhere (kSegDirect, kPacked, kSegDirect, kPacked), and the host path."""
    wire = _sparse()
    offset = 2
    ring = L.RxRing(N, slot_cap=SPARSE_CAP, batch_slots=BATCH, depth=2, host_threshold=N + 1 if route == "host" else 0)
    try:
        ring.set_ports(FULL)
        slot_of = np.random.default_rng(3).permutation(N)   # frame i lives in slot slot_of[i]
        ring.slots[:] = 0x5A
        for i, f in enumerate(wire):
            ring.slots[slot_of[i], offset:offset + len(f)] = np.frombuffer(f, np.uint8)
        ptrs = _slot_ptrs(ring, slot_of)
        lens = [offset + len(f) for f in wire]
        keep = []
        direct = N
        if route == "mixed":
            direct = 0
            for k, a in enumerate(range(0, N, BATCH)):
                b = min(a + BATCH, N)
                if k % 2 == 0:
                    direct += b - a
                    continue
                for i in range(a, b):   # this batch's buffers lie outside the ring
                    keep.append(np.concatenate([np.zeros(offset, np.uint8), np.frombuffer(wire[i], np.uint8)]))
                    ptrs[i] = keep[-1].ctypes.data
            assert 0 < direct < N
        host = route == "host"
        for rep in range(2):
            s0 = ring.stats()
            got = _raw_packets_deliver(ring, ptrs, lens, offset)
            assert _delta(ring, s0) == {"host_frames": N if host else 0, "device_frames": 0 if host else N,
                                        "device_batches": 0 if host else 4,
                                        "zero_copy_frames": 0 if host else direct}, (route, rep)
            _equal(got, _want("sparse", "full"))
        _equal(_raw_packets_deliver(ring, ptrs, lens, offset, ok=False, verdict=False, group=False), _want("sparse", "full"))
        ring.set_ports(DUP)
        _equal(_raw_packets_deliver(ring, ptrs, lens, offset), _want("sparse", "dup"))
        rc, ok, v = _raw_ingress(ring, ptrs, lens, offset)
        assert rc == LNX_OK and np.array_equal(ok, _want("sparse", "full")[0]) and np.array_equal(v, _want("sparse", "full")[1])
    finally:
        ring.close()


def test_python_methods(cuda):
    wire = _sparse()
    ring = L.RxRing(N, slot_cap=SPARSE_CAP, batch_slots=BATCH, depth=3, host_threshold=0)
    try:
        ring.set_ports(FULL)
        _fill(ring, wire, 0, 0)
        want = _want("sparse", "full")
        for got in (ring.ingress_deliver(0, N), ring.ingress_packets_deliver(wire)):
            _equal((LNX_OK,) + tuple(got), want)
        ok, v, rec, order, count = ring.ingress_deliver(0, N, group=False)
        assert order is None and count is None and np.array_equal(rec, want[2])
    finally:
        ring.close()


def test_refusals_write_nothing(cuda):
    wire = _sparse()
    ring = L.RxRing(N, slot_cap=SPARSE_CAP, batch_slots=BATCH, depth=2, host_threshold=0)
    try:
        big = L.RxPorts.make()
        big.n_tcp = 257
        assert L.lib.lnx_rx_ring_set_ports(ring._h, ctypes.byref(big)) == LNX_EINVAL
        big.n_tcp, big.n_udp = 0, 257
        assert L.lib.lnx_rx_ring_set_ports(ring._h, ctypes.byref(big)) == LNX_EINVAL
        _fill(ring, wire, 0, 0)
        s0 = ring.stats()
        ptrs, lens = _slot_ptrs(ring, range(N)), [len(f) for f in wire]
        arr = (ctypes.c_void_p * N)(*ptrs)
        ln = np.array(lens, dtype=np.uint32)
        for drop in ("order", "count", "rec"):
            o, v, rec, order, cnt = _outs(N)
            args = dict(rec=_ptr(rec), order=_ptr(order), count=_ptr(cnt))
            args[drop] = None
            assert L.lib.lnx_rx_ring_ingress_deliver(ring._h, 0, N, 0, 0, _ptr(o), _ptr(v), args["rec"], args["order"],
                                                     args["count"]) == LNX_EINVAL
            assert L.lib.lnx_ingress_packets_deliver(ring._h, arr, ln.ctypes.data, N, 0, 0, _ptr(o), _ptr(v), args["rec"],
                                                     args["order"], args["count"]) == LNX_EINVAL
            assert (o == EE).all() and (v == EE).all() and (rec == EE).all() and (order == EE32).all() and (cnt == EE32).all()
        assert _delta(ring, s0) == {"host_frames": 0, "device_frames": 0, "device_batches": 0, "zero_copy_frames": 0}
        # the refused table left the ring's ports as they were: none
        _equal(_raw_slots_deliver(ring, 0, N, 0), _want("sparse", "none"))
    finally:
        ring.close()
