"""The receive ring's routing (lneto_amd/csrc/rx_ring.hip): which of the four
receive sources and two transmit forms an internal batch takes, calls that mix
them on one stage, the zero-copy refusals of egress, frames anywhere in slot
memory, argument refusals and NULL outputs.

Every expected value comes from the oracle (O.crc32, O.ingress_verdict,
O.tx_checksum, O.fcs_append), never from another route of the library, and is
compared by equality.  Routes are told apart by exact deltas of ring.stats().
The calls go straight through ctypes with their outputs pre-filled with 0xEE
(the binding zero-fills them, and zero is a valid answer), so a batch that
nobody ran shows.

The route conditions are restated here (_dense, _rx_direct, _tx_direct) and
the CPU tests assert that each planned batch takes the intended route and
holds a mix of expected values; the GPU tests then pin results and routes.

The egress frames are tx_frames of at most 1900 B in rooms of 2048 B, which
alone never give ErrShortBuffer (6); four frames of 2045-2048 B are added for
it (they fit their room as they are and cannot grow).  The slot memory of the
kSegDirect ring is 255 x 512 B, so that it is not a multiple of 4096."""
import ctypes
import functools

import numpy as np
import pytest

import lneto_amd as L
from oracle import oracle as O
from tests import framegen as G
from tests.test_rx_ring import _case_frames, _cap_for, _expect, _with_fcs
from tests.test_tx_checksum import tx_frames

EE = 0xEE
BATCH = 64
LNX_OK, LNX_EINVAL = 0, -1


# ------------------------------------------------------------------ the route conditions, restated
def _flen(length, cap, offset):
    l = min(int(length), cap)
    return l - offset if l > offset else 0


def _dense(lengths, cap, offset):
    """lnx_rx_ring_ingress: whole slots by DMA iff total * 10 >= nb * cap * 9."""
    total = sum(_flen(l, cap, offset) for l in lengths)
    return total * 10 >= len(lengths) * cap * 9


def _batches(n, per=BATCH):
    return [(a, min(a + per, n)) for a in range(0, n, per)]


def _in_ring(pos, offset, need, size):
    """in_ring(): the buffer at ring byte `pos` (None: elsewhere) holds [offset, offset + need)."""
    return pos is not None and 0 <= pos <= size and offset + need <= size - pos


def _rx_direct(views, offset, size):
    """lnx_ingress_packets, per internal batch: kSegDirect iff every non-empty frame lies in slot memory."""
    out = []
    for a, b in _batches(len(views)):
        out.append(all(max(l - offset, 0) == 0 or _in_ring(p, offset, max(l - offset, 0), size)
                       for p, l in views[a:b]))
    return out


def _tx_direct(pos, offset, capacity, cap, nslots):
    """lnx_egress_packets, per internal batch: in place iff every room [offset, offset + capacity)
    lies inside one slot and no slot serves two frames of the batch."""
    out = []
    for a, b in _batches(len(pos)):
        seen, ok = set(), True
        for p in pos[a:b]:
            if not _in_ring(p, offset, capacity, nslots * cap):
                ok = False
                break
            slot = p // cap
            if slot >= nslots or p % cap + offset + capacity > cap or slot in seen:
                ok = False
                break
            seen.add(slot)
        out.append(ok)
    return out


def _mix_ok(want_ok, want_v):
    """A batch whose expected values can tell a wrong kernel from a right one."""
    return (want_ok == 1).sum() >= 8 and (want_ok == 0).sum() >= 4 and len(set(want_v.tolist())) >= 3


# ------------------------------------------------------------------ raw calls, outputs pre-filled with 0xEE
def _ring(*a, **kw):
    kw.setdefault("host_threshold", 0)
    return L.RxRing(*a, **kw)


def _ee(n):
    return np.full(max(n, 1), EE, dtype=np.uint8)


def _delta(ring, s0):
    s1 = ring.stats()
    return {k: s1[k] - s0[k] for k in s1}


def _ptr(a):
    return a.ctypes.data if a is not None else None


def _raw_slots(ring, first, count, offset, flags=0, ok=True, verdict=True):
    o, v = (_ee(count) if ok else None), (_ee(count) if verdict else None)
    rc = L.lib.lnx_rx_ring_ingress(ring._h, first, count, offset, flags, _ptr(o), _ptr(v))
    return rc, o, v


def _raw_ingress(ring, ptrs, lens, offset, flags=0, ok=True, verdict=True):
    n = len(ptrs)
    arr = (ctypes.c_void_p * max(n, 1))(*ptrs)
    ln = np.array(list(lens) or [0], dtype=np.uint32)
    o, v = (_ee(n) if ok else None), (_ee(n) if verdict else None)
    rc = L.lib.lnx_ingress_packets(ring._h, arr, ln.ctypes.data, n, offset, flags, _ptr(o), _ptr(v))
    return rc, o, v


def _raw_egress(ring, ptrs, lens, offset, capacity, flags, status=True):
    """Returns (rc, lens after the call, status)."""
    n = len(ptrs)
    arr = (ctypes.c_void_p * max(n, 1))(*ptrs)
    ln = np.array(list(lens) or [0], dtype=np.uint32)
    st = _ee(n) if status else None
    rc = L.lib.lnx_egress_packets(ring._h, arr, ln.ctypes.data, n, offset, capacity, flags, _ptr(st))
    return rc, ln, st


def _udp_wire(wire_len, rng):
    """A valid UDP/IPv4 frame with its FCS, wire_len bytes in all."""
    pay = rng.integers(0, 256, wire_len - 4 - 42, dtype=np.uint8).tobytes()
    f = _with_fcs(G.ether(0x0800, G.ipv4(17, G.udp(pay))))
    assert len(f) == wire_len
    return f


def _damage(f, how):
    """One flipped bit: in the payload, the version nibble, the total length or the FCS itself."""
    b = bytearray(f)
    at, bit = [(len(b) // 2, 0x04), (14, 0x20), (16, 0x40), (len(b) - 1, 0x01)][how % 4]
    b[at] ^= bit
    return bytes(b)


# ================================================================== A. slot range: mixed routes in one call
A_CAP, A_FIRST, A_OFFSET = 1536, 5, 2
A_KINDS = "sdssds"           # sparse / dense per internal batch
A_COUNT = 5 * BATCH + 37     # a short last batch


@functools.lru_cache(maxsize=None)
def _plan_a():
    rng = np.random.default_rng(4100)
    pool = iter(f for f in _case_frames(seed=301, count=640) if 64 <= len(f) <= 600)
    frames = []
    for k, (a, b) in enumerate(_batches(A_COUNT)):
        for i in range(a, b):
            if A_KINDS[k] == "s":
                frames.append(next(pool))
            else:
                f = _udp_wire(1500, rng)
                frames.append(_damage(f, i // 7) if i % 7 == 3 else f)
    want_ok, want_v = _expect(frames)
    return frames, want_ok, want_v


def test_plan_mixed_slot_routes():
    frames, want_ok, want_v = _plan_a()
    assert len(frames) == A_COUNT and A_COUNT % BATCH != 0
    bs = _batches(A_COUNT)
    assert len(bs) == len(A_KINDS) == 6 and bs[-1][1] - bs[-1][0] == 37
    for k, (a, b) in enumerate(bs):
        lengths = [A_OFFSET + len(f) for f in frames[a:b]]
        assert max(lengths) <= A_CAP and _cap_for(frames[a:b], A_OFFSET) <= A_CAP
        assert _dense(lengths, A_CAP, A_OFFSET) == (A_KINDS[k] == "d"), k
        assert _mix_ok(want_ok[a:b], want_v[a:b]), (k, want_ok[a:b].sum(), set(want_v[a:b].tolist()))
    # the stage of the fix (zero copy off, depth 1): packed, whole slots, packed
    assert "sds" in A_KINDS


@pytest.mark.gpu
@pytest.mark.parametrize("zero_copy", [True, False])
@pytest.mark.parametrize("depth", [1, 2, 3])
def test_mixed_slot_routes(cuda, depth, zero_copy):
    """Sparse and dense internal batches alternate in one lnx_rx_ring_ingress
    call, so each stage serves kSlotsDirect / kPacked and kSlotsCopy in turn;
    a second call on the untouched ring reuses every stage's staging after a
    different route.  Zero copy off at depth 1 is the packed, dense, packed
    sequence in which the staging must stay busy across the dense batch."""
    frames, want_ok, want_v = _plan_a()
    ring = _ring(A_FIRST + A_COUNT, slot_cap=A_CAP, batch_slots=BATCH, depth=depth)
    try:
        ring.set_zero_copy(zero_copy)
        ring.slots[:] = 0xA5
        for i, f in enumerate(frames):
            ring.slots[A_FIRST + i, A_OFFSET:A_OFFSET + len(f)] = np.frombuffer(f, np.uint8)
            ring.lengths[A_FIRST + i] = A_OFFSET + len(f)
        sparse = sum(b - a for k, (a, b) in enumerate(_batches(A_COUNT)) if A_KINDS[k] == "s")
        for rep in range(2):
            s0 = ring.stats()
            rc, ok, verdict = _raw_slots(ring, A_FIRST, A_COUNT, A_OFFSET)
            assert rc == LNX_OK
            d = _delta(ring, s0)
            assert not (ok == EE).any() and not (verdict == EE).any(), rep
            assert np.array_equal(ok, want_ok), (rep, np.flatnonzero(ok != want_ok)[:10])
            assert np.array_equal(verdict, want_v), (rep, np.flatnonzero(verdict != want_v)[:10])
            assert d == {"host_frames": 0, "device_frames": A_COUNT, "device_batches": len(A_KINDS),
                         "zero_copy_frames": sparse if zero_copy else 0}, (rep, d)
    finally:
        ring.close()


# ================================================================== B. the 90 % boundary
B_CAP = 1000
B_CASES = {  # offset -> the frames' wire lengths, 64 of them, at the boundary
    0: [900] * 64,
    4: [880, 920] * 32,
}


def test_plan_dense_boundary():
    for offset, lens in B_CASES.items():
        assert len(lens) == BATCH
        at = [offset + l for l in lens]
        assert sum(lens) * 10 == BATCH * B_CAP * 9 and max(at) <= B_CAP
        assert _dense(at, B_CAP, offset)
        below = [at[0] - 1] + at[1:]
        assert sum(lens) * 10 - 10 < BATCH * B_CAP * 9
        assert not _dense(below, B_CAP, offset)


@pytest.mark.gpu
@pytest.mark.parametrize("offset", sorted(B_CASES))
def test_dense_boundary(cuda, offset):
    """total * 10 == nb * cap * 9 exactly: the batch goes up as whole slots
    (no zero-copy frames); one byte less in one frame and it is read in place."""
    rng = np.random.default_rng(4200 + offset)
    ring = _ring(BATCH, slot_cap=B_CAP, batch_slots=BATCH, depth=2)
    try:
        for short in (0, 1):
            lens = list(B_CASES[offset])
            lens[0] -= short
            frames = [_udp_wire(l, rng) for l in lens]
            ring.slots[:] = 0x5A
            for i, f in enumerate(frames):
                ring.slots[i, offset:offset + len(f)] = np.frombuffer(f, np.uint8)
                ring.lengths[i] = offset + len(f)
            want_ok, want_v = _expect(frames)
            assert want_ok.all() and not want_v.any()
            s0 = ring.stats()
            rc, ok, verdict = _raw_slots(ring, 0, BATCH, offset)
            assert rc == LNX_OK
            d = _delta(ring, s0)
            assert np.array_equal(ok, want_ok) and np.array_equal(verdict, want_v), short
            assert d == {"host_frames": 0, "device_frames": BATCH, "device_batches": 1,
                         "zero_copy_frames": BATCH if short else 0}, (short, d)
    finally:
        ring.close()


# ================================================================== C. buffers anywhere in slot memory
C_CAP, C_NSLOTS = 512, 255
C_SIZE = C_CAP * C_NSLOTS


@functools.lru_cache(maxsize=None)
def _plan_c(offset):
    """(image of slot memory, views [(start byte, length)], notes): `offset` bytes of headroom, then the
    frame, per view.  The data is laid out first; the views are cut afterwards, some of them running
    1-40 bytes into their neighbour."""
    rng = np.random.default_rng(4300 + offset)
    pool = [f for f in _case_frames(seed=311, count=900) if len(f) <= 508][:230]
    pool += [_udp_wire(int(l), rng) for l in rng.integers(300, 509, 60)]
    pool += [_damage(_udp_wire(int(l), rng), i) for i, l in enumerate(rng.integers(200, 509, 10))]
    order = rng.permutation(len(pool))
    pool = [pool[i] for i in order]
    image = rng.integers(0, 256, C_SIZE, dtype=np.uint8)
    views, notes = [], {"overlap": [], "cross": 0}
    cur, grow = 0, 0
    for i, f in enumerate(pool):
        n = offset + len(f)
        if i == len(pool) - 1:
            start = C_SIZE - n                      # ends on the last byte of slot memory
        elif i == 0 or grow:
            start = cur                             # byte 0; or right behind a view that runs into this one
        else:
            start = cur + (i - cur) % 128           # view start residue i mod 128
        assert start >= cur and start + n <= C_SIZE
        image[start + offset:start + n] = np.frombuffer(f, np.uint8)
        if grow:                                    # the previous view takes `grow` bytes of this one
            p, l = views[-1]
            views[-1] = (p, l + grow)
            notes["overlap"].append(len(views) - 1)
        grow = 0
        if i % 6 == 4 and i + 2 < len(pool):
            k = 1 + (7 * i) % 40
            if n + k <= C_CAP and k <= offset + len(pool[i + 1]):
                grow = k
        views.append((start, n))
        cur = start + n
    views += [(1000, 0), (C_SIZE, 0), (C_CAP * 9 - 1, min(offset, 1)), (None, 0)]   # empty views
    views = [views[i] for i in rng.permutation(len(views))]                          # shuffled
    for at in (7, BATCH + 20, 3 * BATCH + 1):                                        # the same view twice
        views.insert(at + 5, views[at])
    # the view that the second call takes from a buffer outside the ring: one of the third internal batch
    notes["outside"] = next(i for i in range(2 * BATCH, 3 * BATCH) if views[i][0] is not None
                            and views[i][1] > offset + 64)
    notes["cross"] = sum(1 for p, l in views if p is not None and l > offset and p // C_CAP != (p + l - 1) // C_CAP)
    return image, views, notes


def _view_bytes(image, views, offset):
    return [image[p + offset:p + l].tobytes() if p is not None and l > offset else b"" for p, l in views]


@pytest.mark.parametrize("offset", [0, 2])
def test_plan_views_in_slot_memory(offset):
    image, views, notes = _plan_c(offset)
    assert C_SIZE % 4096 != 0 and C_CAP % 4 == 0
    n = len(views)
    assert 290 <= n <= 330 and len(_batches(n)) == 5
    assert all(l <= C_CAP for _, l in views)
    real = [(p, l) for p, l in views if p is not None and l > offset]
    assert {(p + offset) % 128 for p, _ in real} == set(range(128))
    assert notes["cross"] >= 20
    assert len(notes["overlap"]) >= 20
    spans = sorted(set(real))
    lap = [a[0] + a[1] - b[0] for a, b in zip(spans, spans[1:]) if a[0] + a[1] > b[0]]
    assert len(lap) >= 20 and min(lap) >= 1 and max(lap) <= 40
    assert sum(1 for a, b in _batches(n) if len(set(views[a:b])) < b - a) >= 3      # twice in one batch
    assert [p for p, _ in views if p is not None] != sorted(p for p, _ in views if p is not None)
    assert sum(1 for _, l in views if l <= offset) >= 4 and (None, 0) in views
    assert any(p == 0 and l > offset for p, l in views)
    assert any(p is not None and p + l == C_SIZE and l > offset for p, l in views)
    assert all(_rx_direct(views, offset, C_SIZE))
    out = list(views)
    out[notes["outside"]] = (None, views[notes["outside"]][1])
    assert _rx_direct(out, offset, C_SIZE) == [True, True, False, True, True]
    want_ok, want_v = _expect(_view_bytes(image, views, offset))
    for a, b in _batches(n):
        assert _mix_ok(want_ok[a:b], want_v[a:b]), (a, want_ok[a:b].sum(), set(want_v[a:b].tolist()))
    # a view that runs into its neighbour is a frame of its own (its FCS no longer fits)
    assert (want_ok == 1).sum() >= 150


@pytest.mark.gpu
@pytest.mark.parametrize("offset", [0, 2])
@pytest.mark.parametrize("depth", [2, 1])
def test_views_in_slot_memory(cuda, depth, offset):
    """lnx_ingress_packets on views of slot memory at any byte (kSegDirect, the
    HOST = true receive kernel on a caller's frame table): every start residue
    mod 128, across slot edges, overlapping, repeated, shuffled, empty, at byte 0
    and up to the last byte.  Then one buffer outside the ring in the third
    internal batch: that batch alone is packed (depth 1: direct, direct, packed,
    direct, direct on one stage)."""
    image, views, notes = _plan_c(offset)
    n, out_at = len(views), notes["outside"]
    want_ok, want_v = _expect(_view_bytes(image, views, offset))
    ring = _ring(C_NSLOTS, slot_cap=C_CAP, batch_slots=BATCH, depth=depth)
    try:
        flat = ring.slots.reshape(-1)
        flat[:] = image
        base = flat.ctypes.data
        ptrs = [base + p if p is not None else None for p, _ in views]
        lens = [l for _, l in views]
        outside = np.frombuffer(image[views[out_at][0]:views[out_at][0] + lens[out_at]].tobytes(), np.uint8)
        mixed = list(ptrs)
        mixed[out_at] = outside.ctypes.data
        third = _batches(n)[2]
        for which, pp, zc in (("ring", ptrs, n), ("one outside", mixed, n - (third[1] - third[0]))):
            s0 = ring.stats()
            rc, ok, verdict = _raw_ingress(ring, pp, lens, offset)
            assert rc == LNX_OK
            d = _delta(ring, s0)
            assert not (ok == EE).any() and not (verdict == EE).any(), which
            bad = np.flatnonzero((ok != want_ok) | (verdict != want_v))
            assert bad.size == 0, (which, [(int(i), views[i], int(ok[i]), int(want_ok[i]), int(verdict[i]),
                                            int(want_v[i])) for i in bad[:10]])
            assert d == {"host_frames": 0, "device_frames": n, "device_batches": 5, "zero_copy_frames": zc}, (which, d)
            assert np.array_equal(flat, image), which
    finally:
        ring.close()


# ================================================================== D. egress: refusals and in-place work
D_CAP, D_NSLOTS, D_CAPACITY, D_N = 4096, 128, 2048, 150
D_SIZE = D_CAP * D_NSLOTS
D_BIG = (30, 31, 32, 33)     # frames of 2045-2048 B: no room to grow, ErrShortBuffer
D_OUT = BATCH + 16           # case 6 / 7: the buffer outside the ring


@functools.lru_cache(maxsize=None)
def _tx_set():
    rng = np.random.default_rng(4400)
    frames = [f for f in tx_frames(seed=77, count=400) if len(f) <= 1900][:D_N - len(D_BIG)]
    for k, i in enumerate(D_BIG):
        pay = rng.integers(0, 256, 2045 + k - 54, dtype=np.uint8).tobytes()
        frames.insert(i, G.ether(0x0800, G.ipv4(6, G.tcp(pay), fix_l4=False)))
    assert len(frames) == D_N and [len(frames[i]) for i in D_BIG] == [2045, 2046, 2047, 2048]
    return frames


@functools.lru_cache(maxsize=None)
def _tx_want(flags):
    """[(finished frame, status)] by the oracle."""
    out = []
    for f in _tx_set():
        want, st = O.tx_checksum(f) if flags & L.TX_CHECKSUM else (f, 0)
        st2 = 0
        if flags & L.TX_FCS:
            want, st2 = O.fcs_append(want, D_CAPACITY)
        out.append((want, st or st2))
    return out


def _slot(i, byte):
    return i * D_CAP + byte


def _d_layout(case, offset=0):
    """Ring byte of each frame's buffer (None: outside the ring) and the internal batches that
    must be refused.  Base: frame i < 128 in slot i at byte i % 16, the third batch in the upper
    halves of slots 0..21 (rooms inside their slot, one frame per slot and batch)."""
    frames = _tx_set()
    pos = [_slot(i, i % 16) if i < D_NSLOTS else _slot(i - D_NSLOTS, 2040 - offset) for i in range(D_N)]
    refused = []
    if case == "two per slot":
        pos = [_slot(i // 2, 2048 * (i % 2)) for i in range(D_N)]
        refused = [0, 1, 2]
    elif case == "two per slot, second batch":
        pos[BATCH + 1] = _slot(BATCH, 2048)         # with frame 64 at byte 0 of slot 64
        refused = [1]
    elif case == "room crosses a slot edge":
        j = next(i for i in range(BATCH, 2 * BATCH - 1) if 1100 < len(frames[i]) <= 1900)
        pos[j] = _slot(j, 3000)                     # the frame itself runs into slot j + 1,
        pos[j + 1] = _slot(40, 2040)                # whose frame moves to a free upper half
        refused = [1]
    elif case == "room past the end":
        j = next(i for i in range(BATCH, 2 * BATCH - 1) if 200 < len(frames[i]) <= 1000)
        pos[j], pos[D_NSLOTS - 1] = _slot(D_NSLOTS - 1, 3000), pos[j]
        refused = [1]
    elif case == "one outside":
        pos[D_OUT] = None
        refused = [1]
    else:
        assert case == "allowed"
    return pos, refused


D_CASES = [("allowed", 0), ("allowed", 3), ("two per slot", 0), ("two per slot, second batch", 0),
           ("room crosses a slot edge", 0), ("room past the end", 0), ("one outside", 0)]


def test_plan_egress_routes():
    frames = _tx_set()
    want = _tx_want(L.TX_CHECKSUM | L.TX_FCS)
    assert sum(1 for f, (w, _) in zip(frames, want) if w != f) > D_N // 2
    statuses = {st for _, st in want}
    assert len(statuses) >= 3 and O.ERR_SHORT_BUFFER in statuses and O.ERR_SHORT_BUFFER == 6
    assert {st for _, st in _tx_want(L.TX_FCS)} == {0, 6}
    assert len({st for _, st in _tx_want(L.TX_CHECKSUM)}) >= 3
    nb = len(_batches(D_N))
    assert nb == 3
    for case, offset in D_CASES:
        pos, refused = _d_layout(case, offset)
        direct = _tx_direct(pos, offset, D_CAPACITY, D_CAP, D_NSLOTS)
        assert direct == [k not in refused for k in range(nb)], (case, offset, direct)
        # the finished frames lie in slot memory and are disjoint
        spans = sorted((p + offset, p + offset + len(w)) for p, (w, _) in zip(pos, want) if p is not None)
        assert spans[-1][1] <= D_SIZE
        assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:])), (case, offset)
        if case == "two per slot":      # the rooms themselves do not overlap
            assert all(b - a >= D_CAPACITY for a, b in zip(sorted(pos), sorted(pos)[1:]))
        if case == "room crosses a slot edge":
            j = next(i for i, p in enumerate(pos) if p % D_CAP == 3000)
            assert pos[j] // D_CAP != (pos[j] + len(want[j][0]) - 1) // D_CAP and pos[j] + D_CAPACITY <= D_SIZE
        if case == "room past the end":
            j = next(i for i, p in enumerate(pos) if p % D_CAP == 3000)
            assert pos[j] + D_CAPACITY > D_SIZE and pos[j] // D_CAP == D_NSLOTS - 1
    # each rule alone refuses its case: without it the batch would be taken
    assert all(_in_ring(p, 0, D_CAPACITY, D_SIZE) for p in _d_layout("two per slot")[0])
    assert all(_in_ring(p, 0, D_CAPACITY, D_SIZE) for p in _d_layout("room crosses a slot edge")[0])


def _run_egress(ring, case, offset, flags, junk):
    """One lnx_egress_packets call on a ring freshly filled with junk and the case's frames; checks
    every finished frame, length and status against the oracle, all other memory against the junk and
    the zero-copy count against the refused batches."""
    frames, want = _tx_set(), _tx_want(flags)
    pos, refused = _d_layout(case, offset)
    flat = ring.slots.reshape(-1)
    flat[:] = junk
    expect = junk.copy()
    base = flat.ctypes.data
    outside = out_expect = None
    ptrs = []
    for i, (p, f) in enumerate(zip(pos, frames)):
        w = np.frombuffer(want[i][0], np.uint8)
        if p is None:
            outside = junk[:offset + D_CAPACITY + 16].copy()
            outside[offset:offset + len(f)] = np.frombuffer(f, np.uint8)
            out_expect = outside.copy()
            out_expect[offset:offset + len(w)] = w
            ptrs.append(outside.ctypes.data)
        else:
            flat[p + offset:p + offset + len(f)] = np.frombuffer(f, np.uint8)
            expect[p + offset:p + offset + len(w)] = w
            ptrs.append(base + p)
    s0 = ring.stats()
    rc, lens, status = _raw_egress(ring, ptrs, [len(f) for f in frames], offset, D_CAPACITY, flags)
    assert rc == LNX_OK, (case, L.lib.lnx_last_error())
    d = _delta(ring, s0)
    bad = [(i, len(frames[i]), int(lens[i]), len(w), int(status[i]), st)
           for i, (w, st) in enumerate(want) if int(lens[i]) != len(w) or int(status[i]) != st]
    assert not bad, (case, offset, bad[:10])
    diff = np.flatnonzero(flat != expect)
    assert diff.size == 0, (case, offset, [(int(x) // D_CAP, int(x) % D_CAP) for x in diff[:10]])
    if outside is not None:
        assert np.array_equal(outside, out_expect), case
    taken = sum(b - a for k, (a, b) in enumerate(_batches(D_N)) if k not in refused)
    assert d == {"host_frames": 0, "device_frames": D_N, "device_batches": 3, "zero_copy_frames": taken}, (case, d)


@pytest.fixture(scope="module")
def tx_junk():
    return np.random.default_rng(4401).integers(0, 256, D_SIZE, dtype=np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("case,offset", D_CASES)
def test_egress_routes(cuda, tx_junk, case, offset):
    """lnx_egress_packets on buffers in slot memory: patched in place where every
    room lies in one slot and no slot serves two frames of the internal batch;
    each refusal (two frames in a slot, a room across a slot edge, a room past
    the end of slot memory, a buffer elsewhere) sends that batch, and only
    that batch, through the copying form with the same results."""
    ring = _ring(D_NSLOTS, slot_cap=D_CAP, batch_slots=BATCH, depth=2)
    try:
        _run_egress(ring, case, offset, L.TX_CHECKSUM | L.TX_FCS, tx_junk)
    finally:
        ring.close()


@pytest.mark.gpu
@pytest.mark.parametrize("flags", [L.TX_CHECKSUM | L.TX_FCS, L.TX_FCS, L.TX_CHECKSUM])
def test_egress_one_stage_alternates(cuda, tx_junk, flags):
    """Depth 1: the one stage goes in place, copied, in place."""
    ring = _ring(D_NSLOTS, slot_cap=D_CAP, batch_slots=BATCH, depth=1)
    try:
        _run_egress(ring, "one outside", 0, flags, tx_junk)
    finally:
        ring.close()


# ================================================================== E. refusals and NULL outputs
E_CAP, E_NSLOTS = 512, 256


@functools.lru_cache(maxsize=None)
def _e_frames():
    frames = [f for f in _case_frames(seed=321, count=600) if len(f) <= 500][:200]
    assert len(frames) == 200
    return frames


@pytest.mark.gpu
def test_argument_refusals_touch_nothing(cuda):
    """Every argument error returns LNX_EINVAL before anything is written: the
    caller's lens, status, fcs_ok, verdict and buffers stay as they were."""
    ring = _ring(E_NSLOTS, slot_cap=E_CAP, batch_slots=BATCH, depth=2)
    try:
        rng = np.random.default_rng(4500)
        bufs = [rng.integers(0, 256, E_CAP + 8, dtype=np.uint8) for _ in range(70)]
        before = [b.copy() for b in bufs]
        ptrs = [b.ctypes.data for b in bufs]
        s0 = ring.stats()

        def rx(what, ptrs_, lens_, offset=0):
            rc, ok, v = _raw_ingress(ring, ptrs_, lens_, offset)
            assert rc == LNX_EINVAL, what
            assert (ok == EE).all() and (v == EE).all(), what

        def tx(what, ptrs_, lens_, capacity=E_CAP, flags=3):
            rc, ln, st = _raw_egress(ring, ptrs_, lens_, 0, capacity, flags)
            assert rc == LNX_EINVAL, what
            assert (st == EE).all() and ln.tolist() == list(lens_), what

        for first, count in ((E_NSLOTS - 69, 70), (E_NSLOTS, 1), (2 ** 32 - 1, 2)):
            rc, ok, v = _raw_slots(ring, first, count, 0)
            assert rc == LNX_EINVAL and (ok == EE).all() and (v == EE).all(), (first, count)
        for offset in (E_CAP, E_CAP + 1, 2 ** 32 - 1):
            rc, ok, v = _raw_slots(ring, 0, 70, offset)
            assert rc == LNX_EINVAL and (ok == EE).all() and (v == EE).all(), offset
            rx(("offset", offset), ptrs, [100] * 70, offset)
        rx("lens > slot_cap", ptrs, [100] * 69 + [E_CAP + 1])
        rx("NULL buffer with a length", ptrs[:30] + [None] + ptrs[31:], [100] * 70)
        tx("capacity > slot_cap", ptrs, [100] * 70, capacity=E_CAP + 1)
        tx("lens > capacity", ptrs, [100] * 69 + [301], capacity=300)
        for bit in (4, 8, 1 << 31):
            tx(("flag", bit), ptrs, [100] * 70, flags=3 | bit)
        tx("NULL buffer with a length", ptrs[:30] + [None] + ptrs[31:], [100] * 70)
        tx("NULL empty buffer that the FCS would grow", ptrs[:30] + [None] + ptrs[31:], [100] * 30 + [0] + [100] * 39)
        tx("the same, FCS only", ptrs[:30] + [None] + ptrs[31:], [100] * 30 + [0] + [100] * 39, flags=L.TX_FCS)
        assert ring.stats() == s0
        assert all(np.array_equal(a, b) for a, b in zip(bufs, before))
    finally:
        ring.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host", "device"])
def test_null_empty_buffer_checksum_only(cuda, route):
    """A NULL buffer of length 0 with LNX_TX_CHECKSUM alone is allowed (nothing
    is read or written): the host route and the device route (the copying form;
    NULL is not in the ring) both give LNX_OK, length 0 and the oracle's status
    of an empty frame, and finish the frames around it.  So does an empty room
    (capacity 0) at the very end of slot memory, which has no slot."""
    n, thr = (8, L.HOST_BATCH_DEFAULT) if route == "host" else (200, 0)
    frames = [f for f in tx_frames(seed=78, count=400) if len(f) <= 400][:n]
    want = [O.tx_checksum(f) for f in frames]
    empty_status = O.tx_checksum(b"")[1]
    assert empty_status == O.ERR_TRUNCATED_FRAME
    null_at = [3] if route == "host" else [3, BATCH + 9, 199]
    ring = L.RxRing(E_NSLOTS, slot_cap=E_CAP, batch_slots=BATCH, depth=2, host_threshold=thr)
    try:
        for where in ("elsewhere", "ring"):
            ring.slots[:] = 0x33
            bufs = [np.full(E_CAP, 0x33, dtype=np.uint8) if where == "elsewhere" else ring.slots[i] for i in range(n)]
            ptrs, lens = [], []
            for i, f in enumerate(frames):
                if i in null_at:
                    ptrs.append(None)
                    lens.append(0)
                else:
                    bufs[i][:len(f)] = np.frombuffer(f, np.uint8)
                    ptrs.append(bufs[i].ctypes.data)
                    lens.append(len(f))
            s0 = ring.stats()
            rc, ln, st = _raw_egress(ring, ptrs, lens, 0, E_CAP, L.TX_CHECKSUM)
            assert rc == LNX_OK
            d = _delta(ring, s0)
            for i, (w, s) in enumerate(want):
                if i in null_at:
                    assert (int(ln[i]), int(st[i])) == (0, empty_status), (where, i)
                else:
                    assert (int(ln[i]), int(st[i])) == (len(w), s), (where, i)
                    assert bufs[i][:len(w)].tobytes() == w and (bufs[i][len(w):] == 0x33).all(), (where, i)
            if route == "host":
                assert d == {"host_frames": n, "device_frames": 0, "device_batches": 0, "zero_copy_frames": 0}
            else:   # in the ring, the batches with a NULL buffer are refused
                zc = sum(b - a for a, b in _batches(n) if not any(a <= x < b for x in null_at)) if where == "ring" else 0
                assert d == {"host_frames": 0, "device_frames": n, "device_batches": 4, "zero_copy_frames": zc}, d
        # empty rooms at the end of slot memory
        image = ring.slots.copy()
        end = ring.slots.reshape(-1).ctypes.data + E_CAP * E_NSLOTS
        for flags, status in ((L.TX_CHECKSUM, empty_status), (L.TX_FCS, O.fcs_append(b"", 0)[1])):
            rc, ln, st = _raw_egress(ring, [end] * n, [0] * n, 0, 0, flags)
            assert rc == LNX_OK and not ln[:n].any() and (st[:n] == status).all(), (flags, st[:8])
        assert np.array_equal(ring.slots, image)
    finally:
        ring.close()


@pytest.mark.gpu
@pytest.mark.parametrize("route", ["host", "device"])
def test_null_outputs(cuda, route):
    """fcs_ok, verdict and status may each be NULL: the call succeeds, runs, and
    fills the other array as the oracle says."""
    n, thr = (8, L.HOST_BATCH_DEFAULT) if route == "host" else (200, 0)
    frames = _e_frames()[:n]
    want_ok, want_v = _expect(frames)
    assert route == "host" or _mix_ok(want_ok, want_v)
    ran = {"host_frames": n, "device_frames": 0} if route == "host" else {"host_frames": 0, "device_frames": n}
    ring = L.RxRing(E_NSLOTS, slot_cap=E_CAP, batch_slots=BATCH, depth=2, host_threshold=thr)
    try:
        ring.slots[:] = 0
        for i, f in enumerate(frames):
            ring.slots[i, :len(f)] = np.frombuffer(f, np.uint8)
            ring.lengths[i] = len(f)
        own = [np.frombuffer(f or b"\0", np.uint8) for f in frames]
        for ok_on, v_on in ((False, True), (True, False), (False, False)):
            for entry in ("slots", "packets in the ring", "packets elsewhere"):
                s0 = ring.stats()
                if entry == "slots":
                    rc, ok, v = _raw_slots(ring, 0, n, 0, ok=ok_on, verdict=v_on)
                else:
                    ptrs = [ring.slots[i].ctypes.data if "ring" in entry else own[i].ctypes.data for i in range(n)]
                    rc, ok, v = _raw_ingress(ring, ptrs, [len(f) for f in frames], 0, ok=ok_on, verdict=v_on)
                assert rc == LNX_OK, (entry, ok_on, v_on)
                d = _delta(ring, s0)
                assert {k: d[k] for k in ran} == ran, (entry, d)
                assert ok is None or np.array_equal(ok, want_ok), (entry, ok_on, v_on)
                assert v is None or np.array_equal(v, want_v), (entry, ok_on, v_on)
        # egress with a NULL status: lengths and frames as the oracle says
        tx = [f for f in tx_frames(seed=79, count=400) if len(f) <= 400][:n]
        for where in ("ring", "elsewhere"):
            bufs = [ring.slots[i] if where == "ring" else np.zeros(E_CAP, dtype=np.uint8) for i in range(n)]
            for b, f in zip(bufs, tx):
                b[:] = 0x44
                b[:len(f)] = np.frombuffer(f, np.uint8)
            s0 = ring.stats()
            rc, ln, st = _raw_egress(ring, [b.ctypes.data for b in bufs], [len(f) for f in tx], 0, E_CAP, 3, status=False)
            assert rc == LNX_OK and st is None
            d = _delta(ring, s0)
            assert {k: d[k] for k in ran} == ran, (where, d)
            for i, f in enumerate(tx):
                w, _ = O.fcs_append(O.tx_checksum(f)[0], E_CAP)
                assert int(ln[i]) == len(w) and bufs[i][:len(w)].tobytes() == w, (where, i)
                assert (bufs[i][len(w):] == 0x44).all(), (where, i)
    finally:
        ring.close()
