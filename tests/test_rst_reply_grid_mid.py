"""RST replies between the grid sizes tests/test_rst_reply_gpu.py reaches.

rst_count_kernel and rst_reply_kernel take G = min(ceil(n / 256), 512)
workgroups, one contiguous slice of per = ceil(chunks / G) chunks each, and
rst_scan_kernel turns the workgroups' counts into bases.  The other file runs
G = 1, 2, 3, 6 and 512 (the last with room for every reply) and a capacity
below the demand only where a slice is one chunk.  Here: G between 7 and 511;
bases carried across runs of workgroups that count nothing; a capacity that
ends inside, at the end of and before slices of three chunks; and
rst_frames_kernel past its grid cap, three trips of its grid-stride loop.

Expected values come from the host functions, never from the device:
lnx_rx_rst_entry once per pool frame, lnx_tcp_rst_frame once per reply (its IP
ID differs) in index order.  The batches address a pool of 509 short census
frames n times."""
import ctypes

import numpy as np
import pytest

import lneto_amd as L
from tests import reply_ref as R
from tests.test_deliver_gpu import DUP, FILT, dev, host_records
from tests.test_deliver_gpu import census, short_pool  # noqa: F401  (fixtures)
from tests.test_rst_reply_gpu import CFG, chain, check, cycled, expected, forced_records, rec_tensor, run

pytestmark = pytest.mark.gpu

CHUNK = 256               # slot_frame.hpp kSlotBlock: frames per chunk
GRID_CAP = 512            # slot_frame.hpp kSlotGridCap: workgroups of the count / build launches
FRAMES_GRID_CAP = 2048    # slot_frame.hpp kSlotFramesGridCap: workgroups of the explicit-entries launch
POOL = 509                # short_pool's frames (a prime: no period shared with the chunks)


def grid(n):
    """slice_walk.hpp slice_grid under slot_frame.hpp's kSlotBlock / kSlotGridCap, restated."""
    return min(max(-(-n // CHUNK), 1), GRID_CAP)


def per(n):
    """slice_walk.hpp slice_bounds: the chunks of a workgroup's slice."""
    return -(-(-(-n // CHUNK)) // grid(n))


@pytest.fixture(scope="module")
def pool(short_pool):
    """509 census frames of 64-128 bytes on the wire, a third of their FCSs flipped: (without FCS, with, the host
    records {call flags: records} under FILT / DUP: with the FCS results, and with none)."""
    wire, v, _, rec = short_pool
    assert len(wire) == POOL and np.gcd(POOL, CHUNK) == 1
    bare = [f[:-4] for f in wire]
    return bare, wire, {0: rec, L.RX_NO_FCS: host_records(bare, v, np.ones(POOL, np.uint8), FILT, DUP)}


def pool_entries(bare, rec):
    """lnx_rx_rst_entry once per pool frame under its record: (does it queue, its entry)."""
    rec = np.ascontiguousarray(rec)
    q, entries = np.zeros(len(bare), dtype=bool), []
    for j, f in enumerate(bare):
        e = L.TcpRst()
        rc = L.lib.lnx_rx_rst_entry(f, len(f), rec.ctypes.data + 16 * j, ctypes.byref(e))
        assert rc in (0, 1)
        q[j] = rc == 1
        entries.append(e)
    return q, entries


def tiled_expected(q, entries, n, cfg, ids, cap):
    """tests/test_rst_reply_gpu.py expected() for n frames cycling through the pool: (slots, src, wanted)."""
    src = np.flatnonzero(q[np.arange(n) % len(q)])
    wanted, written = len(src), min(len(src), cap)
    slots = np.zeros((written, 64), dtype=np.uint8)
    slot, ln = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    pc = ctypes.byref(cfg)
    for k in range(written):
        assert L.lib.lnx_tcp_rst_frame(pc, ctypes.byref(entries[src[k] % len(q)]), int(ids[k]), slot, ctypes.byref(ln)) == 0
        slots[k] = slot
    return slots, src[:written].astype(np.int64), wanted


def device_records(d, o, flags, pool_rec):
    """The records of rx_verify_deliver_batch, the reply stage's input: the pool's host records, n times."""
    rec = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | flags, filter=FILT, ports=DUP, group=False)[2]
    got = rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    assert np.array_equal(got, pool_rec[np.arange(len(got)) % POOL])
    return rec


# ------------------------------------------------------------------ mid-range G
@pytest.mark.parametrize("g", [7, 16, 17, 100, 511])
def test_mid_range_grids(cuda, pool, g):
    """One chunk a workgroup, the last of 77 frames; room for every reply."""
    bare, wire, pool_rec = pool
    n = (g - 1) * CHUNK + 77
    assert grid(n) == g and per(n) == 1
    ids = chain(n)
    for flags, frames, fcs in ((0, wire, True), (L.RX_NO_FCS, bare, False)):
        _, data, off = cycled(frames, n)
        d, o = dev(cuda, data, off)
        rec = device_records(d, o, flags, pool_rec[flags])
        q, entries = pool_entries(bare, pool_rec[flags])
        want = tiled_expected(q, entries, n, CFG[fcs], ids, n)
        assert want[2] > n // 40
        if g == 7:   # the tiled expectation is the per-frame loop of the other file
            full = expected([bare[i % POOL] for i in range(n)], rec.cpu().numpy(), CFG[fcs], ids, n)
            assert full[2] == want[2] and np.array_equal(full[0], want[0]) and np.array_equal(full[1], want[1])
        # every workgroup's count differs from some other's, and the last slice queues
        counts = np.add.reduceat(q[np.arange(n) % POOL].astype(np.int64), np.arange(0, n, CHUNK))
        assert len(counts) == g and len(set(counts.tolist())) > 1 and counts[-1] > 0
        check(run(cuda, d, o, rec, CFG[fcs], ids, n, flags), want, n)


# ------------------------------------------------------------------ empty slices between full ones
def test_bases_across_empty_slices(cuda):
    """G = 100: workgroups 1..40 and 60..98 count nothing, so the bases of 41..59 and of 99 (77 frames) are
    carried across runs of zeros."""
    g = 100
    n = (g - 1) * CHUNK + 77
    assert grid(n) == g and per(n) == 1
    syns = [R.syn_frame((0xFFFFFF00 + i) & 0xFFFFFFFF, sport=1024 + i, dport=(9, 1000, 8080)[i % 3], payload=bytes(i % 5))
            for i in range(POOL)]
    frames, data, off = cycled(syns, n)
    rec = forced_records(n)
    for a, b in ((1, 41), (60, 99)):
        rec["flags"][a * CHUNK:b * CHUNK] = 0
    ids = chain(n)
    want = expected(frames, rec, CFG[True], ids, n)
    counts = np.add.reduceat(np.bincount(want[1], minlength=n), np.arange(0, n, CHUNK))
    assert counts.tolist() == [256] + [0] * 40 + [256] * 19 + [0] * 39 + [77]   # every flagged SYN queues
    assert want[2] == 20 * CHUNK + 77 and want[1][-1] == n - 1
    d, o = dev(cuda, data, off)
    check(run(cuda, d, o, rec_tensor(cuda, rec), CFG[True], ids, n, L.RX_NO_FCS), want, n)


# ------------------------------------------------------------------ capacity inside slices of several chunks
def test_capacity_inside_long_slices(cuda, pool):
    """n = 2 x 512 x 256 + 5: 1025 chunks on 512 workgroups, per = 3.  Workgroups 0..340 walk three chunks, 341
    the last two (the second of five frames), the rest none.  A capacity below the demand ends the walk inside a
    slice (`run < cap` fails after its first or second chunk, or `room` cuts a chunk short) or keeps a workgroup
    whose base is at or past it out of its loop."""
    bare, _, pool_rec = pool
    n = 2 * GRID_CAP * CHUNK + 5
    chunks = -(-n // CHUNK)
    assert (chunks, grid(n), per(n)) == (1025, 512, 3) and (chunks - 1) // 3 == 341
    _, data, off = cycled(bare, n)
    assert data.nbytes < 64 << 20
    q, entries = pool_entries(bare, pool_rec[L.RX_NO_FCS])
    cc = np.add.reduceat(q[np.arange(n) % POOL].astype(np.int64), np.arange(0, n, CHUNK))   # per chunk
    cum = np.concatenate([[0], np.cumsum(cc)])           # cum[c]: the queueing frames before chunk c
    wanted = int(cum[-1])
    base = lambda g: int(cum[3 * g])                     # noqa: E731  (the scan's base of workgroup g)
    assert wanted > n // 40 and cc[:-1].min() >= 4       # (the last chunk, five frames, may queue nothing)
    caps = {
        "none": 0,
        "one": 1,
        "a base": base(170),
        "a base + 1": base(170) + 1,
        "in a second chunk": int(cum[3 * 57 + 1]) + int(cc[3 * 57 + 1]) // 2,
        "in a third chunk": int(cum[3 * 300 + 2]) + int(cc[3 * 300 + 2]) // 2,
        "end of a second chunk": int(cum[3 * 229 + 2]),
        "all but one": wanted - 1,
        "all": wanted,
        "room to spare": wanted + 7,
    }
    # each capacity stands where its name says
    assert 0 < base(170) < wanted and base(170) + 1 < int(cum[3 * 170 + 1])
    assert cum[3 * 57 + 1] < caps["in a second chunk"] < cum[3 * 57 + 2]
    assert cum[3 * 300 + 2] < caps["in a third chunk"] < cum[3 * 300 + 3]
    assert base(229) < cum[3 * 229 + 1] < caps["end of a second chunk"] < base(230) and cc[3 * 229 + 2] > 0
    assert base(341) < wanted - 1          # the last replies belong to workgroup 341, the last with a slice
    d, o = dev(cuda, data, off)
    rec = device_records(d, o, L.RX_NO_FCS, pool_rec[L.RX_NO_FCS])
    all_ids = chain(wanted + 7)
    full = {fcs: tiled_expected(q, entries, n, CFG[fcs], all_ids, wanted + 7) for fcs in (True, False)}
    assert len(full[True][0]) == wanted
    for k, (name, cap) in enumerate(caps.items()):
        fcs = k % 2 == 0
        ids = chain(cap)
        assert len(ids) == cap and np.array_equal(ids, all_ids[:cap])   # (the chain is a running one)
        slots, src, _ = full[fcs]
        want = (slots[:min(cap, wanted)], src[:min(cap, wanted)], wanted)
        got = run(cuda, d, o, rec, CFG[fcs], ids, cap, L.RX_NO_FCS)     # uploads exactly cap IDs
        check(got, want, cap)
        assert got[2].tolist() == [min(cap, wanted), wanted], name


# ------------------------------------------------------------------ explicit entries past one pass
K = 4099                  # pool entries (a prime)
A, B = 1237, 29           # idx[i] = (A i + B) mod K, as tests/test_grid_passes.py


def test_explicit_entries_past_the_grid_cap(cuda):
    """n = 2 x 2048 x 256 + 13: three trips of rst_frames_kernel's grid-stride loop, the last of 13 entries in
    workgroup 0 alone; a row of the staged chunk holds a different entry on each trip."""
    import torch
    one_pass = FRAMES_GRID_CAP * CHUNK
    n = 2 * one_pass + 13
    assert -(-n // CHUNK) > FRAMES_GRID_CAP and -(-n // one_pass) == 3 and n % one_pass == 13
    rng = np.random.default_rng(4099)
    raw = rng.integers(0, 256, (K, 20), dtype=np.uint8)
    raw[K // 2, 8:16] = 0xFF                       # seq, ack all ones: the sums' carries
    raw[K // 3, 8:16] = 0x00
    ids = rng.integers(0, 1 << 16, K, dtype=np.uint16)
    host_idx = (A * np.arange(n, dtype=np.int64) + B) % K
    first = host_idx[:one_pass]                    # the entries of trip one against those of trips two and three
    assert (first != host_idx[one_pass:2 * one_pass]).all() and (first[:13] != host_idx[2 * one_pass:]).all()
    assert len(np.unique(host_idx)) == K
    idx = (torch.arange(n, dtype=torch.int64, device=cuda) * A + B) % K
    assert np.array_equal(idx[-20:].cpu().numpy(), host_idx[-20:])
    d_e = torch.from_numpy(raw).to(cuda)[idx].contiguous()
    d_ids = torch.from_numpy(ids.view(np.int16)).to(cuda)[idx].contiguous()
    slot, ln = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    for fcs in (False, True):
        host = np.zeros((K, 64), dtype=np.uint8)
        for k in range(K):
            e = L.TcpRst.from_buffer_copy(raw[k].tobytes())
            assert L.lib.lnx_tcp_rst_frame(ctypes.byref(CFG[fcs]), ctypes.byref(e), int(ids[k]), slot, ctypes.byref(ln)) == 0
            assert ln.value == (64 if fcs else 60)
            host[k] = slot
        assert not (host == 0xA5).all(axis=1).any()            # no reply is the sentinel row
        out = torch.full(((n + 8) * 64,), 0xA5, dtype=torch.uint8, device=cuda)
        got = L.tcp_rst_frames_batch(CFG[fcs], d_e, d_ids, out=out)
        assert got.shape == (n, 64) and got.data_ptr() == out.data_ptr()
        want = torch.from_numpy(host).to(cuda)[idx]
        if not torch.equal(got, want):
            bad = torch.nonzero((got != want).any(dim=1)).flatten()[:5].cpu().tolist()
            raise AssertionError((fcs, bad, [i // one_pass for i in bad]))
        assert bool((out.view(n + 8, 64)[n:] == 0xA5).all())   # the 8 rows behind n are untouched
