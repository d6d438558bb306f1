"""RST replies for SYNs to closed ports on the MI355X (lnx_rx_rst_reply_batch,
lnx_tcp_rst_frames_batch).  Expected values come from the host
functions in a loop over the records the call is given: lnx_rx_rst_entry, then
lnx_tcp_rst_frame for every entry, in index order (tests/test_rst_reply.py pins
both against the restatement).  Slots, sources and counts must be equal byte
for byte, and nothing at or past the written count may be touched."""
import ctypes
import threading

import numpy as np
import pytest

import lneto_amd as L
from tests import reply_ref as R
from tests.test_deliver_gpu import DUP, FILT, dev, host_records, packed, with_fcs

pytestmark = pytest.mark.gpu

CHUNK, GRID_CAP = 256, 512       # slot_frame.hpp: kSlotBlock frames a chunk, kSlotGridCap workgroups
CFG = {fcs: L.RstCfg.make(mac=R.MAC, gw_mac=R.GW_MAC, ip4=R.IP4, fcs=fcs) for fcs in (False, True)}
FILL = 0xA5
PAD = 8                          # sentinel rows behind the capacity


def chain(n, seed=0x0BAD):
    return np.array(L.ip4_id_chain(R.IP4[0], seed, n), dtype=np.uint16)


def expected(frames, rec, cfg, ids, cap):
    """(slots [written, 64], src, wanted) from the host functions; rec: the records as a numpy array."""
    rec = np.ascontiguousarray(rec)
    base, e, slot, ln = rec.ctypes.data, L.TcpRst(), (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    out, src, wanted = [], [], 0
    for i, f in enumerate(frames):
        rc = L.lib.lnx_rx_rst_entry(f, len(f), base + 16 * i, ctypes.byref(e))
        assert rc in (0, 1)
        if rc == 1:
            if wanted < cap:
                assert L.lib.lnx_tcp_rst_frame(ctypes.byref(cfg), ctypes.byref(e), int(ids[wanted]), slot, ctypes.byref(ln)) == 0
                out.append(bytes(slot))
                src.append(i)
            wanted += 1
    return np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 64), np.array(src, dtype=np.int64), wanted


def run(cuda, d, o, rec, cfg, ids, cap, flags=0, stream=None):
    """The C entry on sentinel-filled outputs of cap + PAD rows: (reply, src, d_n) as numpy arrays."""
    import torch
    n = o.numel() - 1
    with torch.cuda.stream(stream or torch.cuda.current_stream(cuda)):   # the fills, the call and the copies on one stream
        reply = torch.full((cap + PAD, 64), FILL, dtype=torch.uint8, device=cuda)
        src = torch.full((cap + PAD,), -1, dtype=torch.int32, device=cuda)
        d_n = torch.full((2,), -1, dtype=torch.int32, device=cuda)
        d_ids = torch.from_numpy(np.ascontiguousarray(ids[:cap]).view(np.int16).copy()).to(cuda) if cap else None
        ws = torch.full((L.rx_rst_ws_bytes(n),), FILL, dtype=torch.uint8, device=cuda)
        assert reply.data_ptr() % 64 == 0
        rc = L.lib.lnx_rx_rst_reply_batch(d.data_ptr(), o.data_ptr(), n, flags, rec.data_ptr(), ctypes.byref(cfg),
                                          d_ids.data_ptr() if cap else None, cap, reply.data_ptr(), src.data_ptr(),
                                          d_n.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
        assert rc == L.LNX_OK, L.lib.lnx_last_error()
        return reply.cpu().numpy(), src.cpu().numpy(), d_n.cpu().numpy().view(np.uint32)


def check(got, want, cap):
    reply, src, d_n = got
    slots, wsrc, wanted = want
    written = min(wanted, cap)
    assert d_n.tolist() == [written, wanted]
    assert len(slots) == written
    assert np.array_equal(src[:written], wsrc), np.flatnonzero(src[:written] != wsrc)[:5]
    bad = np.flatnonzero((reply[:written] != slots).any(axis=1))
    assert bad.size == 0, (bad[:5], bytes(reply[bad[0]]).hex(), bytes(slots[bad[0]]).hex())
    assert (reply[written:] == FILL).all() and (src[written:] == -1).all()   # nothing at or past d_n[0] is touched


def rec_tensor(cuda, rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 16).copy()).to(cuda)


@pytest.fixture(scope="module")
def pool():
    """509 census frames (a prime: no period shared with the chunks) in a fixed shuffle, a third of their FCSs flipped."""
    from tests import deliver_ref as D
    frames = [f for _, f in D.census_frames()]
    perm = np.random.default_rng(5).permutation(len(frames))[:509]
    bare = [frames[i] for i in perm]
    assert np.gcd(len(bare), CHUNK) == 1
    return bare, [with_fcs(f, flip=i % 3 == 1) for i, f in enumerate(bare)]


def cycled(frames, n):
    """n frames cycling through the pool, packed: (the frames, data, off) without joining n byte strings."""
    data, off = packed(frames)
    reps = -(-n // len(frames)) if n else 0
    lens = np.tile(np.diff(off), reps)[:n]
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    bdata = np.tile(data, max(reps, 1))[:max(int(boff[-1]), 1)]
    return [frames[i % len(frames)] for i in range(n)], bdata, boff


# ------------------------------------------------------------ grid boundaries
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, GRID_CAP * CHUNK + 1])
def test_behind_the_receive_check(cuda, pool, n):
    """Past cap x chunk the first 257 workgroups' slices span two chunks (the last of them one frame)."""
    bare, wire = pool
    for flags, frames, fcs in ((0, wire, True), (L.RX_NO_FCS, bare, False)):
        _, data, off = cycled(frames, n)
        stripped = [bare[i % len(bare)] for i in range(n)]
        d, o = dev(cuda, data, off)
        _, _, rec, _, _ = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | flags, filter=FILT, ports=DUP, group=False)
        ids = chain(n)
        want = expected(stripped, rec.cpu().numpy(), CFG[fcs], ids, n)
        check(run(cuda, d, o, rec, CFG[fcs], ids, n, flags), want, n)
        if n >= 256:
            assert want[2] > n // 40
            # packed frames of every length: the headers of the queueing frames start at every dword phase
            assert {int(off[i]) & 3 for i in want[1][:200]} == {0, 1, 2, 3}
    if n == 257:   # the Python entry: the chain from the stack's ipID, the counts, the slots
        reply, src, written, wanted = L.rx_rst_reply_batch(d, o, rec, CFG[False], ip_id=0x0BAD, flags=flags)
        assert (written, wanted) == (want[2], want[2]) and reply.shape == (n, 64)
        assert np.array_equal(reply[:written].cpu().numpy(), want[0])
        assert np.array_equal(src[:written].cpu().numpy(), want[1])


# ------------------------------------------------------------ densities, capacity
@pytest.fixture(scope="module")
def syns():
    """700 SYNs to closed ports with their host records (every frame queues), options on some: (frames, records)."""
    frames = [R.syn_frame((0xFFFFFF00 + i) & 0xFFFFFFFF, sport=1024 + i, dport=(9, 1000, 8080)[i % 3], opts=bytes(4 * (i % 4)),
                          payload=bytes(i % 5)) for i in range(700)]
    rec = host_records(frames, np.zeros(len(frames), dtype=np.uint8), None, FILT, DUP)
    assert ((rec["flags"] & R.DLV_RST) != 0).all()
    return frames, rec


@pytest.mark.parametrize("which", ["all", "none", 0, 63, 64, 255, 256, 699])
def test_densities(cuda, syns, which):
    """Every frame queues; none does; exactly one does: first, at a wave edge, at a chunk edge, last."""
    frames, rec = syns
    rec = rec.copy()
    if which != "all":
        keep = rec["flags"].copy()
        rec["flags"] = 0
        if which != "none":
            rec["flags"][which] = keep[which]
    d, o = dev(cuda, *packed(frames))
    ids = chain(len(frames))
    want = expected(frames, rec, CFG[True], ids, len(frames))
    assert want[2] == {"all": 700, "none": 0}.get(which, 1)
    check(run(cuda, d, o, rec_tensor(cuda, rec), CFG[True], ids, len(frames), L.RX_NO_FCS), want, len(frames))
    if which == "all":
        assert np.array_equal(want[1], np.arange(700)) and want[0][0, 42:46].tolist() == [0xFF, 0xFF, 0xFF, 0x01]


def test_capacity(cuda, pool):
    bare, _ = pool
    frames, data, off = cycled(bare, 1300)
    d, o = dev(cuda, data, off)
    _, _, rec, _, _ = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | L.RX_NO_FCS, filter=FILT, ports=DUP, group=False)
    rec_np = rec.cpu().numpy()
    wanted = expected(frames, rec_np, CFG[True], chain(1300), 1300)[2]
    assert wanted > 30
    for cap in (0, 1, wanted - 1, wanted, wanted + 7):
        ids = chain(cap)
        got = run(cuda, d, o, rec, CFG[True], ids, cap, L.RX_NO_FCS)
        check(got, expected(frames, rec_np, CFG[True], ids, cap), cap)
        assert got[2].tolist() == [min(cap, wanted), wanted]


# ------------------------------------------------------------ offsets in any order, stale records
def forced_records(n, l4_off=34):
    rec = np.zeros(n, dtype=L.DELIVERY_DTYPE)
    rec["handler"], rec["l4_off"], rec["verdict"], rec["flags"] = 0xFFFF, l4_off, 2, R.DLV_RST
    rec["src_port"], rec["dst_port"] = np.arange(n) & 0xFFFF, 443
    return rec


def test_offsets_in_any_order(cuda, pool):
    """Ranks follow the index, not the address: d_off reversed (every frame empty), shuffled (overlaps, ends below
    their starts, long frames) and with every other boundary early, under the call's own records and under
    records that flag every frame."""
    import torch
    bare, _ = pool
    data, off = packed(bare)
    d = torch.from_numpy(data).to(cuda)
    rng = np.random.default_rng(11)
    shuffled = off.copy()
    rng.shuffle(shuffled)
    near = off.copy()
    near[1::2] = np.maximum(near[1::2] - 30, 0)
    n, ids, seen = len(bare), chain(len(bare)), []
    for o_np in (off[::-1].copy(), shuffled, near):
        o = torch.from_numpy(o_np).to(cuda)
        frames = [data[o_np[i]:max(o_np[i + 1], o_np[i])].tobytes() for i in range(n)]
        _, _, rec, _, _ = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | L.RX_NO_FCS, filter=FILT, ports=DUP, group=False)
        for r in (rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1), forced_records(n)):
            want = expected(frames, r, CFG[True], ids, n)
            check(run(cuda, d, o, rec_tensor(cuda, r), CFG[True], ids, n, L.RX_NO_FCS), want, n)
            seen.append(want[2])
    assert seen[0] == seen[1] == 0 and seen[2] > 10 and seen[3] > 50 and seen[5] > 50


def test_stale_records(cuda, pool):
    """Records shifted by one frame against d_off, and records whose l4_off lies past most frames: the host loop
    on the same mismatched pairs, and no fault.  Memory safety rests on L."""
    bare, wire = pool
    d, o = dev(cuda, *packed(wire))
    _, _, rec, _, _ = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=DUP, group=False)
    rec = rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    ids = chain(len(bare))
    for r in (np.roll(rec, 1), np.roll(rec, -3), forced_records(len(bare), 70), forced_records(len(bare), 0xFFFF)):
        want = expected(bare, r, CFG[True], ids, len(bare))
        check(run(cuda, d, o, rec_tensor(cuda, r), CFG[True], ids, len(bare)), want, len(bare))
    assert want[2] == 0
    assert expected(bare, np.roll(rec, 1), CFG[True], ids, len(bare))[2] > 5


# ------------------------------------------------------------ explicit entries
@pytest.mark.parametrize("n", [1, 15, 16, 17, 64, 256, 257, 1000])
def test_explicit_entries(cuda, n):
    """Around a row of 16 and a chunk of 256 (the stage is slot_frame.hpp's, as ARP's is), with the FCS and without."""
    import torch
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 256, (n, 20), dtype=np.uint8)
    raw[n // 2, 8:16] = 0xFF                       # seq, ack all ones: the sums' carries
    ids = rng.integers(0, 1 << 16, n, dtype=np.uint16)
    d_e = torch.from_numpy(raw).to(cuda)
    d_ids = torch.from_numpy(ids.view(np.int16)).to(cuda)
    slot, ln = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    for fcs in (False, True):
        got = L.tcp_rst_frames_batch(CFG[fcs], d_e, d_ids).cpu().numpy()
        for k in range(n):
            e = L.TcpRst.from_buffer_copy(raw[k].tobytes())
            assert L.lib.lnx_tcp_rst_frame(ctypes.byref(CFG[fcs]), ctypes.byref(e), int(ids[k]), slot, ctypes.byref(ln)) == 0
            assert bytes(got[k]) == bytes(slot), (k, fcs)
            assert ln.value == (64 if fcs else 60)


# ------------------------------------------------------------ through the existing kernels, concurrency
def test_replies_pass_the_receive_check(cuda, pool):
    """The replies of one batch, packed at stride 64, through lnx_rx_verify_batch under the peer's filter."""
    import torch
    _, wire = pool
    d, o = dev(cuda, *packed(wire))
    _, _, rec, _, _ = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP, filter=FILT, ports=DUP, group=False)
    reply, src, written, wanted = L.rx_rst_reply_batch(d, o, rec, CFG[True], ip_id=77)
    assert written == wanted > 15
    peer = L.RxFilter.make(mac=R.GW_MAC)
    off = torch.arange(written + 1, dtype=torch.int64, device=cuda) * 64
    ok, v = L.rx_verify_batch(reply.view(-1), off, flags=L.VERIFY_EVIL_BIT | L.VERIFY_ICMP, filter=peer)
    assert ok.cpu().numpy().tolist() == [1] * written and v.cpu().numpy().tolist() == [0] * written


def test_two_streams_and_a_repeated_call(cuda, pool, syns):
    """Two host threads on two streams with separate workspaces, at the same time, each against its own expected
    result; a repeated call gives identical bytes."""
    import torch
    bare, _ = pool
    jobs = []
    for frames, rec, fcs in ((bare, None, True), (syns[0], syns[1], False)):
        d, o = dev(cuda, *packed(frames))
        if rec is None:
            rec = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | L.RX_NO_FCS, filter=FILT, ports=DUP, group=False)[2]
            rec = rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
        ids = chain(len(frames), seed=len(frames))
        jobs.append((d, o, rec_tensor(cuda, rec), CFG[fcs], ids, expected(frames, rec, CFG[fcs], ids, len(frames)),
                     torch.cuda.Stream(device=cuda)))
    torch.cuda.synchronize(cuda)
    results, errors = [None, None], []

    def work(j):
        try:
            d, o, rec, cfg, ids, _, stream = jobs[j]
            results[j] = [run(cuda, d, o, rec, cfg, ids, o.numel() - 1, L.RX_NO_FCS, stream) for _ in range(3)]
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for j in range(2):
        for got in results[j]:
            check(got, jobs[j][5], jobs[j][1].numel() - 1)
            assert all(np.array_equal(a, b) for a, b in zip(got, results[j][0]))
    assert jobs[0][5][2] > 20 and jobs[1][5][2] == 700
