"""Echo replies for ICMPv4 echo requests on the MI355X (lnx_rx_echo_reply_batch,
DESIGN.md §3.20).  Expected values come from the host functions in a loop over
the records the call is given: lnx_rx_echo_entry, then
lnx_icmp_echo_reply_frame for every entry, in index order, each reply in whole
64-byte blocks (tests/test_echo_reply.py pins both against the restatement).
Blocks, starts, lengths, sources and counts must be equal byte for byte, and
nothing at or past what was written may be touched."""
import ctypes
import threading

import numpy as np
import pytest

import lneto_amd as L
from tests import echo_ref as E
from tests.test_deliver_gpu import DUP, FILT, dev, packed, with_fcs

pytestmark = pytest.mark.gpu

CHUNK, GRID_CAP, ROW_BLOCKS, WAVE_BLOCKS = 256, 1024, 2, 32   # echo_kernel.hip: kEpBlock, kEpGridCap, kEpRowBlocks, kEpWaveBlocks
CFG = {fcs: L.RstCfg.make(mac=E.MAC, gw_mac=E.GW_MAC, ip4=E.IP4, fcs=fcs) for fcs in (False, True)}
FILL = 0xA5
PAD = 8                                     # sentinel rows behind the capacities
# Data lengths d on both sides of the copy stage's steps.  A reply takes ceil(L / 64) blocks, L = max(60, 42 + d) and 4
# more with the FCS: a 16-lane row up to ROW_BLOCKS blocks (d <= 82 with the FCS, <= 86 without), then a wave, 64
# dwords a step (a second step past 256 bytes: d > 210 / 214; a third past 512: d > 466 / 470); a wave keeps a reply of
# up to WAVE_BLOCKS blocks in registers (d <= 2002 / 2006) and reads a longer one twice.
STEP_LENGTHS = (82, 83, 86, 87, 210, 211, 214, 215, 466, 467, 470, 471, 2002, 2003, 2006, 2007)


def chain(n, seed=0x0BAD):
    return np.array(L.ip4_id_chain(E.IP4[0], seed, n), dtype=np.uint16)


def expected(frames, rec, cfg, ids, cap, cap_blocks=None):
    """(blocks [blocks written, 64], start, length, src, d_n) from the host functions; rec: the records as a numpy array."""
    rec = np.ascontiguousarray(rec)
    base, e, ln = rec.ctypes.data, L.IcmpEcho(), ctypes.c_uint32(0)
    fcs = 4 if cfg.flags else 0
    out, start, length, src, wanted, blocks, written, bwritten = [], [], [], [], 0, 0, 0, 0
    for i, f in enumerate(frames):
        rc = L.lib.lnx_rx_echo_entry(f, len(f), base + 16 * i, ctypes.byref(e))
        assert rc in (0, 1)
        if rc == 1:
            n = max(60, 42 + e.data_len) + fcs
            nb = -(-n // 64)
            if wanted < cap and (cap_blocks is None or blocks + nb <= cap_blocks):
                buf = (ctypes.c_uint8 * (64 * nb))()
                assert L.lib.lnx_icmp_echo_reply_frame(ctypes.byref(cfg), ctypes.byref(e), f[e.data_off:e.data_off + e.data_len],
                                                       int(ids[wanted]), buf, n, ctypes.byref(ln)) == 0 and ln.value == n
                out.append(bytes(buf))
                start.append(64 * blocks)
                length.append(n)
                src.append(i)
                written, bwritten = written + 1, blocks + nb
            wanted += 1
            blocks += nb
    return (np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 64), np.array(start, dtype=np.int64),
            np.array(length, dtype=np.int64), np.array(src, dtype=np.int64), [written, wanted, bwritten, blocks])


def run(cuda, d, o, rec, cfg, ids, cap, cap_blocks, flags=0, stream=None):
    """The C entry on sentinel-filled outputs of PAD rows more than the capacities: numpy arrays."""
    import torch
    n = o.numel() - 1
    with torch.cuda.stream(stream or torch.cuda.current_stream(cuda)):   # the fills, the call and the copies on one stream
        reply = torch.full((cap_blocks + PAD, 64), FILL, dtype=torch.uint8, device=cuda)
        start = torch.full((cap + PAD,), -1, dtype=torch.int64, device=cuda)
        length = torch.full((cap + PAD,), -1, dtype=torch.int32, device=cuda)
        src = torch.full((cap + PAD,), -1, dtype=torch.int32, device=cuda)
        d_n = torch.full((4,), -1, dtype=torch.int32, device=cuda)
        d_ids = torch.from_numpy(np.ascontiguousarray(ids[:cap]).view(np.int16).copy()).to(cuda) if cap else None
        ws = torch.full((L.rx_echo_ws_bytes(n),), FILL, dtype=torch.uint8, device=cuda)
        assert reply.data_ptr() % 64 == 0 and ws.data_ptr() % 8 == 0
        rc = L.lib.lnx_rx_echo_reply_batch(d.data_ptr(), o.data_ptr(), n, flags, rec.data_ptr(), ctypes.byref(cfg),
                                           d_ids.data_ptr() if cap else None, cap, cap_blocks, reply.data_ptr(),
                                           start.data_ptr(), length.data_ptr(), src.data_ptr(), d_n.data_ptr(), ws.data_ptr(),
                                           torch.cuda.current_stream(cuda).cuda_stream)
        assert rc == L.LNX_OK, L.lib.lnx_last_error()
        return (reply.cpu().numpy(), start.cpu().numpy(), length.cpu().numpy(), src.cpu().numpy(),
                d_n.cpu().numpy().view(np.uint32))


def check(got, want):
    reply, start, length, src, d_n = got
    blocks, wstart, wlength, wsrc, counts = want
    written, _, bwritten, _ = counts
    assert d_n.tolist() == counts
    assert len(blocks) == bwritten and len(wsrc) == written
    assert np.array_equal(src[:written], wsrc), np.flatnonzero(src[:written] != wsrc)[:5]
    assert np.array_equal(start[:written], wstart) and np.array_equal(length[:written], wlength)
    bad = np.flatnonzero((reply[:bwritten] != blocks).any(axis=1))
    if bad.size:
        k = int(np.searchsorted(wstart, 64 * bad[0], side="right")) - 1
        assert False, (bad[:5], "reply", k, "length", int(wlength[k]), "block", int(bad[0] - wstart[k] // 64),
                       bytes(reply[bad[0]]).hex(), bytes(blocks[bad[0]]).hex())
    # nothing at or past what was written is touched
    assert (reply[bwritten:] == FILL).all() and (src[written:] == -1).all()
    assert (start[written:] == -1).all() and (length[written:] == -1).all()


def rec_tensor(cuda, rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 16).copy()).to(cuda)


def records(cuda, d, o, flags):
    return L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | flags, filter=FILT, ports=DUP, group=False)[2]


def requests():
    """Echo requests of the edge and step data lengths, some with IP options, id / seq / data varied."""
    out = []
    for k, dl in enumerate(E.EDGE_LENGTHS[:-1] + STEP_LENGTHS + (5, 33, 64, 100, 300, 777)):
        out.append(E.echo_request(E.pattern(dl, k), 0x100 + k, (0xFFF0 + k) & 0xFFFF, opts=bytes(4 * (k % 3))))
    out.append(E.echo_request(bytes(8), 0, 0))          # all zero: checksum 0xFFFF
    out.append(E.echo_request(b"\xff" * 31, 0xFFFF, 0xFFFF))
    out.append(E.echo_request(E.pattern(40), type_=0))  # an echo reply: nothing
    out.append(E.echo_request(b""))                     # no data: nothing
    return out


@pytest.fixture(scope="module")
def pool():
    """A prime number of frames (no period shared with the chunks) in a fixed shuffle: census frames mixed with echo
    requests of the edge and step lengths, a third of the FCSs flipped.  (bare, with FCS)"""
    from tests import deliver_ref as D
    census = [f for _, f in D.census_frames()]
    rng = np.random.default_rng(5)
    reqs = requests()
    frames = [census[i] for i in rng.permutation(len(census))[:251 - 2 * len(reqs)]] + reqs + reqs
    assert len(frames) == 251
    bare = [frames[i] for i in rng.permutation(len(frames))]
    assert np.gcd(len(bare), CHUNK) == 1
    return bare, [with_fcs(f, flip=i % 3 == 1) for i, f in enumerate(bare)]


def cycled(frames, n):
    """n frames cycling through the pool, packed: (data, off) without joining n byte strings."""
    data, off = packed(frames)
    reps = -(-n // len(frames)) if n else 0
    lens = np.tile(np.diff(off), reps)[:n]
    boff = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(lens, out=boff[1:])
    return np.tile(data, max(reps, 1))[:max(int(boff[-1]), 1)], boff


# ------------------------------------------------------------ grid boundaries
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257, GRID_CAP * CHUNK + 1])
def test_behind_the_receive_check(cuda, pool, n):
    """Past cap x chunk the first 257 workgroups' slices span two chunks (the last of them one frame)."""
    bare, wire = pool
    kinds = set()
    for flags, frames, fcs in ((0, wire, True), (L.RX_NO_FCS, bare, False)):
        data, off = cycled(frames, n)
        stripped = [bare[i % len(bare)] for i in range(n)]
        d, o = dev(cuda, data, off)
        rec = records(cuda, d, o, flags)
        ids = chain(n)
        want = expected(stripped, rec.cpu().numpy(), CFG[fcs], ids, n)
        check(run(cuda, d, o, rec, CFG[fcs], ids, n, want[4][3] + 3, flags), want)
        if n >= 256:
            assert want[4][1] > n // 12
            # packed frames of every length: the requests' data starts at every byte phase, and rows and waves both work
            assert {(int(off[i]) + 42) & 3 for i in want[3][:300]} == {0, 1, 2, 3}
            kinds |= set((-(-want[2] // 64)).tolist())
    if n > 256:    # rows, waves that keep the reply and waves that read it twice all work, up to their last sizes
        assert {1, ROW_BLOCKS, ROW_BLOCKS + 1, WAVE_BLOCKS, WAVE_BLOCKS + 1} <= kinds
    if n == 257:   # the Python entry: the chain from the stack's ipID, the counts, the blocks
        reply, start, length, src, written, wanted = L.rx_echo_reply_batch(d, o, rec, CFG[False], ip_id=0x0BAD, flags=flags)
        assert (written, wanted) == (want[4][0], want[4][1])
        assert np.array_equal(reply.cpu().numpy()[:want[4][2]], want[0])
        assert np.array_equal(start[:written].cpu().numpy(), want[1]) and np.array_equal(length[:written].cpu().numpy(), want[2])
        assert np.array_equal(src[:written].cpu().numpy(), want[3])


# ------------------------------------------------------------ densities, capacities
@pytest.fixture(scope="module")
def pings():
    """700 echo requests with their records (every frame queues), options on some, data 1 .. 140 bytes: (frames, records)."""
    frames = [E.echo_request(E.pattern(1 + (37 * i) % 140, i), i, 0xFFFF - i, opts=bytes(4 * (i % 4))) for i in range(700)]
    rec = np.zeros(len(frames), dtype=L.DELIVERY_DTYPE)
    for i, f in enumerate(frames):
        r = E.record_of(f)
        for k, v in r.items():
            rec[k][i] = v
    return frames, rec


@pytest.mark.parametrize("which", ["all", "none", 0, 63, 64, 255, 256, 699])
def test_densities(cuda, pings, which):
    """Every frame queues; none does; exactly one does: first, at a wave edge, at a chunk edge, last."""
    frames, rec = pings
    rec = rec.copy()
    if which != "all":
        rec["handler"] = 0xFFFF
        if which != "none":
            rec["handler"][which] = E.H_ICMP4
    d, o = dev(cuda, *packed(frames))
    ids = chain(len(frames))
    want = expected(frames, rec, CFG[True], ids, len(frames))
    assert want[4][1] == {"all": 700, "none": 0}.get(which, 1)
    check(run(cuda, d, o, rec_tensor(cuda, rec), CFG[True], ids, len(frames), want[4][3] + 1, L.RX_NO_FCS), want)


def test_capacities(cuda, pool):
    bare, _ = pool
    n = 1300
    data, off = cycled(bare, n)
    frames = [bare[i % len(bare)] for i in range(n)]
    d, o = dev(cuda, data, off)
    rec = records(cuda, d, o, L.RX_NO_FCS)
    rec_np = rec.cpu().numpy()
    full = expected(frames, rec_np, CFG[True], chain(n), n)
    wanted, blocks = full[4][1], full[4][3]
    assert wanted > 200
    for cap in (0, 1, wanted - 1, wanted, wanted + 7):
        ids = chain(cap)
        check(run(cuda, d, o, rec, CFG[True], ids, cap, blocks, L.RX_NO_FCS), expected(frames, rec_np, CFG[True], ids, cap, blocks))
    ids = chain(n)
    nb = -(-full[2] // 64)
    k = int(np.flatnonzero(nb > 4)[3])                    # a multi-block reply: cut between it and the one before, inside it,
    first = int(full[1][k]) // 64                         # and right behind it; then in the first reply of a workgroup's slice
    for cap_blocks in (0, 1, first, first + 2, first + int(nb[k]) - 1, first + int(nb[k]), blocks - 1, blocks):
        want = expected(frames, rec_np, CFG[True], ids, n, cap_blocks)
        check(run(cuda, d, o, rec, CFG[True], ids, n, cap_blocks, L.RX_NO_FCS), want)
        if first < cap_blocks < first + int(nb[k]):
            assert want[4][0] == k and want[4][2] == first   # that reply is left out whole
    at_chunk = int(np.searchsorted(full[3], 2 * CHUNK))       # the first reply of the third chunk: the boundary between two workgroups
    for cap, cap_blocks in ((at_chunk, blocks), (n, int(full[1][at_chunk]) // 64), (at_chunk + 1, int(full[1][at_chunk]) // 64)):
        check(run(cuda, d, o, rec, CFG[True], ids, cap, cap_blocks, L.RX_NO_FCS), expected(frames, rec_np, CFG[True], ids, cap, cap_blocks))


# ------------------------------------------------------------ offsets in any order, stale records
def forced_records(frames_len, l4_off=34, end=None):
    """Records that send every frame to the ICMP client, as stale or foreign records would: whatever lies at l4_off decides."""
    n = len(frames_len)
    rec = np.zeros(n, dtype=L.DELIVERY_DTYPE)
    rec["handler"], rec["l4_off"], rec["verdict"] = E.H_ICMP4, l4_off, 0
    rec["ip_end"] = frames_len if end is None else end
    return rec


def test_offsets_in_any_order(cuda, pool):
    """Ranks and blocks follow the index, not the address: d_off reversed (every frame empty), shuffled (overlaps, ends
    below their starts, long frames) and with every other boundary early, under the call's own records and under
    records that send every frame to the ICMP client."""
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
        lens = np.array([len(f) for f in frames])
        rec = records(cuda, d, o, L.RX_NO_FCS)
        for r in (rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1), forced_records(np.minimum(lens, 34 + 8 + E.MAX_DATA))):
            want = expected(frames, r, CFG[True], ids, n)
            check(run(cuda, d, o, rec_tensor(cuda, r), CFG[True], ids, n, want[4][3] + 1, L.RX_NO_FCS), want)
            seen.append(want[4][1])
    assert seen[0] == seen[1] == 0 and seen[2] > 10 and seen[3] > 5 and seen[5] > 5


def test_stale_records(cuda, pool):
    """Records shifted against d_off, records whose l4_off or ip_end lies past the frame: the host loop on the same
    mismatched pairs, and no fault.  Memory safety rests on L."""
    bare, wire = pool
    d, o = dev(cuda, *packed(wire))
    rec = records(cuda, d, o, 0).cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
    lens = np.array([len(f) for f in bare])
    ids = chain(len(bare))
    counts = []
    for r in (np.roll(rec, 1), np.roll(rec, -3), forced_records(lens), forced_records(lens, 70), forced_records(lens, end=lens + 1),
              forced_records(lens, 0xFFFF), forced_records(lens, end=np.full(len(bare), 0xFFFFFFFF, dtype=np.uint32))):
        want = expected(bare, r, CFG[True], ids, len(bare))
        check(run(cuda, d, o, rec_tensor(cuda, r), CFG[True], ids, len(bare), want[4][3] + 1), want)
        counts.append(want[4][1])
    assert counts[0] > 0 and counts[2] > 10 and counts[4] == counts[5] == counts[6] == 0


# ------------------------------------------------------------ large replies, the existing kernels, concurrency
def test_large_replies(cuda, pings):
    """A 65507-byte request (total length 65535) and a jumbo frame's 8972 bytes among short ones, at odd byte phases."""
    frames = list(pings[0][:40])
    frames[7] = E.echo_request(E.pattern(E.MAX_DATA, 9), 7, 7)
    frames[8] = E.echo_request(E.pattern(3), 8, 8)
    frames[21] = E.echo_request(E.pattern(8972, 4), 21, 21, opts=bytes(8))
    for flags, fcs in ((0, True), (L.RX_NO_FCS, False)):
        wire = [with_fcs(f) for f in frames] if fcs else frames
        d, o = dev(cuda, *packed(wire))
        rec = records(cuda, d, o, flags)
        ids = chain(len(frames))
        want = expected(frames, rec.cpu().numpy(), CFG[fcs], ids, len(frames))
        assert want[4][1] == 40 and want[2][7] == 14 + 65535 + (4 if fcs else 0)
        check(run(cuda, d, o, rec, CFG[fcs], ids, len(frames), want[4][3] + 2, flags), want)


def test_replies_pass_the_receive_check(cuda, pool):
    """The replies of one batch through lnx_crc32_segments in place (start, length) and, gathered, through
    lnx_rx_verify_batch under the peer's filter: every FCS right, every verdict 0."""
    import torch
    _, wire = pool
    d, o = dev(cuda, *packed(wire))
    rec = records(cuda, d, o, 0)
    reply, start, length, src, written, wanted = L.rx_echo_reply_batch(d, o, rec, CFG[True], ip_id=77)
    assert written == wanted > 25
    crc = L.crc32_segments(reply.view(-1), start[:written].contiguous(), length[:written].contiguous())
    assert (crc.cpu().numpy().view(np.uint32) == L.CRC32_RESIDUE).all()
    flat, s, ln = reply.view(-1).cpu().numpy(), start[:written].cpu().numpy(), length[:written].cpu().numpy()
    gathered = [flat[s[k]:s[k] + ln[k]].tobytes() for k in range(written)]
    gd, go = dev(cuda, *packed(gathered))
    peer = L.RxFilter.make(mac=E.GW_MAC)
    ok, v = L.rx_verify_batch(gd, go, flags=L.VERIFY_EVIL_BIT | L.VERIFY_ICMP, filter=peer)
    assert ok.cpu().numpy().tolist() == [1] * written and v.cpu().numpy().tolist() == [0] * written


def test_two_streams_and_a_repeated_call(cuda, pool, pings):
    """Two host threads on two streams with separate workspaces, at the same time, each against its own expected
    result; a repeated call gives identical bytes."""
    import torch
    bare, _ = pool
    jobs = []
    for frames, rec, fcs in ((bare, None, True), (pings[0], pings[1], False)):
        d, o = dev(cuda, *packed(frames))
        if rec is None:
            rec = records(cuda, d, o, L.RX_NO_FCS).cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1)
        ids = chain(len(frames), seed=len(frames))
        want = expected(frames, rec, CFG[fcs], ids, len(frames))
        jobs.append((d, o, rec_tensor(cuda, rec), CFG[fcs], ids, want, torch.cuda.Stream(device=cuda)))
    torch.cuda.synchronize(cuda)
    results, errors = [None, None], []

    def work(j):
        try:
            d, o, rec, cfg, ids, want, stream = jobs[j]
            results[j] = [run(cuda, d, o, rec, cfg, ids, o.numel() - 1, want[4][3] + 1, L.RX_NO_FCS, stream) for _ in range(3)]
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
            check(got, jobs[j][5])
            assert all(np.array_equal(a, b) for a, b in zip(got, results[j][0]))
    assert jobs[0][5][4][1] > 40 and jobs[1][5][4][1] == 700
