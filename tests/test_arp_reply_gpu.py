"""ARP on the MI355X (lnx_rx_arp_batch, lnx_arp_frames_batch).
Expected values come from the host functions in a loop over the records the call
is given: lnx_rx_arp_entry, then lnx_arp_frame for every request for us and the
sender of every reply, in index order (tests/test_arp_reply.py pins both against
the restatement).  Slots, sources, learn records and counts must be equal byte
for byte, and nothing at or past what was written may be touched."""
import ctypes
import struct
import threading

import numpy as np
import pytest

import lneto_amd as L
from tests import arp_ref as A
from tests import deliver_ref as D
from tests import framegen as G
from tests.test_deliver_gpu import FILT, dev, host_records, packed, with_fcs

pytestmark = pytest.mark.gpu

CHUNK, GRID_CAP = 256, 512       # slot_frame.hpp: kSlotBlock frames a chunk, kSlotGridCap workgroups
FRAMES_GRID_CAP = 2048           # ... kSlotFramesGridCap workgroups of the explicit-entries launch
CFG = {fcs: L.RstCfg.make(mac=A.MAC, gw_mac=A.GW_MAC, ip4=A.IP4, fcs=fcs) for fcs in (False, True)}
FILL = 0xA5
PAD = 8                          # sentinel rows behind each capacity


# ------------------------------------------------------------ the host loop, the call, the comparison
def expected(data, off, trim, rec, cfg):
    """(slots [wanted, 64], src, seen [wanted, 16]) without capacities, from the host functions over frame i =
    data[off[i] : off[i + 1]] less its last `trim` bytes (an end below its start: empty) under rec[i]."""
    data, rec = np.ascontiguousarray(data), np.ascontiguousarray(rec)
    base, rbase = data.ctypes.data, rec.ctypes.data
    e, slot, ln = L.ArpEntry(), (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    pe, pc, pl = ctypes.byref(e), ctypes.byref(cfg), ctypes.byref(ln)
    entry_of, frame_of = L.lib.lnx_rx_arp_entry, L.lib.lnx_arp_frame
    out, src, seen = [], [], []
    for i in range(len(off) - 1):
        s = int(off[i])
        n = max(max(int(off[i + 1]) - s, 0) - trim, 0)
        rc = entry_of(base + s, n, rbase + 16 * i, pc, pe, None)
        assert rc in (0, 1, 2)
        if rc == 1:
            assert frame_of(pc, 2, pe, slot, pl) == 0
            out.append(bytes(slot))
            src.append(i)
        elif rc == 2:
            seen.append(bytes(e.hw) + b"\0\0" + bytes(e.ip) + struct.pack("<I", i))
    return (np.frombuffer(b"".join(out), dtype=np.uint8).reshape(-1, 64), np.array(src, dtype=np.int64),
            np.frombuffer(b"".join(seen), dtype=np.uint8).reshape(-1, 16))


def run(cuda, d, o, rec, cfg, cap, cap_seen, flags=0, stream=None, seen_null=False):
    """The C entry on sentinel-filled outputs of cap + PAD rows: (reply, src, seen, d_n) as numpy arrays."""
    import torch
    n = o.numel() - 1
    with torch.cuda.stream(stream or torch.cuda.current_stream(cuda)):   # the fills, the call and the copies on one stream
        reply = torch.full((cap + PAD, 64), FILL, dtype=torch.uint8, device=cuda)
        src = torch.full((cap + PAD,), -1, dtype=torch.int32, device=cuda)
        seen = torch.full((cap_seen + PAD, 16), FILL, dtype=torch.uint8, device=cuda)
        d_n = torch.full((4,), -1, dtype=torch.int32, device=cuda)
        ws = torch.full((L.rx_arp_ws_bytes(n),), FILL, dtype=torch.uint8, device=cuda)
        assert reply.data_ptr() % 64 == 0 and seen.data_ptr() % 16 == 0 and rec.data_ptr() % 16 == 0
        rc = L.lib.lnx_rx_arp_batch(d.data_ptr(), o.data_ptr(), n, flags, rec.data_ptr(), ctypes.byref(cfg), cap, cap_seen,
                                    reply.data_ptr(), src.data_ptr(), None if seen_null else seen.data_ptr(),
                                    d_n.data_ptr(), ws.data_ptr(), torch.cuda.current_stream(cuda).cuda_stream)
        assert rc == L.LNX_OK, L.lib.lnx_last_error()
        return reply.cpu().numpy(), src.cpu().numpy(), seen.cpu().numpy(), d_n.cpu().numpy().view(np.uint32)


def check(got, want, cap, cap_seen):
    reply, src, seen, d_n = got
    slots, wsrc, wseen = want
    w1, w2 = min(len(slots), cap), min(len(wseen), cap_seen)
    assert d_n.tolist() == [w1, len(slots), w2, len(wseen)]
    assert np.array_equal(src[:w1], wsrc[:w1]), np.flatnonzero(src[:w1] != wsrc[:w1])[:5]
    bad = np.flatnonzero((reply[:w1] != slots[:w1]).any(axis=1))
    assert bad.size == 0, (bad[:5], bytes(reply[bad[0]]).hex(), bytes(slots[bad[0]]).hex())
    bad = np.flatnonzero((seen[:w2] != wseen[:w2]).any(axis=1))
    assert bad.size == 0, (bad[:5], bytes(seen[bad[0]]).hex(), bytes(wseen[bad[0]]).hex())
    # nothing at or past what was written is touched
    assert (reply[w1:] == FILL).all() and (src[w1:] == -1).all() and (seen[w2:] == FILL).all()


def rec_tensor(cuda, rec):
    import torch
    return torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1, 16).copy()).to(cuda)


def forced_records(n, handler=D.H_ETH + 2, verdict=0):
    rec = np.zeros(n, dtype=L.DELIVERY_DTYPE)
    rec["handler"], rec["verdict"] = handler, verdict
    return rec


def sender(i):
    return bytes([0x02, 0x11, (i >> 16) & 255, (i >> 8) & 255, i & 255, 0x5A]), bytes([10, (i >> 16) & 255, (i >> 8) & 255, i & 255])


def request(i, pad=True, tpa=A.IP4):
    sha, spa = sender(i)
    return A.arp_eth(A.arp_body(A.OP_REQUEST, sha=sha, spa=spa, tpa=tpa), pad=pad)


def reply_frame(i):
    sha, spa = sender(i)
    return A.arp_eth(A.arp_body(A.OP_REPLY, sha=sha, spa=spa, tha=A.MAC, tpa=A.IP4 if i % 2 else A.OTHER_IP))


def invalid(i):
    return A.arp_eth(A.arp_body((0, 3, 0x0100)[i % 3] if i % 2 else A.OP_REQUEST, htype=1 if i % 2 else 2))


def non_arp(i):
    return G.ether(0x0800, G.ipv4(17, G.udp(bytes(i % 23))))


def chained(cuda, wire, flags=0):
    """The wire frames on the device with the records the receive check gives them: (d, o, rec tensor, rec numpy, data, off)."""
    data, off = packed(wire)
    d, o = dev(cuda, data, off)
    rec = L.rx_verify_deliver_batch(d, o, flags=L.VERIFY_ICMP | flags, filter=FILT, ports=None, group=False)[2]
    return d, o, rec, rec.cpu().numpy().view(L.DELIVERY_DTYPE).reshape(-1), data, off


# ------------------------------------------------------------ all requests for us: the row pass, the chunk edge
@pytest.mark.parametrize("n", [1, 15, 16, 17, 255, 256, 257, 511, 513])
def test_all_requests_for_us(cuda, n):
    """Behind the receive check itself, under both LNX_TX_FCS settings."""
    wire = [with_fcs(request(i)) for i in range(n)]
    d, o, rec, rec_np, data, off = chained(cuda, wire)
    assert (rec_np["handler"] == D.H_ETH + 2).all() and (rec_np["verdict"] == 0).all()
    for fcs in (False, True):
        want = expected(data, off, 4, rec_np, CFG[fcs])
        assert len(want[0]) == n and len(want[2]) == 0 and np.array_equal(want[1], np.arange(n))
        check(run(cuda, d, o, rec, CFG[fcs], n, n), want, n, n)
    assert want[0][0, :6].tolist() == list(sender(0)[0]) and (want[0][:, 60:] != 0).any()


# ------------------------------------------------------------ mixed batches
@pytest.fixture(scope="module")
def pool():
    """The census and every self-made case, twice over in two shuffles (3.6 k frames: fourteen chunks), a fifth of the
    FCSs flipped: (bare frames, wire frames, the cases' own records)."""
    cases = [(f, rec) for f, rec in A.census_cases()] + [(f, rec) for _, f, rec in A.self_made_cases()]
    order = np.concatenate([np.random.default_rng(s).permutation(len(cases)) for s in (5, 6)])
    bare = [cases[i][0] for i in order]
    own = np.array([tuple(cases[i][1][k] for k in ("ip_end", "handler", "l4_off", "src_port", "dst_port", "verdict", "flags",
                                                    "zero")) for i in order], dtype=L.DELIVERY_DTYPE)
    return bare, [with_fcs(f, flip=i % 5 == 1) for i, f in enumerate(bare)], own


def test_census_and_self_made_cases(cuda, pool):
    """Under the records of the device's own receive check, and under the cases' own (host and forced) records."""
    bare, wire, own = pool
    d, o, rec, rec_np, data, off = chained(cuda, wire)
    n = len(wire)
    for r_np, r in ((rec_np, rec), (own, rec_tensor(cuda, own))):
        want = expected(data, off, 4, r_np, CFG[True])
        check(run(cuda, d, o, r, CFG[True], n, n), want, n, n)
    # the cases' own records: every self-made case that queues or is learned, twice
    kinds = [k for k, _ in A.EXPECT.values()]
    assert len(want[0]) == 2 * kinds.count(1) and len(want[2]) == 2 * kinds.count(2) and kinds.count(1) >= 8
    assert {int(off[i]) & 3 for i in want[1]} == {0, 1, 2, 3}


def test_interleaved_kinds(cuda):
    """A fixed interleave of requests for us, replies, invalid ARP and non-ARP frames whose periods (7, 3, 5) share
    nothing with a wave, so the two ranks differ inside every wave; chunk 1 holds no request, chunk 2 holds 256."""
    make = {"q": request, "r": reply_frame, "x": invalid, "n": non_arp}
    pat = ["qrxnrqq"[i % 7] for i in range(CHUNK)] + ["rxn"[i % 3] for i in range(CHUNK)] + ["q"] * CHUNK + \
          ["rqxqn"[i % 5] for i in range(CHUNK + 37)]
    bare = [make[k](i) for i, k in enumerate(pat)]
    rec_np = host_records(bare, np.zeros(len(bare), dtype=np.uint8), None, FILT, None)
    data, off = packed([with_fcs(f) for f in bare])
    d, o = dev(cuda, data, off)
    want = expected(data, off, 4, rec_np, CFG[True])
    assert len(want[0]) == pat.count("q") and len(want[2]) == pat.count("r")
    n = len(bare)
    check(run(cuda, d, o, rec_tensor(cuda, rec_np), CFG[True], n, n), want, n, n)


# ------------------------------------------------------------ the grid
def numpy_batch(n):
    """n 64-byte frames from one request: i % 5 in (0, 1, 2) a request for us, 3 a reply, 4 a request for somebody
    else; every sender its own; the FCS bytes are junk, and every 11th record carries a verdict."""
    f = np.frombuffer(request(0) + b"\xde\xad\xbe\xef", dtype=np.uint8)
    data = np.tile(f, n).reshape(n, 64)
    i = np.arange(n)
    data[:, 21] = np.where(i % 5 == 3, 2, 1)
    data[:, 41] ^= (i % 5 == 4).astype(np.uint8)
    for k in range(3):
        data[:, 24 + k] = data[:, 29 + k] = (i >> (8 * (2 - k))) & 255
    rec = forced_records(n)
    rec["verdict"][::11] = 3
    return data.reshape(-1), np.arange(n + 1, dtype=np.int64) * 64, rec


@pytest.mark.parametrize("n", [CHUNK * GRID_CAP + 257, CHUNK * (GRID_CAP // 2) + 3])
def test_grid(cuda, n):
    """Past cap x chunk the first 257 workgroups' slices span two chunks and the last slices are short or empty;
    at half the cap every workgroup has one chunk and the last three frames."""
    data, off, rec_np = numpy_batch(n)
    d, o = dev(cuda, data, off)
    want = expected(data, off, 4, rec_np, CFG[True])
    assert len(want[0]) > n // 2 and len(want[2]) > n // 6
    check(run(cuda, d, o, rec_tensor(cuda, rec_np), CFG[True], n, n), want, n, n)


# ------------------------------------------------------------ capacities
def test_capacities(cuda):
    """Chunk 0 all requests, chunk 1 all replies, then alternating: a capacity of 256 ends at a chunk edge for either
    kind, 300 falls inside workgroup 2's slice, wanted - 1 inside workgroup 3's; the two vary independently."""
    pat = ["q"] * CHUNK + ["r"] * CHUNK + ["qr"[i % 2] for i in range(CHUNK + 100)]
    bare = [request(i) if k == "q" else reply_frame(i) for i, k in enumerate(pat)]
    data, off = packed(bare)
    d, o = dev(cuda, data, off)
    rec_np = forced_records(len(bare))
    rec = rec_tensor(cuda, rec_np)
    want = expected(data, off, 0, rec_np, CFG[True])
    w1, w2 = len(want[0]), len(want[2])
    assert w1 == w2 == CHUNK + (CHUNK + 100) // 2
    for cap in (0, 1, CHUNK, 300, w1 - 1, w1, w1 + 8):
        for cap_seen in (0, 1, CHUNK, 300, w2 - 1, w2, w2 + 8):
            check(run(cuda, d, o, rec, CFG[True], cap, cap_seen, L.RX_NO_FCS), want, cap, cap_seen)
        got = run(cuda, d, o, rec, CFG[True], cap, 0, L.RX_NO_FCS, seen_null=True)   # d_seen = NULL: d_n[3] still reported
        check(got, want, cap, 0)
        assert got[3].tolist() == [min(cap, w1), w1, 0, w2]


# ------------------------------------------------------------ byte phase, LNX_RX_NO_FCS
def test_byte_phases_and_no_fcs_flag(cuda):
    """Unpadded 42- and 43-byte frames (46 and 47 with their FCS) mixed with 60- and 41-byte ones: frames start at
    all four phases mod 4 and their bodies straddle 64- and 128-byte lines.  Then LNX_RX_NO_FCS against the same
    frames, which carry their FCS: the 41-byte frame, truncated without the flag, is long enough with it."""
    rng = np.random.default_rng(42)
    bare = []
    for i in range(700):
        k = int(rng.integers(0, 5))
        f = request(i, pad=False) if i % 3 else A.arp_eth(A.arp_body(A.OP_REPLY, *sender(i)), pad=False)
        bare.append((f, f + b"\x77", request(i), f[:41], reply_frame(i))[k])
    wire = [with_fcs(f) for f in bare]
    data, off = packed(wire)
    d, o = dev(cuda, data, off)
    rec_np = forced_records(len(bare))
    rec = rec_tensor(cuda, rec_np)
    n = len(bare)
    counts = []
    for flags, trim in ((0, 4), (L.RX_NO_FCS, 0)):
        want = expected(data, off, trim, rec_np, CFG[False])
        check(run(cuda, d, o, rec, CFG[False], n, n, flags), want, n, n)
        assert {int(off[i]) & 3 for i in want[1]} == {0, 1, 2, 3} and {int(off[i]) & 3 for i in want[2][:, 12:].copy().view("<u4")[:, 0]} == {0, 1, 2, 3}
        assert {(int(off[i]) + 14) // 64 != (int(off[i]) + 41) // 64 for i in want[1]} == {False, True}
        counts.append(len(want[0]) + len(want[2]))
    assert counts[1] > counts[0] + 20   # the 41-byte replies (a 41-byte request's target now ends in an FCS byte)


# ------------------------------------------------------------ offsets in any order
def test_offsets_in_any_order(cuda):
    """Ranks follow the index, not the address: d_off reversed (every frame empty) and shuffled (ends below their
    starts, overlaps, frames of many slots)."""
    import torch
    data, off, rec_np = numpy_batch(3 * CHUNK + 11)
    d = torch.from_numpy(data).to(cuda)
    rec = rec_tensor(cuda, rec_np)
    shuffled = off.copy()
    np.random.default_rng(11).shuffle(shuffled)
    n, seen = len(off) - 1, []
    for o_np in (off[::-1].copy(), shuffled):
        want = expected(data, o_np, 4, rec_np, CFG[True])
        check(run(cuda, d, torch.from_numpy(o_np).to(cuda), rec, CFG[True], n, n), want, n, n)
        seen.append(len(want[0]) + len(want[2]))
    assert seen[0] == 0 and seen[1] > 100


# ------------------------------------------------------------ explicit entries
@pytest.mark.parametrize("n", [1, 16, 17, 257, FRAMES_GRID_CAP * CHUNK // 16 + 5])
def test_explicit_entries(cuda, n):
    import torch
    rng = np.random.default_rng(n)
    raw = rng.integers(0, 256, (n, 12), dtype=np.uint8)      # (the zero field too: it is not looked at)
    raw[n // 2] = 0xFF
    ops = rng.integers(1, 3, n, dtype=np.uint16)
    assert n == 1 or {1, 2} <= set(ops.tolist())
    bad = n // 3
    if n > 1:
        ops[bad] = (0, 3, 0x0100, 0x0201)[n % 4]             # a bad op: an all-zero slot
    d_e = torch.from_numpy(raw).to(cuda)
    d_op = torch.from_numpy(ops.view(np.int16)).to(cuda)
    slot, ln = (ctypes.c_uint8 * 64)(), ctypes.c_uint32(0)
    for fcs in (False, True):
        got = L.arp_frames_batch(CFG[fcs], d_e, d_op).cpu().numpy()
        for k in range(n):
            e = L.ArpEntry.from_buffer_copy(raw[k].tobytes())
            rc = L.lib.lnx_arp_frame(ctypes.byref(CFG[fcs]), int(ops[k]), ctypes.byref(e), slot, ctypes.byref(ln))
            if n > 1 and k == bad:
                assert rc == L.LNX_EINVAL and not got[k].any()
                continue
            assert rc == 0 and ln.value == (64 if fcs else 60)
            assert bytes(got[k]) == bytes(slot), (k, fcs, int(ops[k]))


# ------------------------------------------------------------ through the existing kernels, streams, threads
def test_python_entry_and_replies_pass_the_receive_check(cuda):
    """The Python entry on a non-default stream; its replies, packed at stride 64, through lnx_fcs_verify_batch and
    lnx_rx_verify_batch under a peer's filter."""
    import torch
    peer_mac = bytes.fromhex("021122334455")
    bare = [A.arp_eth(A.arp_body(sha=peer_mac, spa=bytes([10, 0, i >> 8, i & 255]))) if i % 4 else reply_frame(i) for i in range(600)]
    d, o, rec, rec_np, data, off = chained(cuda, [with_fcs(f) for f in bare])
    want = expected(data, off, 4, rec_np, CFG[True])
    stream = torch.cuda.Stream(device=cuda)
    torch.cuda.synchronize(cuda)
    reply, src, seen, counts = L.rx_arp_batch(d, o, rec, CFG[True], stream=stream)
    assert counts == (450, 450, 150, 150) and reply.shape == (600, 64) and seen.shape == (600, 16)
    assert np.array_equal(reply[:450].cpu().numpy(), want[0]) and np.array_equal(src[:450].cpu().numpy(), want[1])
    assert np.array_equal(seen[:150].cpu().numpy(), want[2])
    s = seen[:150].cpu().numpy().view(L.ARP_SEEN_DTYPE).reshape(-1)
    assert s["src"].tolist() == list(range(0, 600, 4)) and bytes(s["hw"][1]) == sender(4)[0] and bytes(s["ip"][1]) == sender(4)[1]
    packed_off = torch.arange(451, dtype=torch.int64, device=cuda) * 64
    flat = reply[:450].contiguous().view(-1)
    assert L.fcs_verify_batch(flat, packed_off).cpu().numpy().tolist() == [1] * 450
    peer = L.RxFilter.make(mac=peer_mac, ethertypes=(0x0800, 0x0806))
    ok, v = L.rx_verify_batch(flat, packed_off, filter=peer)
    assert ok.cpu().numpy().tolist() == [1] * 450 and v.cpu().numpy().tolist() == [0] * 450
    # capacities through the Python entry
    _, _, _, counts = L.rx_arp_batch(d, o, rec, CFG[False], cap=7, cap_seen=0)
    assert counts == (7, 450, 0, 150)


def test_two_streams_and_a_repeated_call(cuda, pool):
    """Two host threads on two streams with buffers of their own, at the same time, each against its own expected
    result; a repeated call gives identical bytes."""
    import torch
    _, wire, own = pool
    jobs = []
    data, off = packed(wire)
    jobs.append((data, off, own, 4, 0, True))
    data, off, rec_np = numpy_batch(5 * CHUNK + 77)
    jobs.append((data, off, rec_np, 0, L.RX_NO_FCS, False))
    prepared = []
    for data, off, rec_np, trim, flags, fcs in jobs:
        d, o = dev(cuda, data, off)
        prepared.append((d, o, rec_tensor(cuda, rec_np), CFG[fcs], flags, expected(data, off, trim, rec_np, CFG[fcs]),
                         torch.cuda.Stream(device=cuda)))
    torch.cuda.synchronize(cuda)
    results, errors = [None, None], []

    def work(j):
        try:
            d, o, rec, cfg, flags, _, stream = prepared[j]
            n = o.numel() - 1
            results[j] = [run(cuda, d, o, rec, cfg, n, n, flags, stream) for _ in range(3)]
        except Exception as exc:   # noqa: BLE001
            errors.append(exc)

    threads = [threading.Thread(target=work, args=(j,)) for j in range(2)]
    for t in threads:
        t.start()
    for t in threads:
        t.join()
    assert not errors, errors
    for j in range(2):
        n = prepared[j][1].numel() - 1
        for got in results[j]:
            check(got, prepared[j][5], n, n)
            assert all(np.array_equal(a, b) for a, b in zip(got, results[j][0]))
    assert len(prepared[0][5][0]) > 10 and len(prepared[1][5][0]) > 500


def test_nothing_to_do(cuda):
    """n == 0: d_n zeroed and nothing else touched; both caps 0: d_n alone is written."""
    import torch
    o = torch.zeros(1, dtype=torch.int64, device=cuda)
    d = torch.zeros(1, dtype=torch.uint8, device=cuda)
    rec = torch.zeros((1, 16), dtype=torch.uint8, device=cuda)
    got = run(cuda, d, o, rec, CFG[True], 4, 4)
    assert got[3].tolist() == [0, 0, 0, 0] and (got[0] == FILL).all() and (got[1] == -1).all() and (got[2] == FILL).all()
    data, off, rec_np = numpy_batch(700)
    d, o = dev(cuda, data, off)
    want = expected(data, off, 4, rec_np, CFG[True])
    check(run(cuda, d, o, rec_tensor(cuda, rec_np), CFG[True], 0, 0), want, 0, 0)
