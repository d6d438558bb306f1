"""Echo replies between the grid sizes tests/test_echo_reply_gpu.py reaches.

echo_count_kernel and echo_reply_kernel take G = min(ceil(n / 256), 1024)
workgroups, one contiguous slice of per = ceil(chunks / G) chunks each
(slice_walk.hpp), and echo_scan_kernel turns the workgroups' two sums, replies
and blocks, into bases in one scan.  The other file runs G = 1, 2 and the cap.
Here: G = 3, 64, 65, 511 and 1023, one chunk a workgroup and the last of 77
frames, with room for every reply; and for G = 65 and 511 a reply capacity and
a block capacity that end inside a middle workgroup's chunk.

Expected values come from tests/echo_ref.py, once per pool frame, and are
tiled: the batches address a pool of 61 frames n times, and reply k carries an
IP ID that depends on its pool frame alone, so that a pool frame's reply is the
same bytes wherever it stands.  The pool's replies take 1, 2, 3 and 6 blocks, so
the block sums are no multiple of the reply counts."""
import numpy as np
import pytest

import lneto_amd as L
from tests import echo_ref as E
from tests.test_deliver_gpu import dev, packed, with_fcs
from tests.test_echo_reply_gpu import CFG, check, cycled, rec_tensor, run

pytestmark = pytest.mark.gpu

CHUNK = 256               # echo_kernel.hip kEpBlock: frames per chunk
GRID_CAP = 1024           # echo_kernel.hip kEpGridCap: workgroups of the count / build launches
POOL = 61                 # the pool's frames (a prime: no period shared with the chunks)


def grid(n):
    """slice_walk.hpp slice_grid, restated."""
    return min(max(-(-n // CHUNK), 1), GRID_CAP)


def pool_id(j):
    """The IP ID of a reply to pool frame j."""
    return (0x1000 + 1031 * j) & 0xFFFF


@pytest.fixture(scope="module")
def pool():
    """61 frames and their records: echo requests whose replies take 1, 2, 3 and 6 blocks, at every byte phase once
    packed; frames under another handler's record; echo replies (type 0) under the ICMP client's record.  Per
    configuration (FCS or none), from tests/echo_ref.py once per frame: does it queue, its reply's length, its blocks
    and the first of them in `rows`, the pool's replies block by block."""
    frames, recs = [], []
    for j in range(POOL):
        kind = j % 8
        # data lengths of 1 block (d <= 18), 2 (40 .. 59), 3 (100 .. 119) and 6 blocks (300 .. 329), with an FCS or none
        d = (1 + j % 18, 9 + j % 5, 40 + j % 20, 30 + j % 7, 1 + j % 18, 9 + j % 5, 100 + j % 20, 300 + j % 30)[kind]
        f = E.echo_request(E.pattern(d, j), 0x200 + j, (0xFFF0 + j) & 0xFFFF, opts=bytes(4 * (j % 3)),
                           type_=0 if kind == 3 else 8)
        frames.append(f)
        recs.append(E.record_of(f, handler=0xFFFF) if kind in (1, 5) else E.record_of(f))
    rec = np.zeros(POOL, dtype=L.DELIVERY_DTYPE)
    for j, r in enumerate(recs):
        for k, v in r.items():
            rec[k][j] = v
    per_cfg = {}
    for fcs in (True, False):
        q, ln, nb, rows = np.zeros(POOL, dtype=bool), np.zeros(POOL, np.int64), np.zeros(POOL, np.int64), []
        for j, (f, r) in enumerate(zip(frames, recs)):
            e = E.echo_entry(f, r)
            if e is None:
                continue
            reply = E.echo_frame(E.MAC, E.GW_MAC, E.IP4, fcs, e, f[e["data_off"]:e["data_off"] + e["data_len"]], pool_id(j))
            q[j], ln[j], nb[j] = True, len(reply), -(-len(reply) // 64)
            rows.append(np.frombuffer(reply + bytes(64 * nb[j] - len(reply)), dtype=np.uint8).reshape(-1, 64))
        first = np.cumsum(nb) - nb
        assert {1, 2, 3, 6} <= set(nb[q].tolist()) and 20 < q.sum() < POOL - 15
        per_cfg[fcs] = q, ln, nb, first, np.concatenate(rows)
    assert np.gcd(POOL, CHUNK) == 1
    return frames, [with_fcs(f, flip=j % 3 == 1) for j, f in enumerate(frames)], rec, per_cfg


def tiled(per_cfg, n):
    """The n frames cycling through the pool: (src, the pool frame of each reply, its first block, its blocks)."""
    q, _, nb, _, _ = per_cfg
    src = np.flatnonzero(q[np.arange(n) % POOL])
    pj = src % POOL
    end = np.cumsum(nb[pj])
    return src, pj, end - nb[pj], nb[pj]


def tiled_expected(per_cfg, n, cap, cap_blocks):
    """tests/test_echo_reply_gpu.py expected() from the pool's replies: reply k is written iff k < cap and its last
    block lies below cap_blocks (both sums are monotone: a prefix)."""
    _, ln, _, first, rows = per_cfg
    src, pj, blk, nbk = tiled(per_cfg, n)
    wanted, blocks = len(src), int(nbk.sum())
    written = min(cap, int(np.searchsorted(blk + nbk, cap_blocks, side="right")), wanted)
    bwritten = int(blk[written - 1] + nbk[written - 1]) if written else 0
    w = slice(0, written)
    at = np.repeat(first[pj[w]] - blk[w], nbk[w]) + np.arange(bwritten)    # the pool's row of every written block
    return rows[at], 64 * blk[w], ln[pj[w]], src[w], [written, wanted, bwritten, blocks]


def ids_of(per_cfg, n):
    return np.array([pool_id(j) for j in range(POOL)], dtype=np.uint16)[tiled(per_cfg, n)[1]]


CONFIGS = ((0, True), (L.RX_NO_FCS, False))    # (call flags, replies with an FCS): frames with their FCS, and bare


@pytest.mark.parametrize("g", [3, 64, 65, 511, 1023])
def test_mid_range_grids(cuda, pool, g):
    """One chunk a workgroup, the last of 77 frames; room for every reply, then (G = 65, 511) a boundary in a
    middle workgroup: by replies, and by blocks."""
    bare, wire, pool_rec, per_cfg = pool
    n = (g - 1) * CHUNK + 77
    assert grid(n) == g and -(-n // CHUNK) == g
    rec = rec_tensor(cuda, pool_rec[np.arange(n) % POOL])
    for flags, fcs in CONFIGS:
        data, off = cycled(wire if fcs else bare, n)
        d, o = dev(cuda, data, off)
        src, pj, blk, nbk = tiled(per_cfg[fcs], n)
        ids = ids_of(per_cfg[fcs], n)
        wanted, blocks = len(src), int(nbk.sum())
        want = tiled_expected(per_cfg[fcs], n, wanted + 7, blocks + 9)
        assert want[4] == [wanted, wanted, blocks, blocks] and wanted > n // 3 and blocks % wanted != 0
        if g == 3:   # the tiled expectation is the per-frame loop of the restatement
            recs = [{k: int(pool_rec[k][i % POOL]) for k in pool_rec.dtype.names} for i in range(n)]
            out, starts, rsrc, rw, rb = E.echo_replies([bare[i % POOL] for i in range(n)], recs, E.MAC, E.GW_MAC, E.IP4, fcs, ids)
            assert (rw, rb) == (wanted, blocks) and starts == want[1].tolist() and rsrc == want[3].tolist()
            assert [len(r) for r in out] == want[2].tolist()
            assert b"".join(r + bytes(-len(r) % 64) for r in out) == want[0].tobytes()
        # every workgroup's two sums differ from some other's, and the last slice queues
        edges = np.arange(0, n, CHUNK)
        cc = np.add.reduceat(np.bincount(src, minlength=n), edges)
        bb = np.add.reduceat(np.bincount(src, weights=nbk, minlength=n).astype(np.int64), edges)
        assert len(cc) == g and len(set(cc.tolist())) > 1 and len(set(bb.tolist())) > 1 and cc[-1] > 0
        check(run(cuda, d, o, rec, CFG[fcs], ids, wanted + 7, blocks + 9, flags), want)
        if g not in (65, 511):
            continue
        mid = g // 2
        cum = np.concatenate([[0], np.cumsum(cc)])        # cum[w]: the replies before workgroup w
        k = int(cum[mid] + cc[mid] // 2)                  # a reply inside workgroup mid's chunk
        assert cum[mid] < k < cum[mid + 1] - 1
        inside = int(blk[k] + nbk[k] - 1) if nbk[k] > 1 else int(blk[k])   # a block capacity that leaves reply k out
        for cap, cap_blocks in ((k, blocks + 9), (wanted + 7, inside)):
            want = tiled_expected(per_cfg[fcs], n, cap, cap_blocks)
            assert want[4] == [k, wanted, int(blk[k]), blocks]
            check(run(cuda, d, o, rec, CFG[fcs], ids, cap, cap_blocks, flags), want)   # nothing at or past the boundary
