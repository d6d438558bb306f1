"""Every capped grid past its first pass.

Most kernels clamp their grid to a multiple of the CU count and walk the batch
with a grid-stride loop; at the batch sizes of the other tests that loop runs
once.  Here every such entry runs at n = 2 x (items in one pass) + 13: three
trips, the last one partial and no multiple of a wave's group, with inputs
arranged so that a slot holds a different case in each trip (a carry, an LDS
area, a `found` or `best` left from the trip before, or a 32-bit index would
show).  The launch rules are restated in LAUNCH below from the sources'
launchers; the comment beside each cap there names this file.

Inputs stay small: a base set of K cases (K prime, so no multiple of a pass)
with oracle results is addressed n times, through idx[i] = (A i + B) mod K for
the entries with separate start / length arrays, and by tiling the bytes on
the device for the entries whose fast paths need packed, increasing offsets.
Outputs are pre-filled with a value no expected result takes and compared on
the device by integer equality."""
import struct
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests import framegen as G

pytestmark = pytest.mark.gpu

# entry -> (items a workgroup takes per trip, workgroups per CU at the cap)
LAUNCH = {
    "search": (16 * 8, 1),          # crc32_search_o_kernel: 16 waves x 8 captures (search_kernel.hip launch_octets)
    "sum16": (4 * 4, 256),          # sum16_lines_kernel: 4 waves x 4 segments (sum16_kernel.hip)
    "ingress_rows": (4 * 4, 128),   # ingress_verify_kernel: 4 waves x 4 frames (ingress_kernel.hip)
    "tx_rows": (4 * 4, 128),        # the same kernel, GEN (launch_tx_checksum)
    "combine": (256, 8),            # combine_pairs_kernel: one lane per pair (crc32_combine_kernel.hip grid_for)
    "seed": (256, 8),               # the same kernel, lnx_crc32_update_batch's seed step
    "chain": (16, 8),               # chain_fold_kernel: sixteen 16-lane rows
}
RV_WAVES, RV_GROUP = 16, 56         # rx_verify_kernel: one workgroup per CU, 16 waves, groups of up to 56 frames
INGRESS_SHORT_MEAN, TX_SHORT_MEAN = 1280, 896  # api.cpp kIngressShortMean, kTxChecksumShortMean
K, K_LONG = 4099, 1031              # base cases (primes); K_LONG where a case is a 1.3-1.5 KB frame
A, B = 1237, 29                     # idx[i] = (A i + B) mod K


def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def per_pass(entry):
    items, wg = LAUNCH[entry]
    return items * wg * cus()


def three_trips(entry):
    return 2 * per_pass(entry) + 13


def balanced_group(n, waves, gmax):
    """rx_verify_kernel.hip balanced_group, restated."""
    rounds = ((n + gmax - 1) // gmax + waves - 1) // waves
    g = (n + waves * rounds - 1) // (waves * rounds)
    g = (g + 3) & ~3
    return min(max(g, 4), gmax), rounds


def dev(a, cuda, dtype):
    import torch
    a = np.array(a, dtype=dtype)
    view = {np.uint32: np.int32, np.uint64: np.int64, np.uint16: np.int16}.get(dtype)
    return torch.from_numpy(a.view(view) if view else a).to(cuda)


def dev_idx(n, cuda, k=K):
    import torch
    return (torch.arange(n, dtype=torch.int64, device=cuda) * A + B) % k


def sentinel_for(want, bits):
    """A value the expected results never take (asserted), as the signed torch value."""
    taken = set(int(x) for x in np.asarray(want).ravel())
    s = next(v for v in range((1 << bits) - 0x1112, 0, -1) if v not in taken)  # 0xEEEE / 0xEEEEEEEE unless taken
    assert s not in taken
    return s - (1 << bits)  # torch's signed type holds the same bits


def assert_same(got, want, what):
    import torch
    assert got.shape == want.shape and got.dtype == want.dtype, what
    if not torch.equal(got, want):
        g, w = got.reshape(-1), want.reshape(-1)
        bad = torch.nonzero(g != w).flatten()
        first = bad[:8].cpu().tolist()
        raise AssertionError((what, int(bad.numel()), [(i, int(g[i]), int(w[i])) for i in first]))


def tiled(blob, base_off, n, cuda, pad=3):
    """K packed frames (base_off[0] == 0, base_off[K] == len(blob)) repeated on the
    device until they hold n frames: (bytes, off of n + 1 entries, case of frame i)."""
    import torch
    k = len(base_off) - 1
    assert int(base_off[0]) == 0 and int(base_off[k]) == len(blob)
    reps = (n + k - 1) // k
    b = dev(np.frombuffer(blob, dtype=np.uint8), cuda, np.uint8)
    d = torch.cat([torch.full((pad,), 0xA5, dtype=torch.uint8, device=cuda), b.repeat(reps),
                   torch.zeros(8, dtype=torch.uint8, device=cuda)])
    i = torch.arange(n + 1, dtype=torch.int64, device=cuda)
    off = dev(base_off[:k], cuda, np.int64)[i % k] + (i // k) * len(blob) + pad
    return d, off, i[:n] % k


# ------------------------------------------------------------------------- search
def fcs(b):
    return struct.pack("<I", zlib.crc32(b))


def test_search_three_passes(cuda):
    """crc32_search_batch: captures of 0 to 3100 bytes, hits early, late and
    absent; a slot that ran several blocks in one pass gets a one-block capture
    with a hit in the next (its carry and `found` start afresh)."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(401)
    caps, mins = [], []
    for i in range(K):
        ln = int(rng.choice([0, 3, 40, 200, 1600, 3100]))
        cap = bytearray(rng.bytes(ln))
        kind = i % 4
        if ln >= 4 and kind != 3:
            cut = int(rng.integers(0, min(ln - 3, 30))) if kind == 0 else int(rng.integers(max(ln - 60, 0), ln - 3))
            cap[cut:cut + 4] = fcs(bytes(cap[:cut]))
        caps.append(bytes(cap))
        mins.append(int(rng.choice([0, 0, 1, ln // 2])))
    want = np.array([O.c_crc32_search(c, m) for c, m in zip(caps, mins)], dtype=np.int64)
    lens = np.array([len(c) for c in caps])
    n, pp = three_trips("search"), per_pass("search")
    i = np.arange(pp)
    fresh = (lens[i % K] > 1536) & (lens[(i + pp) % K] <= 1536) & (want[(i + pp) % K] >= 0)
    assert fresh.sum() >= pp // 50 and (want >= 0).sum() >= 1000 and (want < 0).sum() >= 1000
    base_off = np.concatenate([[0], np.cumsum(lens)])
    d, off, case = tiled(b"".join(caps), base_off, n, cuda)
    out = torch.full((n,), -7, dtype=torch.int64, device=cuda)
    assert want.min() >= -1
    got = L.crc32_search_batch(d, off, dev(mins, cuda, np.int64)[case], out=out)
    assert_same(got, dev(want, cuda, np.int64)[case], "search")


# -------------------------------------------------------------------------- sum16
def test_sum16_three_passes(cuda):
    """sum16_batch: lengths 0..80 and a few of 2000 (the slots of one wave then
    run different line counts from pass to pass), every start alignment mod 128,
    the seeds of test_sum16_random_segments among random ones."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(402)
    blob = rng.integers(0, 256, 1 << 18, dtype=np.uint8)
    lens = (np.arange(K) % 81).astype(np.uint32)
    lens[rng.integers(0, K, 12)] = 2000
    starts = (rng.integers(0, (len(blob) - 4096) // 128, K) * 128 + np.arange(K) % 128).astype(np.uint64)
    seeds = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    seeds[:4] = [0, 0xFFFFFFFF, 0xFFFF0000, 0x0001FFFE]
    want = O.sum16_segments(blob, starts, lens, seeds)
    assert len(set((starts % 128).tolist())) == 128 and (lens == 2000).sum() >= 8
    n = three_trips("sum16")
    idx = dev_idx(n, cuda)
    out = torch.full((n,), sentinel_for(want, 16), dtype=torch.int16, device=cuda)
    got = L.sum16_batch(dev(blob, cuda, np.uint8), dev(starts, cuda, np.uint64)[idx], dev(lens, cuda, np.uint32)[idx],
                        dev(seeds, cuda, np.uint32)[idx], out=out)
    assert_same(got, dev(want, cuda, np.uint16)[idx], "sum16")


# ------------------------------------------------------------------------ combine
def test_combine_three_passes(cuda):
    """crc32_combine_batch: lengths spread over all 64 bits; `out` separate and
    aliasing d_crc_a."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(403)
    a = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    b = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    k = rng.integers(0, 1 << 63, K, dtype=np.uint64) * 2 + rng.integers(0, 2, K, dtype=np.uint64)
    k >>= (np.arange(K) % 64).astype(np.uint64)
    k[:4] = np.array([0, 1, 2**64 - 1, 2**63], dtype=np.uint64)
    assert all(((k >> np.uint64(bit)) & np.uint64(1)).any() for bit in range(64))
    want = np.array([L.crc32_combine(int(x), int(y), int(z)) for x, y, z in zip(a, b, k)], dtype=np.uint32)
    n = three_trips("combine")
    idx = dev_idx(n, cuda)
    da, db, dk = dev(a, cuda, np.uint32)[idx], dev(b, cuda, np.uint32)[idx], dev(k, cuda, np.uint64)[idx]
    dw = dev(want, cuda, np.uint32)[idx]
    out = torch.full((n,), sentinel_for(want, 32), dtype=torch.int32, device=cuda)
    assert_same(L.crc32_combine_batch(da, db, dk, out=out), dw, "combine")
    alias = da.clone()
    assert L.crc32_combine_batch(alias, db, dk, out=alias) is alias
    assert_same(alias, dw, "combine, out aliasing d_crc_a")


# -------------------------------------------------------------------- update_batch
def test_update_batch_seed_step_three_passes(cuda):
    """crc32_update_batch with seeds: frames of 0..40 bytes, the seed step
    (combine_pairs_kernel in its seed form) past two passes."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(404)
    lens = np.arange(K) % 41
    base_off = np.concatenate([[0], np.cumsum(lens)])
    blob = rng.bytes(int(base_off[-1]))
    seeds = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    seeds[0::5], seeds[1::5] = 0, 0xFFFFFFFF
    want = np.array([zlib.crc32(blob[base_off[i]:base_off[i + 1]], int(seeds[i])) for i in range(K)], dtype=np.uint32)
    n = three_trips("seed")
    d, off, case = tiled(blob, base_off, n, cuda)
    out = torch.full((n,), sentinel_for(want, 32), dtype=torch.int32, device=cuda)
    got = L.crc32_update_batch(d, off, dev(seeds, cuda, np.uint32)[case], out=out)
    assert_same(got, dev(want, cuda, np.uint32)[case], "update_batch")


# -------------------------------------------------------------------------- chains
def test_chain_three_passes(cuda):
    """crc32_chain_batch and fcs_verify_chain_batch: frames of 0..5 segments, and
    one of 300 segments (the workgroup's fold, through big_* and wave_* in LDS)
    at the same workgroup slot in passes 1, 2 and 3."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(405)
    frames = []
    for i in range(K - 1):
        body = rng.bytes(int(rng.choice([0, 1, 3, 4, 7, 60, 333])))
        if i % 5 < 2:
            body += fcs(body)
        nseg = i % 6  # 0 segments: an empty frame, whatever the body
        pts = [0] + sorted(int(x) for x in rng.integers(0, len(body) + 1, max(nseg - 1, 0))) + [len(body)]
        frames.append([body[a:b] for a, b in zip(pts[:-1], pts[1:])] if nseg else [])
    big = rng.bytes(1200)
    big += fcs(big)
    frames.append([big[4 * j:4 * j + 4] for j in range(len(big) // 4)])  # 301 segments: the workgroup path
    big_case = K - 1
    assert len(frames) == K and len(frames[big_case]) > 256 and max(len(f) for f in frames[:-1]) <= 5
    assert {len(f) for f in frames[:-1]} == {0, 1, 2, 3, 4, 5}
    segs = [g for f in frames for g in f]
    nsegs_b = np.array([len(f) for f in frames], dtype=np.int64)
    first_b = np.concatenate([[0], np.cumsum(nsegs_b)])
    order, pos = rng.permutation(len(segs)), 0
    start_b, len_b = np.zeros(len(segs), dtype=np.uint64), np.array([len(g) for g in segs], dtype=np.uint32)
    for j in order:  # the segments in shuffled address order, with gaps
        pos += int(rng.integers(0, 8))
        start_b[j] = pos
        pos += len(segs[j])
    buf = rng.integers(0, 256, pos + 64, dtype=np.uint8)
    for j, g in enumerate(segs):
        buf[int(start_b[j]):int(start_b[j]) + len(g)] = np.frombuffer(g, np.uint8)
    seeds_b = rng.integers(0, 1 << 32, K, dtype=np.uint64).astype(np.uint32)
    seeds_b[0::4] = 0
    want_crc = np.array([zlib.crc32(b"".join(f), int(s)) for f, s in zip(frames, seeds_b)], dtype=np.uint32)
    want_ok = np.array([len(b"".join(f)) >= 4 and zlib.crc32(b"".join(f)) == O.CRC32_RESIDUE for f in frames],
                       dtype=np.uint8)
    assert want_ok[big_case] == 1 and 800 < want_ok.sum() < 2000
    n, pp = three_trips("chain"), per_pass("chain")
    idx = (A * np.arange(n, dtype=np.int64) + B) % K
    slot = 5
    idx[[slot, slot + pp, slot + 2 * pp]] = big_case  # block 0, row 5, trips 1, 2 and 3
    assert slot + 2 * pp < n and (idx == big_case).sum() >= 3
    counts = nsegs_b[idx]
    first = np.concatenate([[0], np.cumsum(counts)])
    seg_src = np.repeat(first_b[idx], counts) + (np.arange(first[-1]) - np.repeat(first[:-1], counts))
    args = (dev(buf, cuda, np.uint8), dev(start_b[seg_src], cuda, np.uint64), dev(len_b[seg_src], cuda, np.uint32),
            dev(first, cuda, np.uint64))
    out = torch.full((n,), sentinel_for(want_crc, 32), dtype=torch.int32, device=cuda)
    got = L.crc32_chain_batch(*args, d_seed=dev(seeds_b[idx], cuda, np.uint32), out=out)
    assert_same(got, dev(want_crc[idx], cuda, np.uint32), "chain")
    ok = L.fcs_verify_chain_batch(*args, out=torch.full((n,), 0xEE, dtype=torch.uint8, device=cuda))
    assert_same(ok, dev(want_ok[idx], cuda, np.uint8), "chain verify")


# ------------------------------------------------------------------------- ingress
def rx_frames(rng, count, lo, hi):
    """Frames of lo..hi bytes of every verdict class: valid IPv4 / IPv6 TCP and UDP,
    a corrupted payload or header byte, a total length past the buffer, bad IHL /
    total length / version fields, the evil bit, another EtherType, destinations
    the stack filter drops, Ethernet padding behind the packet."""
    out = []
    for i in range(count):
        kind = i % 13
        t = max(int(rng.integers(lo, hi + 1)), 96 if kind in (2, 3, 8) else 72)  # room for the headers
        if kind in (2, 3, 8):
            v6 = True
            l4 = G.tcp(rng.bytes(t - 74)) if kind != 3 else G.udp(rng.bytes(t - 62))
            f = G.ether(0x86DD, G.ipv6(6 if kind != 3 else 17, l4))
        elif kind == 9:
            v6 = False
            f = G.ether(int(rng.choice([0x0806, 0x88CC])), rng.bytes(t - 14))
        else:
            v6 = False
            l4 = G.udp(rng.bytes(t - 42)) if kind == 1 else G.tcp(rng.bytes(t - 54))
            dst = bytes([192, 168, 10, 77]) if kind == 10 else G.IP4_DST
            f = G.ether(0x0800, G.ipv4(17 if kind == 1 else 6, l4, flags=0x2000 if kind == 7 else 0x4000, dst=dst))
        assert len(f) == t
        b = bytearray(f)
        if kind in (4, 8):    # a payload byte
            b[int(rng.integers(t - 20, t))] ^= 1 << int(rng.integers(0, 8))
        elif kind == 5:       # an IPv4 header byte (not the length / version fields)
            b[int(rng.choice([15, 18, 19, 22, 26, 27, 30, 33]))] ^= 0x10
        elif kind == 6:       # the packet's total length is past the buffer
            b[16:18] = struct.pack(">H", t - 14 + int(rng.integers(1, 200)))
        elif kind == 11:
            m = (i // 13) % 4
            if m == 0:
                b[14] = 0x40 | int(rng.integers(0, 5))
            elif m == 1:
                b[16:18] = struct.pack(">H", int(rng.integers(0, 20)))
            elif m == 2:
                b[14] = 0x60 | (b[14] & 15)
            else:
                b[0:6] = bytes.fromhex("02aabbccddee")  # another unicast MAC
        elif kind == 12:      # padding behind the packet: the frame is longer than its total length
            pad = int(rng.integers(1, 30))
            b = bytearray(G.ether(0x0800, G.ipv4(17, G.udp(rng.bytes(t - 42 - pad))))) + bytes(pad)
        assert len(b) == t and not (v6 and kind == 5)
        out.append(bytes(b))
    return out


def ingress_case(cuda, name, count, lo, hi):
    import lneto_amd as L
    rng = np.random.default_rng(406 + lo)
    frames = rx_frames(rng, count, lo, hi)
    if name == "filtered":
        kw = dict(ip4=G.IP4_DST, ip6=G.IP6_DST)
        ofilt, cfilt = O.StackFilter(mac=G.MAC_US, **kw), L.RxFilter.make(mac=G.MAC_US, **kw)
    else:
        ofilt = cfilt = None
    want = np.array([O.ingress_verdict(f, O.VERIFY_EVIL_BIT, ofilt) for f in frames], dtype=np.uint8)
    classes = {0, O.ERR_PACKET_DROP, O.ERR_BAD_CRC, O.ERR_INVALID_FIELD, O.ERR_INVALID_LENGTH_FIELD,
               O.ERR_TRUNCATED_FRAME}
    assert set(want.tolist()) == classes and 0xEE not in classes, set(want.tolist())
    assert all((want == c).sum() >= count // 40 for c in classes - {O.ERR_INVALID_FIELD, O.ERR_INVALID_LENGTH_FIELD})
    lens = np.array([len(f) for f in frames])
    return b"".join(frames), np.concatenate([[0], np.cumsum(lens)]), want, cfilt


@pytest.mark.parametrize("name", ["plain", "filtered"])
def test_ingress_rows_three_passes(cuda, name):
    """ingress_verify_batch on 1300-1514 byte frames (the rows route: mean >=
    1280), plain and with a stack filter, every verdict class present."""
    import torch
    import lneto_amd as L
    blob, base_off, want, cfilt = ingress_case(cuda, name, K_LONG, 1300, 1514)
    n = three_trips("ingress_rows")
    d, off, case = tiled(blob, base_off, n, cuda)
    ends = off[[0, n]].cpu().tolist()
    assert ends[1] - ends[0] >= INGRESS_SHORT_MEAN * n  # the kernel's own route rule: the rows
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device=cuda)
    got = L.ingress_verify_batch(d, off, flags=L.VERIFY_EVIL_BIT, out=out, filter=cfilt)
    assert_same(got, dev(want, cuda, np.uint8)[case], "ingress rows " + name)


@pytest.mark.parametrize("name", ["plain", "filtered"])
def test_ingress_short_route_three_passes(cuda, name):
    """ingress_verify_batch on 60-200 byte frames (mean under 1280: the receive
    check without its CRC and without `ok`), past two of its passes."""
    import torch
    import lneto_amd as L
    blob, base_off, want, cfilt = ingress_case(cuda, name, K, 60, 200)
    waves = cus() * RV_WAVES
    n = 2 * waves * RV_GROUP + 13
    g, rounds = balanced_group(n, waves, RV_GROUP)
    assert rounds == 3 and n > 2 * waves * g and n % g != 0
    d, off, case = tiled(blob, base_off, n, cuda)
    ends = off[[0, n]].cpu().tolist()
    assert ends[1] - ends[0] < INGRESS_SHORT_MEAN * n  # the short route
    out = torch.full((n,), 0xEE, dtype=torch.uint8, device=cuda)
    got = L.ingress_verify_batch(d, off, flags=L.VERIFY_EVIL_BIT, out=out, filter=cfilt)
    assert_same(got, dev(want, cuda, np.uint8)[case], "ingress short route " + name)


# --------------------------------------------------------------------- tx_checksum
def tx_frames(rng, count):
    """Frames before the checksum step (stale sums and lengths), 1000-1514 bytes
    with a few short ones of each status among them."""
    out = []
    for i in range(count):
        kind = i % 12
        t = int(rng.integers(1000, 1515))
        if kind in (0, 1, 2):
            f = G.ether(0x0800, G.ipv4(6, G.tcp(rng.bytes(t - 54)), fix_l4=False))
        elif kind in (3, 4):
            f = G.ether(0x0800, G.ipv4(17, G.udp(rng.bytes(t - 42)), fix_l4=False))
        elif kind == 5:
            f = G.ether(0x86DD, G.ipv6(6, G.tcp(rng.bytes(t - 74)), fix_l4=False))
        elif kind == 6:
            f = G.ether(0x86DD, G.ipv6(17, G.udp(rng.bytes(t - 62)), fix_l4=False))
        elif kind == 7:
            f = G.ether(0x0800, G.ipv4(1, bytes([8, 0, 0, 0]) + rng.bytes(t - 38)))
        elif kind == 8:
            f = G.ether(0x86DD, G.ipv6(58, bytes([128, 0, 0, 0]) + rng.bytes(t - 58)))
        elif kind == 9:   # other EtherTypes: untouched
            f = G.ether(0x0806, rng.bytes(t - 14))
        elif kind == 10:  # transport too short for its header: ErrTruncatedFrame
            f = G.ether(0x0800, G.ipv4(6, rng.bytes(int(rng.integers(0, 20))), fix_l4=False))
        else:             # IHL below 5: ErrInvalidLengthField
            b = bytearray(G.ether(0x0800, G.ipv4(6, G.tcp(rng.bytes(t - 54)), fix_l4=False)))
            b[14] = 0x40 | int(rng.integers(0, 5))
            f = bytes(b)
        b = bytearray(f)
        if kind < 5:      # stale total length, header CRC and transport CRC
            b[16:18], b[24:26] = rng.bytes(2), rng.bytes(2)
            at = 34 + (16 if b[23] == 6 else 6)
            b[at:at + 2] = rng.bytes(2)
        out.append(bytes(b))
    return out


def test_tx_checksum_rows_three_passes(cuda):
    """tx_checksum_batch over 1536-byte slots (the generate rows: the 64 sampled
    lengths have a mean of 896 or more): the whole buffer, gaps included, and
    the status against the base image repeated."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(407)
    cap = 1536
    frames = tx_frames(rng, K_LONG)
    done = [O.tx_checksum(f) for f in frames]
    want_st = np.array([s for _, s in done], dtype=np.uint8)
    assert set(want_st.tolist()) == {0, O.ERR_TRUNCATED_FRAME, O.ERR_INVALID_LENGTH_FIELD}  # never 0xEE
    assert sum(1 for f, (g, _) in zip(frames, done) if f != g) >= K_LONG // 2
    lens = np.array([len(f) for f in frames], dtype=np.int32)
    before = np.full(K_LONG * cap, 0xA5, dtype=np.uint8)
    after = before.copy()
    for i, (f, (g, _)) in enumerate(zip(frames, done)):
        before[i * cap:i * cap + len(f)] = np.frombuffer(f, np.uint8)
        after[i * cap:i * cap + len(g)] = np.frombuffer(g, np.uint8)
    n = three_trips("tx_rows")
    sample = [(t * n) >> 6 for t in range(64)]
    assert sum(int(lens[i % K_LONG]) for i in sample) >= 64 * TX_SHORT_MEAN  # tx_gate_probe_kernel: the rows
    reps, rest = n // K_LONG, n % K_LONG
    base = dev(before, cuda, np.uint8)
    d = torch.cat([base.repeat(reps), base[:rest * cap]])
    i = torch.arange(n, dtype=torch.int64, device=cuda)
    case = i % K_LONG
    d_len = dev(lens, cuda, np.int32)[case]
    st = L.tx_checksum_batch(d, i * cap, d_len, status=torch.full((n,), 0xEE, dtype=torch.uint8, device=cuda))
    assert_same(st, dev(want_st, cuda, np.uint8)[case], "tx status")
    img = dev(after, cuda, np.uint8)
    assert_same(d[:reps * K_LONG * cap].view(reps, -1), img.expand(reps, -1), "tx bytes")
    assert_same(d[reps * K_LONG * cap:], img[:rest * cap], "tx bytes, last repeat")
    assert_same(d_len, dev(lens, cuda, np.int32)[case], "tx lengths untouched")
