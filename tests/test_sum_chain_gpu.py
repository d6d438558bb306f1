"""Running internet checksums on the MI355X: lnx_sum_partial_batch (raw sums,
either byte phase, running over several calls) and lnx_sum16_chain_batch
(frames made of segments), against a restatement of lneto's crc.go:17-59 over
the concatenated bytes written here (nothing from the library): big-endian
16-bit words summed mod 2^32, an odd last byte << 8, then sum16's two folds.

The restatement comes twice: byte by byte in plain Python (ref_raw), and the
same sum over many frames at once in numpy (ref_frames: a byte at an even
offset of its frame is the high byte of its word, at an odd offset the low
one); the tests check the second against the first on their own inputs."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

M32 = 0xFFFFFFFF
# entry -> (items a workgroup takes per trip, workgroups per CU at the cap)
LAUNCH = {
    "bytes": (4 * 4, 256),  # sum_bytes_kernel: 4 waves x 4 segments (sum16_chain_kernel.hip launch_sum_bytes)
    "fold": (16 * 4, 6),    # sum_fold_kernel: sixteen 16-lane rows x 4 frames (launch_sum_fold)
}


# ---- the oracle
def ref_raw(seed, b):
    """sumWriteEven over the even part (crc.go:23-28), the odd last byte << 8 (crc.go:56)."""
    s = seed
    for i in range(0, len(b) - 1, 2):
        s = (s + ((b[i] << 8) | b[i + 1])) & M32
    if len(b) & 1:
        s = (s + (b[-1] << 8)) & M32
    return s


def ref_sum16(s):
    """sum16 (crc.go:17-21), on an array or an int."""
    s = (s & 0xFFFF) + (s >> 16)
    return ~(s + (s >> 16)) & 0xFFFF


def ref_frames(blob, start, length, seg_of, frame_of, nframes, seeds, lead=None):
    """Raw sums (uint32 values in uint64) of `nframes` frames: frame f is the
    concatenation of segments seg_of[k] (bytes blob[start : start + length]) for
    the k with frame_of[k] == f, in the order given; `lead` = bytes put in
    front of each frame that count for the offsets' parity only."""
    seg_of, frame_of = np.asarray(seg_of, dtype=np.int64), np.asarray(frame_of, dtype=np.int64)
    assert len(frame_of) == 0 or (np.diff(frame_of) >= 0).all()
    reps = np.asarray(length, dtype=np.int64)[seg_of]
    total = int(reps.sum())
    seg_byte0 = np.cumsum(reps) - reps                              # offset of each listed segment in the stream
    frame_byte0 = np.zeros(nframes + 1, dtype=np.int64)
    np.add.at(frame_byte0, frame_of + 1, reps)
    frame_byte0 = np.cumsum(frame_byte0)[:-1]                       # offset of each frame in the stream
    at = np.arange(total, dtype=np.int64)
    src = np.repeat(np.asarray(start, dtype=np.int64)[seg_of] - seg_byte0, reps) + at
    fid = np.repeat(frame_of, reps)
    j = at - frame_byte0[fid]                                       # the byte's offset in its frame
    if lead is not None:
        j = j + np.asarray(lead, dtype=np.int64)[fid]
    contrib = blob[src].astype(np.float64) * np.where(j & 1, 1.0, 256.0)
    sums = np.bincount(fid, weights=contrib, minlength=nframes)     # exact: every sum is far below 2^53
    assert sums.max(initial=0) < 2.0**52
    return (sums.astype(np.uint64) + np.asarray(seeds, dtype=np.uint64)) & np.uint64(M32)


def ref_segments(blob, start, length, seeds, phase):
    n = len(start)
    return ref_frames(blob, start, length, np.arange(n), np.arange(n), n, seeds, lead=phase)


def ref_planes(blob, start, length):
    """E and O of every segment by their definition: the bytes at even / odd offsets from the segment's start."""
    n = len(start)
    reps = np.asarray(length, dtype=np.int64)
    at = np.arange(int(reps.sum()), dtype=np.int64)
    seg0 = np.cumsum(reps) - reps
    sid = np.repeat(np.arange(n), reps)
    j = at - seg0[sid]
    b = blob[np.asarray(start, dtype=np.int64)[sid] + j].astype(np.float64)
    return (np.bincount(sid, weights=np.where(j & 1, 0.0, b), minlength=n).astype(np.uint32),
            np.bincount(sid, weights=np.where(j & 1, b, 0.0), minlength=n).astype(np.uint32))


def frames_from_first(first, nseg):
    """(seg_of, frame_of) of the C-ABI's layout: frame f = segments min(first[f], nseg) .. min(first[f+1], nseg) - 1."""
    f = np.minimum(np.asarray(first, dtype=np.int64), nseg)
    cnt = np.maximum(f[1:] - f[:-1], 0)
    frame_of = np.repeat(np.arange(len(cnt)), cnt)
    seg_of = np.repeat(f[:-1], cnt) + (np.arange(int(cnt.sum())) - np.repeat(np.cumsum(cnt) - cnt, cnt))
    return seg_of, frame_of


def spot_check(blob, start, length, first, seeds, want, rng, count=40):
    """ref_frames against the byte-by-byte restatement on some of the frames."""
    nseg = len(start)
    for f in rng.choice(len(want), min(count, len(want)), replace=False):
        a, b = min(int(first[f]), nseg), min(int(first[f + 1]), nseg)
        body = b"".join(blob[int(start[k]):int(start[k]) + int(length[k])].tobytes() for k in range(a, max(a, b)))
        assert ref_raw(int(seeds[f]), body) == int(want[f]), f


# ---- plumbing
def cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def three_trips(entry):
    items, wg = LAUNCH[entry]
    return 2 * items * wg * cus() + 13


def dev(a, cuda, dtype):
    import torch
    a = np.ascontiguousarray(np.asarray(a).astype(dtype))
    view = {np.uint32: np.int32, np.uint64: np.int64, np.uint16: np.int16}.get(dtype)
    return torch.from_numpy(a.view(view) if view else a).to(cuda)


def host(t, dtype):
    return t.cpu().numpy().view(dtype)


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want).astype(got.dtype)
    assert got.shape == want.shape, what
    bad = np.nonzero(got != want)[0]
    assert bad.size == 0, (what, int(bad.size), [(int(i), int(got[i]), int(want[i])) for i in bad[:8]])


def mixed_seeds(rng, n):
    s = rng.integers(0, 1 << 32, n, dtype=np.uint64)
    s[0::3], s[1::3] = 0, M32
    return s


# ------------------------------------------------------------------------ partial
def test_partial_every_length_shift_phase_and_seed(cuda):
    """3000 segments: every length 0..300 at each start shift of {0, 1, 2, 3, 63,
    64, 127} past a line boundary (both start parities, starts that cross a
    line), both phases mixed in one batch, seeds 0 / 0xFFFFFFFF / random;
    segments at random lines of one blob, so in shuffled order and overlapping;
    then d_phase NULL, d_seed NULL and both."""
    import lneto_amd as L
    rng = np.random.default_rng(1601)
    n = 3000
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    i = np.arange(n)
    length = i % 301
    shift = np.array([0, 1, 2, 3, 63, 64, 127])[(i // 301) % 7]
    assert len(set(zip(length[:2107].tolist(), shift[:2107].tolist()))) == 2107  # every (length, shift) pair
    start = rng.integers(0, (len(blob) - 1024) // 128, n) * 128 + shift
    phase = rng.integers(0, 256, n)  # only bit 0 counts
    seeds = mixed_seeds(rng, n)
    order = np.argsort(start, kind="stable")
    assert (np.diff(start) < 0).any() and (start[order][1:] < (start + length)[order][:-1]).any()  # shuffled, overlapping
    d = dev(blob, cuda, np.uint8)
    args = (d, dev(start, cuda, np.uint64), dev(length, cuda, np.uint32))
    d_seed, d_phase = dev(seeds, cuda, np.uint32), dev(phase, cuda, np.uint8)
    zeros = np.zeros(n, dtype=np.uint64)
    want = ref_segments(blob, start, length, seeds, phase & 1)
    for k in rng.choice(n, 60, replace=False):  # the two restatements agree: the phase as one byte in front
        seg = blob[start[k]:start[k] + length[k]].tobytes()
        lead = b"\0" * int(phase[k] & 1)
        assert ref_raw(int(seeds[k]), lead + seg) == int(want[k]), k
    same(host(L.sum_partial_batch(*args, d_seed=d_seed, d_phase=d_phase), np.uint32), want, "seeds and phases")
    same(host(L.sum_partial_batch(*args, d_seed=d_seed), np.uint32), ref_segments(blob, start, length, seeds, zeros),
         "d_phase NULL")
    same(host(L.sum_partial_batch(*args, d_phase=d_phase), np.uint32), ref_segments(blob, start, length, zeros, phase & 1),
         "d_seed NULL")
    same(host(L.sum_partial_batch(*args), np.uint32), ref_segments(blob, start, length, zeros, zeros), "both NULL")


def test_running_sum_over_two_and_three_calls(cuda):
    """A 3001-byte string summed in two and in three calls at every split of a
    small set with odd splits in it (one batch element per split), ping-ponging
    two arrays, equals one call; folded through sum16_batch with zero lengths
    it equals lnx_sum16_payload."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(1602)
    data = rng.integers(0, 256, 3001, dtype=np.uint8)
    pad = 5  # the string starts at an odd address
    d = dev(np.concatenate([np.zeros(pad, np.uint8), data, np.zeros(64, np.uint8)]), cuda, np.uint8)
    seed = 0xFFFF1234
    want = ref_raw(seed, data.tobytes())
    cuts = [0, 1, 2, 127, 128, 129, 1500, 1501, 2999, 3000, 3001]
    pairs = [(a, b) for a in cuts for b in cuts if a <= b]
    assert any(a & 1 and b & 1 for a, b in pairs) and any(a & 1 and not b & 1 for a, b in pairs)

    def call(lo, hi, d_seed, out):
        lo, hi = np.asarray(lo), np.asarray(hi)
        return L.sum_partial_batch(d, dev(lo + pad, cuda, np.uint64), dev(hi - lo, cuda, np.uint32), d_seed=d_seed,
                                   d_phase=dev(lo & 1, cuda, np.uint8), out=out)

    n2, n3 = len(cuts), len(pairs)
    ping, pong = (torch.empty(n3, dtype=torch.int32, device=cuda) for _ in range(2))
    seeds2, seeds3 = dev([seed] * n2, cuda, np.uint32), dev([seed] * n3, cuda, np.uint32)
    one = call([0], [3001], seeds2[:1], ping[:1])
    assert int(host(one, np.uint32)[0]) == want
    c = np.array(cuts)
    call(c * 0, c, seeds2, ping[:n2])
    two = call(c, c * 0 + 3001, ping[:n2], pong[:n2])
    same(host(two, np.uint32), [want] * n2, "two calls")
    a, b = np.array(pairs).T
    call(a * 0, a, seeds3, ping)
    call(a, b, ping, pong)
    three = call(b, b * 0 + 3001, pong, ping)
    same(host(three, np.uint32), [want] * n3, "three calls")
    nothing = torch.zeros(n3, dtype=torch.int32, device=cuda)
    folded = L.sum16_batch(d, nothing.to(torch.int64), nothing, d_seed=three)
    assert L.payload_sum16(seed, data.tobytes()) == ref_sum16(want)
    same(host(folded, np.uint16), [ref_sum16(want)] * n3, "Sum16 through sum16_batch")


# -------------------------------------------------------------------------- chain
def chain_case(rng, nframes, max_segs, lens, blob_bytes=1 << 20):
    """Frames of 0..max_segs segments at random places of one blob (any address
    order, overlapping), with equal and decreasing d_first pairs among them."""
    blob = rng.integers(0, 256, blob_bytes, dtype=np.uint8)
    first, cur = [0], 0
    for f in range(nframes):
        kind = f % 11
        if kind == 3:
            nxt = cur                                   # an equal pair
        elif kind == 7 and cur > 0:
            nxt = cur - int(rng.integers(1, min(cur, 50) + 1))  # a decreasing pair: no segments, the next frame starts lower
        else:
            nxt = cur + int(rng.integers(0, max_segs + 1))
        first.append(nxt)
        cur = nxt
    first = np.array(first, dtype=np.int64)
    nseg = int(first.max())
    length = rng.choice(lens, nseg)
    start = rng.integers(0, blob_bytes - int(max(lens)) - 256, nseg)
    return blob, start, length, first, nseg


def test_chain_random_frames(cuda):
    """2000 frames of 0..40 segments, lengths from {0, 1, 2, 3, 5, 64, 127, 129,
    1500}: d_out16, d_sum32 and both planes of d_seg_eo; each output alone;
    d_seed NULL."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(1603)
    nframes = 2000
    blob, start, length, first, nseg = chain_case(rng, nframes, 40, [0, 1, 2, 3, 5, 64, 127, 129, 1500])
    empty = first[1:] <= first[:-1]
    assert (first[1:] == first[:-1]).sum() > 100 and (first[1:] < first[:-1]).sum() > 100
    order = np.argsort(start, kind="stable")
    assert (np.diff(start) < 0).any() and (start[order][1:] < (start + length)[order][:-1]).any()
    seeds = mixed_seeds(rng, nframes)
    seg_of, frame_of = frames_from_first(first, nseg)
    assert np.bincount(frame_of, minlength=nframes).max() == 40 and not np.bincount(frame_of, minlength=nframes)[empty].any()
    want = ref_frames(blob, start, length, seg_of, frame_of, nframes, seeds)
    spot_check(blob, start, length, first, seeds, want, rng)
    same(want[empty], seeds[empty], "a frame with no segments is its seed")
    we, wo = ref_planes(blob, start, length)
    args = (dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32), dev(first, cuda, np.uint64))
    d_seed = dev(seeds, cuda, np.uint32)
    eo = torch.full((2 * nseg,), -0x11111112, dtype=torch.int32, device=cuda)
    o16, s32 = L.sum16_chain_batch(*args, d_seed=d_seed, out16=True, sum32=True, seg_eo=eo)
    same(host(s32, np.uint32), want, "d_sum32")
    same(host(o16, np.uint16), ref_sum16(want), "d_out16")
    same(host(eo, np.uint32)[:nseg], we, "E plane")
    same(host(eo, np.uint32)[nseg:], wo, "O plane")
    o16, none = L.sum16_chain_batch(*args, d_seed=d_seed, out16=True, sum32=False)
    assert none is None
    same(host(o16, np.uint16), ref_sum16(want), "d_out16 alone")
    none, s32 = L.sum16_chain_batch(*args, d_seed=d_seed, out16=False, sum32=True)
    assert none is None
    same(host(s32, np.uint32), want, "d_sum32 alone")
    _, s32 = L.sum16_chain_batch(*args, out16=False, sum32=True)
    same(host(s32, np.uint32), ref_frames(blob, start, length, seg_of, frame_of, nframes, np.zeros(nframes)), "d_seed NULL")
    # nseg == 0 with frames: every frame is its seed
    o16, s32 = L.sum16_chain_batch(args[0], args[1][:0], args[2][:0], args[3], d_seed=d_seed, out16=True, sum32=True)
    same(host(s32, np.uint32), seeds, "nseg == 0")
    same(host(o16, np.uint16), ref_sum16(seeds), "nseg == 0, folded")


def long_frame(rng, blob, m, lens):
    length = rng.choice(lens, m)
    start = rng.integers(0, len(blob) - int(max(lens)) - 256, m)
    return start, length


@pytest.mark.parametrize("m", [16, 17, 255, 256, 257, 1000])
def test_chain_one_long_frame(cuda, m):
    """A single frame of m segments around the row's step (16) and the row /
    workgroup threshold (256), odd lengths among them."""
    import lneto_amd as L
    rng = np.random.default_rng(1604 + m)
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    start, length = long_frame(rng, blob, m, [0, 1, 2, 3, 5, 64, 127, 129])
    assert (length & 1).sum() > m // 4
    first, seeds = np.array([0, m]), np.array([0x89ABCDEF], dtype=np.uint64)
    want = ref_frames(blob, start, length, np.arange(m), np.zeros(m, np.int64), 1, seeds)
    spot_check(blob, start, length, first, seeds, want, rng)
    o16, s32 = L.sum16_chain_batch(dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32),
                                   dev(first, cuda, np.uint64), d_seed=dev(seeds, cuda, np.uint32), out16=True, sum32=True)
    same(host(s32, np.uint32), want, "d_sum32")
    same(host(o16, np.uint16), ref_sum16(want), "d_out16")


def test_chain_70000_one_byte_segments(cuda):
    """One frame of 70 000 one-byte segments: the phase alternates every segment."""
    import lneto_amd as L
    rng = np.random.default_rng(1605)
    m = 70000
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    start, length = rng.integers(0, len(blob), m), np.ones(m, dtype=np.int64)
    first, seeds = np.array([0, m]), np.array([M32], dtype=np.uint64)
    want = ref_frames(blob, start, length, np.arange(m), np.zeros(m, np.int64), 1, seeds)
    assert ref_raw(M32, blob[start].tobytes()) == int(want[0])
    o16, s32 = L.sum16_chain_batch(dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32),
                                   dev(first, cuda, np.uint64), d_seed=dev(seeds, cuda, np.uint32), out16=True, sum32=True)
    same(host(s32, np.uint32), want, "d_sum32")
    same(host(o16, np.uint16), ref_sum16(want), "d_out16")


def test_chain_long_frame_among_short_ones(cuda):
    """A 1000-segment frame and a 300-segment one among 100 frames of 0..5
    segments: the workgroup's fold and the rows' in the same passes."""
    import lneto_amd as L
    rng = np.random.default_rng(1606)
    counts = rng.integers(0, 6, 100)
    counts[37], counts[38], counts[90] = 1000, 0, 300
    first = np.concatenate([[0], np.cumsum(counts)])
    nseg, nframes = int(first[-1]), len(counts)
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    start, length = long_frame(rng, blob, nseg, [0, 1, 2, 3, 5, 64, 127, 129])
    seeds = mixed_seeds(rng, nframes)
    seg_of, frame_of = frames_from_first(first, nseg)
    want = ref_frames(blob, start, length, seg_of, frame_of, nframes, seeds)
    spot_check(blob, start, length, first, seeds, want, rng, count=100)
    o16, s32 = L.sum16_chain_batch(dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32),
                                   dev(first, cuda, np.uint64), d_seed=dev(seeds, cuda, np.uint32), out16=True, sum32=True)
    same(host(s32, np.uint32), want, "d_sum32")
    same(host(o16, np.uint16), ref_sum16(want), "d_out16")


# --------------------------------------------------------------------------- wrap
def test_the_wrap_through_both_entries(cuda):
    """70001 + 3 + 70000 bytes of 0xFF from 0xFFFFFFF0: raw 0x1170EE7E, sum16 17
    (the unwrapped value is 0x21170EE7E: a 64-bit accumulator fails this)."""
    import torch
    import lneto_amd as L
    lens = np.array([70001, 3, 70000])
    start = np.array([3, 70100, 70200])
    blob = np.full(141000, 0xFF, dtype=np.uint8)
    assert ref_raw(0xFFFFFFF0, bytes(blob[:int(lens.sum())])) == 0x1170EE7E and ref_sum16(0x1170EE7E) == 17
    d, d_start, d_len = dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(lens, cuda, np.uint32)
    o16, s32 = L.sum16_chain_batch(d, d_start, d_len, dev([0, 3], cuda, np.uint64), d_seed=dev([0xFFFFFFF0], cuda, np.uint32),
                                   out16=True, sum32=True)
    assert int(host(s32, np.uint32)[0]) == 0x1170EE7E and int(host(o16, np.uint16)[0]) == 17
    run, pos = dev([0xFFFFFFF0], cuda, np.uint32), 0
    for k in range(3):  # a running sum, one piece per call
        run = L.sum_partial_batch(d, d_start[k:k + 1], d_len[k:k + 1], d_seed=run, d_phase=dev([pos & 1], cuda, np.uint8))
        pos += int(lens[k])
    assert int(host(run, np.uint32)[0]) == 0x1170EE7E
    zero = torch.zeros(1, dtype=torch.int32, device=cuda)
    assert int(host(L.sum16_batch(d, zero.to(torch.int64), zero, d_seed=run), np.uint16)[0]) == 17


# ------------------------------------------------------------------- capped grids
def test_partial_three_passes(cuda):
    """sum_partial_batch just past two full passes of its capped grid: tiny
    segments (0..12 bytes, a few of 300 so that a wave's rows run different line
    counts from pass to pass), outputs pre-filled with a value no result takes
    and 64 elements longer than the batch."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(1607)
    K = 4099  # base cases (a prime: no multiple of a pass), addressed idx[i] = (1237 i + 29) mod K
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    length = np.arange(K) % 13
    length[rng.integers(0, K, 12)] = 300
    start = rng.integers(0, len(blob) - 1024, K)
    phase, seeds = rng.integers(0, 2, K), mixed_seeds(rng, K)
    want = ref_segments(blob, start, length, seeds, phase)
    sentinel = next(v for v in range(0xEEEEEEEE, 0, -1) if v not in set(want.tolist()))
    n = three_trips("bytes")
    idx = (torch.arange(n, dtype=torch.int64, device=cuda) * 1237 + 29) % K
    out = torch.full((n + 64,), sentinel - (1 << 32), dtype=torch.int32, device=cuda)
    got = L.sum_partial_batch(dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64)[idx], dev(length, cuda, np.uint32)[idx],
                              d_seed=dev(seeds, cuda, np.uint32)[idx], d_phase=dev(phase, cuda, np.uint8)[idx], out=out)
    assert got is out
    assert torch.equal(out[:n], dev(want, cuda, np.uint32)[idx]), "partial, three passes"
    assert bool((out[n:] == sentinel - (1 << 32)).all()), "written past the batch"


def test_chain_three_passes(cuda):
    """sum16_chain_batch with both of its launches just past two full passes of
    their capped grids: 2 * 64 * 6 * CUs + 13 frames of 11..13 segments of 0..7
    bytes make more than 2 * 16 * 256 * CUs + 13 segments, with a frame of 300
    segments (the workgroup's fold, through its LDS areas) at the same workgroup
    slot in passes 1, 2 and 3.  Outputs and both planes pre-filled with values no result takes, the outputs 64 elements
    longer than the batch."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(1608)
    nframes = three_trips("fold")
    counts = 11 + np.arange(nframes) % 3
    pp, slot = (nframes - 13) // 2, 5
    counts[[slot, slot + pp, slot + 2 * pp]] = 300  # workgroup 0, row 5, trips 1, 2 and 3
    assert slot + 2 * pp < nframes
    first = np.concatenate([[0], np.cumsum(counts)])
    nseg = int(first[-1])
    assert nseg >= three_trips("bytes")
    blob = rng.integers(0, 256, 1 << 16, dtype=np.uint8)
    length = rng.integers(0, 8, nseg)
    start = rng.integers(0, len(blob) - 64, nseg)
    seeds = mixed_seeds(rng, nframes)
    seg_of, frame_of = frames_from_first(first, nseg)
    want = ref_frames(blob, start, length, seg_of, frame_of, nframes, seeds)
    spot_check(blob, start, length, first, seeds, want, rng)
    we, wo = ref_planes(blob, start, length)
    s16 = ref_sum16(want)
    sent32 = next(v for v in range(0xEEEEEEEE, 0, -1) if v not in set(want.tolist()))
    sent16 = next(v for v in range(0xEEEE, 0, -1) if v not in set(s16.tolist()))
    assert max(int(we.max()), int(wo.max())) < sent32
    o16 = torch.full((nframes + 64,), sent16 - (1 << 16), dtype=torch.int16, device=cuda)
    s32 = torch.full((nframes + 64,), sent32 - (1 << 32), dtype=torch.int32, device=cuda)
    eo = torch.full((2 * nseg,), sent32 - (1 << 32), dtype=torch.int32, device=cuda)
    L.sum16_chain_batch(dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32),
                        dev(first, cuda, np.uint64), d_seed=dev(seeds, cuda, np.uint32), out16=o16, sum32=s32, seg_eo=eo)
    assert torch.equal(s32[:nframes], dev(want, cuda, np.uint32)), "d_sum32, three passes"
    assert torch.equal(o16[:nframes], dev(s16, cuda, np.uint16)), "d_out16, three passes"
    assert torch.equal(eo[:nseg], dev(we, cuda, np.uint32)), "E plane, three passes"
    assert torch.equal(eo[nseg:], dev(wo, cuda, np.uint32)), "O plane, three passes"
    assert bool((s32[nframes:] == sent32 - (1 << 32)).all()) and bool((o16[nframes:] == sent16 - (1 << 16)).all())


# -------------------------------------------------------------------- repeat call
def test_each_entry_twice_on_one_stream(cuda):
    """Both entries keep nothing between calls: twice on one stream, into the
    same outputs and into fresh ones, gives the same results."""
    import torch
    import lneto_amd as L
    rng = np.random.default_rng(1609)
    nframes = 300
    blob, start, length, first, nseg = chain_case(rng, nframes, 20, [0, 1, 2, 3, 5, 64, 127, 129, 1500], 1 << 18)
    seeds = mixed_seeds(rng, nframes)
    seg_of, frame_of = frames_from_first(first, nseg)
    want = ref_frames(blob, start, length, seg_of, frame_of, nframes, seeds)
    args = (dev(blob, cuda, np.uint8), dev(start, cuda, np.uint64), dev(length, cuda, np.uint32), dev(first, cuda, np.uint64))
    d_seed = dev(seeds, cuda, np.uint32)
    stream = torch.cuda.Stream(device=cuda)
    stream.wait_stream(torch.cuda.current_stream(cuda))
    with torch.cuda.stream(stream):
        o16 = torch.zeros(nframes, dtype=torch.int16, device=cuda)
        s32 = torch.zeros(nframes, dtype=torch.int32, device=cuda)
        eo = torch.zeros(2 * nseg, dtype=torch.int32, device=cuda)
        L.sum16_chain_batch(*args, d_seed=d_seed, out16=o16, sum32=s32, seg_eo=eo, stream=stream)
        L.sum16_chain_batch(*args, d_seed=d_seed, out16=o16, sum32=s32, seg_eo=eo, stream=stream)
        o16b, s32b = L.sum16_chain_batch(*args, d_seed=d_seed, out16=True, sum32=True, stream=stream)
        pseed, pphase = dev(mixed_seeds(rng, nseg), cuda, np.uint32), dev(rng.integers(0, 2, nseg), cuda, np.uint8)
        p1 = L.sum_partial_batch(*args[:3], d_seed=pseed, d_phase=pphase, stream=stream)
        p1 = L.sum_partial_batch(*args[:3], d_seed=pseed, d_phase=pphase, out=p1, stream=stream)
        p2 = L.sum_partial_batch(*args[:3], d_seed=pseed, d_phase=pphase, stream=stream)
    stream.synchronize()
    same(host(s32, np.uint32), want, "chain, the second call into the same outputs")
    same(host(o16, np.uint16), ref_sum16(want), "chain, the second call, folded")
    assert torch.equal(s32, s32b) and torch.equal(o16, o16b)
    same(host(p1, np.uint32), ref_segments(blob, start, length, host(pseed, np.uint32), host(pphase, np.uint8)), "partial, twice")
    assert torch.equal(p1, p2)
