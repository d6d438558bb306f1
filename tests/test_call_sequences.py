"""The gated two-launch entries across call sequences and host threads.

lnx_crc32_batch / lnx_fcs_verify_batch, lnx_ingress_verify_batch and
lnx_tx_checksum_batch each launch two kernels of which one works; the second
is opened on the device by a gate word of the stream's scratch set that must
equal the call's epoch (api.cpp kStageFlag, kIngressGate, kTxChecksumGate).
The set, its giant-slice slots and its epoch counter are kept per stream and
reused by every later call, of whichever entry, on that stream.  These tests
issue calls of different kinds back to back with no host sync between them,
on one stream, on two, on more streams than the device keeps sets, and from
several host threads on one stream, and compare every call's output with the
oracle by integer equality.  Every output is pre-filled with a sentinel that
no expected value equals, so a call whose second launch nobody ran is seen."""
import ctypes
import functools
import threading
import types

import numpy as np
import pytest

import lneto_amd as L
from lneto_amd import synth
from oracle import oracle as O
from tests import framegen as G
from tests.test_ingress import _pack
from tests.test_tx_checksum import _pack_slots, tx_frames

KINDS = ["K1", "K2", "K3", "K4", "K5", "K6", "K7", "K8", "K9", "K10"]
GATED = ["K2", "K6", "K8"]      # the kinds whose first launch writes its gate word
CRC_SENTINEL = 0x5EAD5EAD       # CRC outputs (int32 tensors: below 2^31)
U8_SENTINEL = 0xEE              # verdict / ok / status outputs
INGRESS_FLAGS = 3               # LNX_VERIFY_EVIL_BIT | LNX_VERIFY_ICMP
MIB = 1 << 20


# ------------------------------------------------------------------ the kinds (CPU)
def _crc_kind(name, entry, lengths, base, seed):
    off = synth.offsets_from_lengths(np.asarray(lengths, dtype=np.int64)) + np.uint64(base)
    data = synth.bytes_np(int(off[-1]) + 8, seed=synth.SEED + seed)
    want = O.crc32_frames(data, off, threads=8)
    return types.SimpleNamespace(name=name, entry=entry, data=data, off=off, want=want, sentinel=CRC_SENTINEL)


def _zipf(n, v):
    return synth.zipf_lengths(n, seed=synth.ZIPF_SEED + v)


def _ingress_short(v):
    return G.frames(seed=91 + 10 * v, count=360) + G.icmp_frames(seed=92 + 10 * v, count=100) \
        + G.filter_frames(seed=93 + 10 * v, count=140)


def _tx_short(v):
    return [f for f in tx_frames(seed=60 + 10 * v, count=560) if len(f) < 600]


def _tx_kind(name, frames, cap):
    buf, starts, lens = _pack_slots(frames, cap, 3)
    want = [O.tx_checksum(f) for f in frames]
    img = buf.copy()
    for s, (w, _) in zip(starts, want):
        img[s:s + len(w)] = np.frombuffer(w, dtype=np.uint8)
    n = len(frames)
    return types.SimpleNamespace(name=name, entry="tx_checksum", data=buf, starts=starts, lens=lens, cap=cap,
                                 frames=frames, want=np.array([s for _, s in want], dtype=np.uint8), want_img=img,
                                 changed=sum(w != f for f, (w, _) in zip(frames, want)),
                                 sample_sum=sum(len(frames[(i * n) >> 6]) for i in range(64)), sentinel=U8_SENTINEL)


@functools.lru_cache(maxsize=None)
def kind(name, v=0):
    """The fixed input of a kind and the oracle's answer (host arrays; built
    once).  v > 0: the same kind on other data (K1, K2, K4, K6 and K8: a
    thread's, or a half's, own batch)."""
    if name == "K1":
        return _crc_kind(name, "crc32", np.full(2048, 1500), 0, 0x101 + v)
    if name == "K2":
        return _crc_kind(name, "crc32", _zipf(4096, v), 3, 0x202 + v)
    if name == "K10":
        k = _crc_kind(name, "crc32_update", _zipf(4096, v), 3, 0x202 + v)
        k.seed = np.random.default_rng(1010 + v).integers(0, 1 << 32, size=4096, dtype=np.uint64).astype(np.uint32)
        o = k.off.astype(np.int64)
        k.want = np.array([O.crc32_update(int(s), k.data[o[i]:o[i + 1]].tobytes()) for i, s in enumerate(k.seed)],
                          dtype=np.uint32)
        return k
    if name == "K3":
        lengths = np.concatenate([np.full(1024, 1500), _zipf(2048, 3)])
        k = _crc_kind(name, "fcs_verify", lengths, 0, 0x303)
        o = k.off.astype(np.int64)
        rng = np.random.default_rng(303)
        for i in range(len(lengths)):
            a, b = int(o[i]), int(o[i + 1])
            k.data[b - 4:b] = np.frombuffer(O.crc32(k.data[a:b - 4].tobytes()).to_bytes(4, "little"), dtype=np.uint8)
            if i % 3 == 0:
                k.data[a + int(rng.integers(0, b - a))] ^= np.uint8(1 << int(rng.integers(0, 8)))
        k.want = (O.crc32_frames(k.data, k.off, threads=8) == O.CRC32_RESIDUE).astype(np.uint8)
        k.sentinel = U8_SENTINEL
        return k
    if name == "K4":
        return _crc_kind(name, "crc32", np.full(8, MIB + 3), 0, 0x404 + v)
    if name == "K5":
        return _crc_kind(name, "crc32", [3 * MIB + 1, MIB, 2 * MIB + 17, 3 * MIB // 2, MIB + 5], 5, 0x505)
    if name in ("K6", "K7"):
        frames = _ingress_short(v)
        if name == "K7":  # long valid frames until the mean passes 1280 B with margin (test_gpu_ingress_both_routes)
            rng = np.random.default_rng(94)
            need = 1280 * len(frames) - sum(len(f) for f in frames)
            while need > -1280 * (len(frames) + 1):
                pay = rng.integers(0, 256, size=int(rng.integers(7000, 8900)), dtype=np.uint8).tobytes()
                f = G.ether(0x0800, G.ipv4(17, G.udp(pay))) if len(frames) % 2 else \
                    G.ether(0x86DD, G.ipv6(6, G.tcp(pay)))
                frames.append(f)
                need += 1280 - len(f)
        data, off = _pack(frames, 3)
        want = np.array([O.ingress_verdict(f, INGRESS_FLAGS) for f in frames], dtype=np.uint8)
        return types.SimpleNamespace(name=name, entry="ingress", data=data, off=off, want=want, frames=frames,
                                     sentinel=U8_SENTINEL)
    if name == "K8":
        return _tx_kind(name, _tx_short(v), 640)
    if name == "K9":
        rng = np.random.default_rng(70)
        short = _tx_short(0)
        jumbo = []
        for _ in range(len(short)):  # stale sums, as in test_gpu_tx_checksum_both_routes
            b = bytearray(G.ether(0x0800, G.ipv4(int(rng.choice([6, 17])), G.tcp(
                rng.integers(0, 256, int(rng.integers(3000, 8900)), dtype=np.uint8).tobytes()), fix_l4=False)))
            b[24:26] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes()
            jumbo.append(bytes(b))
        return _tx_kind(name, jumbo + short, 9100)
    raise KeyError(name)


def euler_walk(k=len(KINDS)):
    """A closed walk over k nodes that uses every ordered pair (loops included)
    as an edge exactly once: k * k + 1 nodes (Hierholzer)."""
    used, stack, out = [0] * k, [0], []
    while stack:
        v = stack[-1]
        if used[v] < k:
            used[v] += 1
            stack.append((v + used[v] - 1) % k)
        else:
            out.append(stack.pop())
    return out[::-1]


# dispatch.hpp restated: the kind of every workgroup slice of an offsets batch
def slice_kinds(off, num_cus):
    off = [int(x) for x in off]
    n = len(off) - 1
    grid = max(1, min(num_cus, (n + 63) // 64))
    per = (n + grid * 16 - 1) // (grid * 16) * 16
    gmean = (off[n] - off[0]) // n
    kinds = []
    for w in range(grid):
        f0, f1 = min(n, w * per), min(n, (w + 1) * per)
        if f1 <= f0:
            continue
        nf, span = f1 - f0, off[f1] - off[f0]
        if span + (off[f0] & 127) >= (1 << 31) - MIB or span >= nf * MIB or (span >= 16 * MIB and span >= nf * 8 * gmean):
            kinds.append("giant")
            continue
        idx = [lane * (nf // 64) if nf >= 64 else min(lane, nf - 1) for lane in range(64)]
        lens = [off[f0 + i + 1] - off[f0 + i] for i in idx]
        mean = span // nf
        rows = max(lens) - min(lens) <= 8 and (mean >= 960 or 176 <= mean < 576)
        kinds.append("rows" if rows else "stage")
    return kinds


def check_inputs(num_cus):
    """The conditions the table of kinds states, on a device of num_cus CUs."""
    for name in KINDS:
        k = kind(name)
        assert not (k.want == k.sentinel).any(), name
    assert set(slice_kinds(kind("K1").off, num_cus)) == {"rows"}
    assert set(slice_kinds(kind("K2").off, num_cus)) == {"stage"}
    assert set(slice_kinds(kind("K10").off, num_cus)) == {"stage"}
    assert set(slice_kinds(kind("K4").off, num_cus)) == {"giant"}
    assert set(slice_kinds(kind("K5").off, num_cus)) == {"giant"}
    if num_cus >= 48:
        assert slice_kinds(kind("K3").off, num_cus) == ["rows"] * 16 + ["stage"] * 32
    k3 = kind("K3")
    assert k3.want.tolist() == [int(i % 3 != 0) for i in range(len(k3.want))]
    for name, short in (("K6", True), ("K7", False)):
        k = kind(name)
        assert ((int(k.off[-1]) - int(k.off[0])) // len(k.frames) < 1280) == short, name
        assert len(set(k.want.tolist())) >= 4, name
    assert 550 <= len(kind("K6").frames) <= 650
    for name, short in (("K8", True), ("K9", False)):
        k = kind(name)
        assert (k.sample_sum < 64 * 896) == short, name
        assert 2 * k.changed > len(k.frames), (name, k.changed)  # "nobody ran" must not look right
        assert len(set(k.want.tolist())) >= 3, name
    assert 350 <= len(kind("K8").frames) <= 450
    for v in (1, 2, 3, 4):  # the threads' and the multi halves' own batches
        assert set(slice_kinds(kind("K2", v).off, num_cus)) == {"stage"}
        assert (int(kind("K6", v).off[-1]) - 3) // len(kind("K6", v).frames) < 1280
        assert kind("K8", v).sample_sum < 64 * 896 and 2 * kind("K8", v).changed > len(kind("K8", v).frames)
        for name in GATED:
            assert not (kind(name, v).want == kind(name, v).sentinel).any()
    for name in ("K1", "K4"):  # the multi entry's rows-only and giant halves
        assert not (kind(name, 1).want == CRC_SENTINEL).any()
    assert max(len(kind(name).data) for name in KINDS) <= 9 * MIB


def test_kinds_meet_their_input_conditions():
    """Every kind builds on the CPU and takes the route its row of the table
    names (dispatch.hpp restated, on 48 and on 256 CUs), no expected value
    equals its sentinel, the in-place kinds change most frames, and the walk
    has every ordered pair of kinds adjacent."""
    for cus in (48, 256):
        check_inputs(cus)
    w = euler_walk()
    assert len(w) == 101 and w[0] == w[-1]
    assert {(a, b) for a, b in zip(w, w[1:])} == {(a, b) for a in range(10) for b in range(10)}
    r = w[1:] + [w[1]]  # the second stream's walk: the same circuit from its second call
    assert {(a, b) for a, b in zip(r, r[1:])} == {(a, b) for a in range(10) for b in range(10)}


# ------------------------------------------------------------------ on the device
class Dev:
    """A kind's inputs and expected outputs on the device, and its calls through
    the C-ABI on caller-made outputs."""

    def __init__(self, k, cuda):
        import torch
        self.k, self.cuda = k, cuda
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).astype(dt, copy=False)).to(cuda)
        self.data = torch.from_numpy(k.data).to(cuda)
        self.tx = k.entry == "tx_checksum"
        if self.tx:
            self.starts, self.lens, self.want_img = up(k.starts, np.int64), up(k.lens, np.int32), up(k.want_img, np.uint8)
            self.n = len(k.frames)
        else:
            self.off = up(k.off, np.int64)
            self.n = len(k.off) - 1
        self.seed = up(k.seed.view(np.int32), np.int32) if k.entry == "crc32_update" else None
        self.crc = k.sentinel == CRC_SENTINEL
        self.want = up(k.want.view(np.int32), np.int32) if self.crc else up(k.want, np.uint8)

    def outputs(self):
        """One call's own output (and, in place, its working copy), not yet filled."""
        import torch
        out = torch.empty(self.n, dtype=torch.int32 if self.crc else torch.uint8, device=self.cuda)
        return (out, torch.empty_like(self.data)) if self.tx else (out, None)

    def fill(self, outs):
        """Sentinels (and the pristine bytes) on the current stream."""
        outs[0].fill_(self.k.sentinel)
        if self.tx:
            outs[1].copy_(self.data)

    def call(self, outs, stream):
        """(function, arguments) of the C-ABI call on `stream` (a hipStream_t as an integer)."""
        p, n, o = ctypes.c_void_p, self.n, outs[0].data_ptr()
        e = self.k.entry
        if e == "tx_checksum":
            return L.lib.lnx_tx_checksum_batch, (p(outs[1].data_ptr()), p(self.starts.data_ptr()),
                                                 p(self.lens.data_ptr()), n, p(o), p(stream))
        d, f = p(self.data.data_ptr()), p(self.off.data_ptr())
        if e == "ingress":
            return L.lib.lnx_ingress_verify_batch, (d, f, n, INGRESS_FLAGS, p(o), p(stream))
        if e == "crc32_update":
            return L.lib.lnx_crc32_update_batch, (d, f, n, p(self.seed.data_ptr()), p(o), p(stream))
        return (L.lib.lnx_fcs_verify_batch if e == "fcs_verify" else L.lib.lnx_crc32_batch), (d, f, n, p(o), p(stream))

    def wrong(self, outs):
        """0-d device tensor: how many output elements (and image bytes) differ."""
        w = (outs[0] != self.want).sum()
        return w + (outs[1] != self.want_img).sum() if self.tx else w

    def detail(self, outs):
        """The first wrong frames: (frame, got, want), how many hold the sentinel, and for
        the in-place kinds the first frames whose bytes are wrong."""
        got = outs[0].cpu().numpy()
        got = got.view(np.uint32) if self.crc else got
        bad = np.nonzero(got != self.k.want)[0]
        msg = {"wrong": int(bad.size), "sentinels": int((got == self.k.sentinel).sum()),
               "first": [(int(i), hex(int(got[i])), hex(int(self.k.want[i]))) for i in bad[:6]]}
        if self.tx:
            at = np.nonzero(outs[1].cpu().numpy() != self.k.want_img)[0]
            msg["byte_frames"] = sorted({int((a - 3) // self.k.cap) for a in at[:2000]})[:6]
        return msg


def _check(calls):
    """calls: (label, Dev, outs, rc) after the final synchronise.  One device
    read for all the counts, then the details of the failed calls only."""
    import torch
    assert [c[0] for c in calls if c[3] != 0] == [], "return codes"
    counts = torch.stack([d.wrong(outs) for _, d, outs, _ in calls]).cpu().numpy()
    failed = [(label, d.detail(outs)) for (label, d, outs, _), c in zip(calls, counts) if c]
    held = sum(1 for _, m in failed if m["sentinels"])
    assert not failed, f"{len(failed)} of {len(calls)} calls wrong, {held} holding sentinels; first: {failed[:4]}"


@pytest.fixture(scope="module")
def devs(cuda):
    import torch
    check_inputs(torch.cuda.get_device_properties(cuda).multi_processor_count)
    cache = {}

    def get(name, v=0):
        if (name, v) not in cache:
            cache[name, v] = Dev(kind(name, v), cuda)
        return cache[name, v]
    for name in KINDS:
        get(name)
    return get


def _walk_calls(devs, walk, tag):
    return [[f"{tag} call {i}: {KINDS[a]} after {KINDS[walk[i - 1]] if i else 'nothing'}", devs(KINDS[a]), None, None]
            for i, a in enumerate(walk)]


def _issue(c, stream):
    """Fill and call on torch's current stream `stream`; nothing waits on the host."""
    import torch
    with torch.cuda.stream(stream):
        c[1].fill(c[2])
    fn, args = c[1].call(c[2], stream.cuda_stream)
    c[3] = fn(*args)


@pytest.mark.gpu
@pytest.mark.parametrize("which", ["default", "fresh"])
def test_gpu_every_ordered_pair_adjacent_on_one_stream(cuda, devs, which):
    """The 101-call walk in which every kind follows every kind, itself too, on
    one stream with nothing waiting on the host before the last call is in:
    a stale gate word, the epoch moving between entries and the giant-slice
    slots under another piece map all leave every call exact."""
    import torch
    s = torch.cuda.default_stream(cuda) if which == "default" else torch.cuda.Stream(device=cuda)
    calls = _walk_calls(devs, euler_walk(), which)
    for c in calls:
        c[2] = c[1].outputs()
    torch.cuda.synchronize()
    for c in calls:
        _issue(c, s)
    torch.cuda.synchronize()
    _check(calls)


@pytest.mark.gpu
def test_gpu_two_streams_alternating_walks(cuda, devs):
    """The walk on two streams, call by call in turn, the second stream's walk
    one step ahead so the two sets' epochs and kinds differ at every step:
    the sets do not see each other."""
    import torch
    w = euler_walk()
    streams = [torch.cuda.Stream(device=cuda), torch.cuda.Stream(device=cuda)]
    walks = [_walk_calls(devs, w, "stream 0"), _walk_calls(devs, w[1:] + [w[1]], "stream 1")]
    for c in walks[0] + walks[1]:
        c[2] = c[1].outputs()
    torch.cuda.synchronize()
    for a, b in zip(*walks):
        _issue(a, streams[0])
        _issue(b, streams[1])
    torch.cuda.synchronize()
    _check(walks[0] + walks[1])


@pytest.mark.gpu
def test_gpu_gate_words_through_eviction(cuda, devs):
    """K6, K8 and K2 in turn on 40 fresh streams (more than the 32 sets a
    device keeps), twice round: a set made anew starts at epoch 1 on zeroed
    memory, and the first calls on it are the ones that write their gate."""
    import torch
    streams = [torch.cuda.Stream(device=cuda) for _ in range(40)]
    for rnd in range(2):
        calls = [[f"round {rnd} stream {i} {name}", devs(name), devs(name).outputs(), None]
                 for i in range(40) for name in ("K6", "K8", "K2")]
        torch.cuda.synchronize()
        for j, c in enumerate(calls):
            _issue(c, streams[j // 3])
        torch.cuda.synchronize()
        _check(calls)


def _multi(devs_pair, outs):
    import torch
    for d, o in zip(devs_pair, outs):
        d.fill(o)
    torch.cuda.synchronize()
    arr = lambda xs: (ctypes.c_void_p * 2)(*xs)
    dev = devs_pair[0].cuda.index or 0
    return L.lib.lnx_crc32_batch_multi(2, (ctypes.c_int * 2)(dev, dev), arr([d.data.data_ptr() for d in devs_pair]),
                                       arr([d.off.data_ptr() for d in devs_pair]),
                                       (ctypes.c_uint64 * 2)(*[d.n for d in devs_pair]),
                                       arr([o[0].data_ptr() for o in outs]))


@pytest.mark.gpu
def test_gpu_multi_entry_one_gpu_staged_halves(cuda, devs):
    """lnx_crc32_batch_multi(2, [0, 0]): two host threads of the library on the
    null stream of one device, each with its own 4096-frame Zipf batch (all
    staged slices: both write the stream's flag word), 50 rounds on
    sentinel-filled outputs; then a rows-only half beside a giant one."""
    import torch
    pair = [devs("K2", 1), devs("K2", 2)]
    outs = [d.outputs() for d in pair]
    failed = []
    for rnd in range(50):
        rc = _multi(pair, outs)
        assert rc == 0, (rnd, rc)
        counts = torch.stack([d.wrong(o) for d, o in zip(pair, outs)]).cpu().numpy()
        failed += [(rnd, h, d.detail(o)) for h, (d, o, c) in enumerate(zip(pair, outs, counts)) if c]
    rounds = sorted({r for r, _, _ in failed})
    assert not failed, f"{len(rounds)} of 50 rounds came back wrong (sentinels left); first: {failed[:3]}"
    pair = [devs("K1", 1), devs("K4", 1)]
    outs = [d.outputs() for d in pair]
    assert _multi(pair, outs) == 0
    _check([(f"half {h} {d.k.name}", d, o, 0) for h, (d, o) in enumerate(zip(pair, outs))])


def _threads_on_one_stream(cuda, devs, nthreads, stream, ncalls=100):
    """Each thread: ncalls C-ABI calls cycling K2, K6, K8 on its own data and
    outputs, all on `stream`; everything is prepared and synchronised before the
    threads start, and checked after the join and one synchronise."""
    import torch
    plan = []
    for t in range(nthreads):
        calls = []
        for i in range(ncalls):
            d = devs(GATED[i % 3], 1 + t)
            outs = d.outputs()
            d.fill(outs)
            calls.append([f"thread {t} call {i} {GATED[i % 3]}", d, outs, None, d.call(outs, stream)])
        plan.append(calls)
    torch.cuda.synchronize()
    go = threading.Barrier(nthreads)

    def run(calls):
        torch.cuda.set_device(cuda)
        go.wait()
        for c in calls:
            c[3] = c[4][0](*c[4][1])

    th = [threading.Thread(target=run, args=(calls,)) for calls in plan]
    for x in th:
        x.start()
    for x in th:
        x.join()
    torch.cuda.synchronize()
    _check([tuple(c[:4]) for calls in plan for c in calls])


@pytest.mark.gpu
@pytest.mark.parametrize("stream", ["explicit", "null"])
@pytest.mark.parametrize("nthreads", [2, 4])
def test_gpu_host_threads_on_one_stream(cuda, devs, nthreads, stream):
    """2 and 4 host threads, 100 calls each of the kinds that write their gate,
    all on one hipStream_t (an explicit stream, and the NULL stream): each
    call's launches reach the stream as a unit, so every output is exact."""
    import torch
    s = torch.cuda.Stream(device=cuda) if stream == "explicit" else None
    _threads_on_one_stream(cuda, devs, nthreads, s.cuda_stream if s else 0)


@pytest.mark.gpu
def test_gpu_per_thread_stream_gated_kinds(cuda, devs):
    """hipStreamPerThread from two host threads with the K2 / K6 / K8 cycle:
    the handle names a stream per thread, and each has its own set and epochs."""
    _threads_on_one_stream(cuda, devs, 2, 2)
