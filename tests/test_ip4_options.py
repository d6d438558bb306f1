"""Non-zero IPv4 options (IHL 5..15) on every verdict and transmit kernel.

lneto sums exactly 20 bytes of the IPv4 header (ipv4/frame.go:144-146) and the
transport segment starts at 14 + 4 IHL, so option bytes belong to neither sum.
The fused kernels carry code of their own for them ("IPv4
options pinned"): the
segment sum is S - [14, la) - tail with la = 14 + 4 IHL, the receive check and
tx_finish stage 72 bytes of each frame and fetch the option bytes past them
with a load of their own (qwords 9 and 10), the UDP length and ICMP type are
read at IHL-dependent offsets (dyn16, with a path through memory past the
staged bytes), and tx_finish writes a checksum that straddles the staged bytes
half into the staged copy and half directly.  With all-zero options none of
that shows: a sum over 4 IHL header bytes, a segment sum that keeps [34, la),
a load that never happens all give the right answer.

tests/framegen.py ip4_option_frames() crosses IHL 5..15, option fills that no
wrong sum survives (checked below against the oracle alone), six transports,
payload lengths on both sides of every row width and the malformations the
receive path tells apart.  Every entry runs the whole list with every frame
starting at each address residue 0..15 modulo 16 and is compared with the
oracle by integer and byte equality."""
import ctypes
import collections
import functools
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import framegen as G

import lneto_amd as L

STRIDE = 4224   # slot stride of the GPU layouts: a multiple of 16 past the longest frame (4094 B) and its FCS
CAP_SMALL = 4000  # a tx_finish capacity the 4000-byte payloads do not fit (ErrShortBuffer)
RESIDUE_GROUPS = [tuple(range(g, g + 4)) for g in range(0, 16, 4)]
INGRESS_SHORT_MEAN, TX_SHORT_MEAN = 1280, 896  # api.cpp kIngressShortMean, kTxChecksumShortMean
# (protocol, IHL, address & 7) at which tx_finish's 16-bit checksum field has its first byte in the staged
# 72 bytes and its second past them: la + 16 / la + 6 / la + 2 + (address & 7) == 71
STRADDLE_CELLS = (("tcp", 10, 1), ("tcp", 9, 5), ("udp", 12, 3), ("udp", 11, 7), ("echo", 13, 3), ("echo", 12, 7))


# ---------------------------------------------------------------- the frames
@functools.lru_cache(maxsize=None)
def matrix():
    pairs = G.ip4_option_frames()
    return tuple(n for n, _ in pairs), tuple(f for _, f in pairs)


def _filters(name):
    from tests.test_rx_filter import _pair
    return _pair(name) if name else (None, None)


@functools.lru_cache(maxsize=None)
def want_verdicts(frames, flags, filt):
    """oracle.ingress_verdict of every frame of the tuple `frames` (once per argument set)."""
    of, _ = _filters(filt)
    return np.array([O.ingress_verdict(f, flags, of) for f in frames], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def want_pcap(frames):
    return np.array([O.pcap_checksums(f) for f in frames], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def want_tx(frames):
    return tuple(O.tx_checksum(f) for f in frames)


def _fields(name):
    form, l4, ihl, fill, n, variant = name.split("/")
    return form, l4, int(ihl[3:]), fill, int(n), variant


def _report(names, got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return int(bad.size), [(int(i), names[i] if i < len(names) else "-", int(got[i]), int(want[i])) for i in bad[:10]]


# ------------------------------------------------------------------ CPU tests
def test_generator_covers_the_matrix_and_every_outcome():
    names, frames = matrix()
    assert len(set(names)) == len(names) and 10000 < len(names) <= 20000
    have = {nm: i for i, nm in enumerate(names)}
    for l4 in G.OPT_L4:
        for ihl in range(5, 16):
            for fill in G.OPT_FILLS + ("ff",):
                for n in G.OPT_LENGTHS + ((4000,) if fill == "rand" else ()):
                    f = frames[have[f"rx/{l4}/ihl{ihl}/{fill}/{n}/valid"]]
                    assert (f"tx/{l4}/ihl{ihl}/{fill}/{n}/stale" in have) == (fill != "ff")
                    la = 14 + 4 * ihl
                    assert f[14] == 0x40 | ihl and f[23] == G.OPT_PROTO[l4]
                    assert len(f) == la + {"tcp": 20, "udp": 8, "p47": 0}.get(l4, 8) + n
                    opts = f[34:la]
                    if ihl > 5:
                        assert {"rand": 0 not in opts, "ramp": 0 not in opts and len(set(opts)) > 3,
                                "first": opts[0] != 0 and not any(opts[1:]),
                                "last": opts[-1] != 0 and not any(opts[:-1]), "ff": set(opts) == {255}}[fill]
    seen = collections.defaultdict(set)
    for nm in names:
        form, l4, ihl, fill, n, variant = _fields(nm)
        seen[(form, variant)].add((l4, ihl))
    every = {(l4, ihl) for l4 in G.OPT_L4 for ihl in range(5, 16)}
    for v in ("valid", "l4flip", "ttl+l4flip", "srcflip", "ttl", "trail", "cut1", "tl=hl-1", "tl=hl", "ver5", "evil"):
        assert seen[("rx", v)] == every, v
    for v in ("optflip", "cutopt"):
        assert seen[("rx", v)] == {c for c in every if c[1] > 5}, v
    assert {c[0] for c in seen[("rx", "runt")]} == set(G.OPT_L4)
    for v in ("ulen7", "ulenP+1", "ulenP+1+ttl", "ulen_short", "csum0"):
        assert seen[("rx", v)] == {("udp", ihl) for ihl in range(5, 16)}, v
    for v in ("doff4", "doff4+ttl", "doff15"):
        assert seen[("rx", v)] == {("tcp", ihl) for ihl in range(5, 16)}, v
    assert seen[("tx", "stale")] == every
    assert seen[("tx", "zero_sum")] == {("udp", ihl) for ihl in range(5, 16)}
    assert {c[1] for c in seen[("tx", "ihl_low")]} == set(range(5))
    assert {c[1] for c in seen[("tx", "cutopt")]} == set(range(6, 16))
    assert seen[("tx", "short_l4")] == {(l4, ihl) for l4 in ("tcp", "udp", "echo") for ihl in range(5, 16)}
    # the cells where tx_finish's checksum field straddles the staged bytes: in the list, at every residue
    assert sorted(r for g in RESIDUE_GROUPS for r in g) == list(range(16))
    for l4, ihl, mis in STRADDLE_CELLS:
        at = 14 + 4 * ihl + {"tcp": 16, "udp": 6, "echo": 2}[l4]
        assert at + mis == 71 and (l4, ihl) in seen[("tx", "stale")] and (l4, ihl) in seen[("rx", "valid")]
    # every outcome
    v0, v3 = want_verdicts(frames, 0, None), want_verdicts(frames, 3, None)
    assert set(v0.tolist()) == {0, 3, 14, 15, 18} and set(v3.tolist()) == {0, 2, 3, 14, 15, 18}
    p = set(want_pcap(frames).tolist())
    assert p == {0, 1, 2, 3, 15 << 2, 18 << 2, 15 << 2 | 1, 18 << 2 | 1}, p
    t = collections.Counter(s for _, s in want_tx(frames))
    assert set(t) == {0, 15, 18} and t[15] >= 15 and t[18] >= 60
    for i, (nm, f, (g, s)) in enumerate(zip(names, frames, want_tx(frames))):
        form, l4, ihl, fill, n, variant = _fields(nm)
        if variant == "valid":
            assert v3[i] == (2 if l4 == "icmp3" else 0) and v0[i] == 0 and want_pcap(frames)[i] == 0, nm
            assert (g, s) == (f, 0), nm  # the step reproduces a valid frame
        elif variant == "stale":
            assert s == 0 and g == frames[have[f"rx/{l4}/ihl{ihl}/{fill}/{n}/valid"]], nm
        elif variant == "zero_sum":
            la = 14 + 4 * ihl
            assert s == 0 and g[la + 6:la + 8] == b"\xff\xff" and O.ingress_verdict(g) == 0, nm
        elif variant == "ihl_low":
            assert s == 15 and g == f
        elif form == "tx":
            assert s == 18 and g == f, nm


def _wrong_verdict(frame, flags, wide_header, keep_options):
    """The receive verdict of a frame that passes the size checks, by two
    deliberately wrong models: wide_header sums 4 IHL header bytes instead of
    20; keep_options leaves the option bytes [34, la) in the segment sum."""
    ip = frame[14:]
    hl, tl, proto = 4 * (ip[0] & 15), (ip[2] << 8) | ip[3], ip[9]
    c = O.CRC791()
    c.write_even(ip[:hl] if wide_header else ip[:20])
    if c.sum16() != 0:
        return O.ERR_BAD_CRC
    payload, extra = ip[hl:tl], (ip[20:hl] if keep_options else b"")
    if proto == O.IPPROTO_TCP:
        c = O.ipv4_tcp_pseudo(ip)
    elif proto == O.IPPROTO_UDP:
        c = O.ipv4_udp_pseudo(ip, (payload[4] << 8) | payload[5])
    elif proto == O.IPPROTO_ICMP and flags & O.VERIFY_ICMP:
        if payload[0] not in (0, 8):
            return O.ERR_PACKET_DROP
        c = O.CRC791()
    else:
        return 0
    c.write_even(extra)
    return O.ERR_BAD_CRC if c.payload_sum16(payload) != 0 else 0


def test_option_fills_defeat_both_wrong_sums():
    """A condition on the inputs, against the oracle alone: on every valid
    frame with options and a fill of OPT_FILLS, a header sum over 4 IHL bytes
    gives another verdict than the oracle, and so does a segment sum that keeps
    the options, wherever the reference sums a segment at all (TCP, UDP, ICMP
    echo and echo reply; protocol 47 and ICMP type 3 have no segment sum).
    Without options both models are the oracle."""
    names, frames = matrix()
    v0, v3 = want_verdicts(frames, 0, None), want_verdicts(frames, 3, None)
    checked = collections.Counter()
    for i, nm in enumerate(names):
        form, l4, ihl, fill, n, variant = _fields(nm)
        if form != "rx" or variant != "valid":
            continue
        wide, kept = _wrong_verdict(frames[i], 0, True, False), _wrong_verdict(frames[i], 3, False, True)
        assert _wrong_verdict(frames[i], 3, False, False) == v3[i], nm  # the models' frame is the oracle's
        if ihl == 5:
            assert wide == v0[i] and kept == v3[i], nm
        elif fill in G.OPT_FILLS:
            assert wide != v0[i], nm
            checked["wide", fill] += 1
            if l4 in ("tcp", "udp", "echo", "reply"):
                assert kept != v3[i], nm
                checked["kept", fill] += 1
    for fill in G.OPT_FILLS:
        assert checked["wide", fill] >= 10 * 6 * len(G.OPT_LENGTHS) and checked["kept", fill] >= 10 * 4 * len(G.OPT_LENGTHS)


def test_option_flip_changes_nothing():
    names, frames = matrix()
    pos = {nm: i for i, nm in enumerate(names)}
    count = 0
    for i, nm in enumerate(names):
        if nm.endswith("/optflip"):
            ihl, la = _fields(nm)[2], 14 + 4 * _fields(nm)[2]
            flip, cut = frames[i], frames[pos[nm[:-len("optflip")] + "cutopt"]]
            assert 34 < len(cut) < la
            # the same frame with one more option byte changed: the same answers (the untouched twin is `ttl` + TTL)
            twin = bytearray(frames[pos[nm[:-len("optflip")] + "ttl"]])
            twin[22] ^= 0x01
            twin = bytes(twin)
            diff = [k for k in range(len(twin)) if twin[k] != flip[k]]
            assert len(diff) == 1 and 34 <= diff[0] < la, nm
            for flags in range(4):
                assert O.ingress_verdict(flip, flags) == O.ingress_verdict(twin, flags) == (
                    2 if "/icmp3/" in nm and flags & 2 else 0), nm
            assert O.pcap_checksums(flip) == O.pcap_checksums(twin) == 0, nm
            count += 1
    assert count == 6 * 10 * len(G.OPT_VARIANT_LENGTHS)


def _host_verdict(frame, flags, cfilt):
    return L.lib.lnx_ingress_verdict(frame, len(frame), flags, ctypes.byref(cfilt) if cfilt is not None else None)


@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 3])
def test_host_verdicts_with_options(flags, filt):
    names, frames = matrix()
    _, cf = _filters(filt)
    nbad, bad = _report(names, [_host_verdict(f, flags, cf) for f in frames], want_verdicts(frames, flags, filt))
    assert not nbad, bad


def test_host_pcap_with_options():
    names, frames = matrix()
    nbad, bad = _report(names, [L.pcap_checksums(f) for f in frames], want_pcap(frames))
    assert not nbad, bad


def test_host_tx_checksum_then_fcs_append_with_options():
    names, frames = matrix()
    for nm, f, (want, wst) in zip(names, frames, want_tx(frames)):
        cap = max(len(f), 60) + 4
        buf = (ctypes.c_uint8 * cap).from_buffer_copy(f + b"\xa5" * (cap - len(f)))
        st = L.lib.lnx_tx_checksum(buf, len(f))
        assert st == wst and bytes(buf)[:len(f)] == want and bytes(buf)[len(f):] == b"\xa5" * (cap - len(f)), (nm, st, wst)
        ln = ctypes.c_uint32(len(f))
        st = L.lib.lnx_fcs_append(buf, ctypes.byref(ln), cap)
        fin, fst = O.fcs_append(want, cap)
        assert st == fst == 0 and ln.value == len(fin) == cap and bytes(buf) == fin, nm


# ------------------------------------------------------------------ GPU tests
# Slots of STRIDE bytes: slot i holds frame i and then non-zero bytes.  Offset-addressed entries get
# off = [s0, e0, s1, e1, ...]: the even frames are the list's, the odd ones the gaps, compared with the oracle too.
@functools.lru_cache(maxsize=None)
def slots(frames):
    """(n, STRIDE) uint8: row i = frames[i] followed by bytes 1..255 (another phase of one pool in each row)."""
    pool = np.random.default_rng(72).integers(1, 256, STRIDE + 256, dtype=np.uint8)
    base = np.empty((len(frames), STRIDE), dtype=np.uint8)
    for i, f in enumerate(frames):
        k = (i * 37) % 251
        base[i] = pool[k:k + STRIDE]
        base[i, :len(f)] = np.frombuffer(f, np.uint8)
    base.setflags(write=False)
    return base


def _lens(frames):
    return np.array([len(f) for f in frames], dtype=np.int64)


def _gaps(frames):
    base = slots(frames)
    return [base[i, len(f):].tobytes() for i, f in enumerate(frames[:-1])]


@functools.lru_cache(maxsize=None)
def want_gap_verdicts(frames, flags, filt, strip):
    of, _ = _filters(filt)
    return np.array([O.ingress_verdict(g[:len(g) - strip], flags, of) for g in _gaps(frames)], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def want_gap_pcap(frames):
    return np.array([O.pcap_checksums(g) for g in _gaps(frames)], dtype=np.uint8)


def pair_offsets(frames, empties=0):
    """off of 2 n + empties entries: frame k = entry 2 k, the gap behind it entry 2 k + 1 (k < n - 1), then
    `empties` empty entries at the last frame's end."""
    n = len(frames)
    off = np.empty(2 * n, dtype=np.int64)
    off[0::2] = np.arange(n, dtype=np.int64) * STRIDE
    off[1::2] = off[0::2] + _lens(frames)
    return np.concatenate([off, np.full(empties, off[-1], dtype=np.int64)])


def interleave(per_frame, per_gap, empties, empty_value):
    n = len(per_frame)
    out = np.empty(2 * n - 1 + empties, dtype=np.uint8)
    out[0:2 * n - 1:2] = per_frame
    out[1:2 * n - 1:2] = per_gap
    out[2 * n - 1:] = empty_value
    return out


_DEVICE = {}


@pytest.fixture(scope="module", autouse=True)
def _release_cached_images():
    """The slot images (58 MB each, host and device) go when this file's tests are done."""
    yield
    _DEVICE.clear()
    for cached in (slots, want_gap_verdicts, want_gap_pcap, want_fcs_ok, tx_sequence, want_finish, ring_subset, fcs_frames):
        cached.cache_clear()


def on_device(cuda, key, make):
    """A tensor made once per session from a host array (the unplaced slots and the expected images)."""
    import torch
    if key not in _DEVICE:
        _DEVICE[key] = torch.from_numpy(np.array(make())).to(cuda)  # (a copy: the cached host arrays are read-only)
    return _DEVICE[key]


def place(image, residue):
    """A fresh copy of the 1-D device tensor `image` whose first byte lies at `residue` modulo 16."""
    import torch
    buf = torch.empty(image.numel() + 32, dtype=torch.uint8, device=image.device)
    pad = (residue - buf.data_ptr()) % 16
    d = buf[pad:pad + image.numel()]
    d.copy_(image)
    assert d.data_ptr() % 16 == residue and d.is_contiguous()
    return d


def _dev(cuda, a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _flat(cuda, key, frames):
    return on_device(cuda, ("slots", key), lambda: slots(frames).reshape(-1))


def _entry_names(names, count):
    return [names[i // 2] if i % 2 == 0 and i // 2 < len(names) else "gap/empty" for i in range(count)]


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
@pytest.mark.parametrize("route", ["rows", "short"])
@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_gpu_ingress_verify_with_options(cuda, flags, filt, route, residues):
    """lnx_ingress_verify_batch on both routes: the slot stride makes the mean
    entry 2112 B (the ingress rows); 2 n empty entries after the list bring it
    under 1280 B (the receive check without its CRC)."""
    names, frames = matrix()
    n = len(frames)
    empties = 2 * n if route == "short" else 0
    off = pair_offsets(frames, empties)
    ne = len(off) - 1
    assert (int(off[ne] - off[0]) >= INGRESS_SHORT_MEAN * ne) == (route == "rows")  # the kernel's own route rule
    want = interleave(want_verdicts(frames, flags, filt), want_gap_verdicts(frames, flags, filt, 0), empties,
                      O.ERR_TRUNCATED_FRAME)
    _, cf = _filters(filt)
    image, o = _flat(cuda, "rx", frames), _dev(cuda, off)
    for r in residues:
        got = L.ingress_verify_batch(place(image, r), o, flags=flags, filter=cf).cpu().numpy()
        nbad, bad = _report(_entry_names(names, ne), got, want)
        assert not nbad, (r, nbad, bad)


@functools.lru_cache(maxsize=None)
def fcs_frames():
    """Every frame of the list with its LE FCS: valid on two thirds, one byte (anywhere) flipped in the rest."""
    _, frames = matrix()
    rng = np.random.default_rng(33)
    out = []
    for i, f in enumerate(frames):
        b = bytearray(f + struct.pack("<I", O.crc32(f)))
        if i % 3 == 2:
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def want_fcs_ok(frames):
    ok = [int(O.crc32(f) == O.CRC32_RESIDUE) for f in frames]
    gap = [int(O.crc32(g) == O.CRC32_RESIDUE) for g in _gaps(frames)]
    return np.array(ok, np.uint8), np.array(gap, np.uint8)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_gpu_rx_verify_with_options(cuda, flags, filt, residues):
    """lnx_rx_verify_batch: fcs_ok and the verdict of the frame without its FCS."""
    names, _ = matrix()
    frames = fcs_frames()
    bare = tuple(f[:-4] for f in frames)
    off = pair_offsets(frames)
    ok_f, ok_g = want_fcs_ok(frames)
    assert 0.6 < ok_f.mean() < 0.7 and not ok_g.any()
    want_ok = interleave(ok_f, ok_g, 0, 0)
    want_v = interleave(want_verdicts(bare, flags, filt), want_gap_verdicts(frames, flags, filt, 4), 0, 0)
    _, cf = _filters(filt)
    image, o = _flat(cuda, "rxfcs", frames), _dev(cuda, off)
    for r in residues:
        ok, verdict = L.rx_verify_batch(place(image, r), o, flags=flags, filter=cf)
        en = _entry_names(names, len(off) - 1)
        nbad, bad = _report(en, ok.cpu().numpy(), want_ok)
        assert not nbad, ("fcs_ok", r, nbad, bad)
        nbad, bad = _report(en, verdict.cpu().numpy(), want_v)
        assert not nbad, ("verdict", r, nbad, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 3])
def test_gpu_rx_verify_no_fcs_with_options(cuda, flags, filt, residues):
    """LNX_RX_NO_FCS: fcs_ok = 1, the verdict over the whole frame."""
    names, frames = matrix()
    off = pair_offsets(frames)
    want_v = interleave(want_verdicts(frames, flags, filt), want_gap_verdicts(frames, flags, filt, 0), 0, 0)
    _, cf = _filters(filt)
    image, o = _flat(cuda, "rx", frames), _dev(cuda, off)
    for r in residues:
        ok, verdict = L.rx_verify_batch(place(image, r), o, flags=flags | L.RX_NO_FCS, filter=cf)
        assert bool(ok.all()), r
        nbad, bad = _report(_entry_names(names, len(off) - 1), verdict.cpu().numpy(), want_v)
        assert not nbad, (r, nbad, bad)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
def test_gpu_pcap_with_options(cuda, residues):
    names, frames = matrix()
    off = pair_offsets(frames)
    want = interleave(want_pcap(frames), want_gap_pcap(frames), 0, 0)
    image, o = _flat(cuda, "rx", frames), _dev(cuda, off)
    for r in residues:
        got = L.pcap_verify_batch(place(image, r), o).cpu().numpy()
        nbad, bad = _report(_entry_names(names, len(off) - 1), got, want)
        assert not nbad, (r, nbad, bad)


# ---- transmit
def _image(frames, results):
    """The bytes a call must leave: results[i] at slot i, every other byte of the slots as it was."""
    img = slots(frames).copy()
    for i, w in enumerate(results):
        img[i, :len(w)] = np.frombuffer(w, np.uint8)
    return img.reshape(-1)


def _first_diff(got, want, names):
    """None, or where the device tensors `got` and `want` first differ: (count, slot, label, offset in the slot)."""
    import torch
    if torch.equal(got, want):
        return None
    bad = torch.nonzero(got != want).flatten()
    at = int(bad[0])
    return int(bad.numel()), at // STRIDE, names[at // STRIDE], at % STRIDE, int(got[at]), int(want[at])


@functools.lru_cache(maxsize=None)
def tx_sequence(route):
    """(labels, frames): the list with 64 filler frames at the indices (t n) >> 6 the route rule samples:
    1514-byte stale TCP frames behind 8 option bytes (mean 1514: the generate rows) or 60-byte stale UDP
    runts (mean 60: tx_finish's checksum step)."""
    names, frames = matrix()
    rng = np.random.default_rng(896)
    n = len(frames) + 64
    at = {(t * n) >> 6 for t in range(64)}
    assert len(at) == 64
    rest = iter(zip(names, frames))
    out = []
    for i in range(n):
        if i in at:
            size = 1514 - 14 - 28 - 20 if route == "generate_rows" else 60 - 14 - 20 - 8
            pay = rng.integers(0, 256, size, dtype=np.uint8).tobytes()
            if route == "generate_rows":
                f = G.ether(0x0800, G.ipv4(6, G.tcp(pay), opts=G.opt_fill("rand", 8, rng), fix_l4=False))
            else:
                f = G.ether(0x0800, G.ipv4(17, G.udp(pay), fix_l4=False))
            b = bytearray(f)
            b[16:18], b[24:26] = rng.integers(0, 256, 2, dtype=np.uint8).tobytes(), b"\xde\xad"
            out.append((f"filler/{len(f)}", bytes(b)))
        else:
            out.append(next(rest))
    return tuple(nm for nm, _ in out), tuple(f for _, f in out)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
@pytest.mark.parametrize("route", ["generate_rows", "tx_finish"])
def test_gpu_tx_checksum_both_routes_with_options(cuda, route, residues):
    """lnx_tx_checksum_batch: the whole buffer, the lengths and the statuses."""
    import torch
    names, frames = tx_sequence(route)
    n = len(frames)
    sampled = [len(frames[(t * n) >> 6]) for t in range(64)]
    assert (sum(sampled) >= 64 * TX_SHORT_MEAN) == (route == "generate_rows"), sum(sampled)  # tx_gate_probe_kernel
    want = want_tx(frames)
    image = _flat(cuda, route, frames)
    after = on_device(cuda, ("tx image", route), lambda: _image(frames, [w for w, _ in want]))
    starts = torch.arange(n, dtype=torch.int64, device=cuda) * STRIDE
    lens = _dev(cuda, _lens(frames).astype(np.int32))
    for r in residues:
        d, dl = place(image, r), lens.clone()
        st = L.tx_checksum_batch(d, starts, dl).cpu().numpy()
        nbad, bad = _report(names, st, [s for _, s in want])
        assert not nbad, (r, nbad, bad)
        assert torch.equal(dl, lens), r
        diff = _first_diff(d, after, names)
        assert diff is None, (r, diff)


@functools.lru_cache(maxsize=None)
def want_finish(flags, capacity):
    """(bytes, status) of oracle.tx_checksum then oracle.fcs_append on every frame of the list."""
    _, frames = matrix()
    out = []
    for f, (g, st) in zip(frames, want_tx(frames)):
        w, st = (g, st) if flags & 1 else (f, 0)
        st2 = 0
        if flags & 2:
            w, st2 = O.fcs_append(w, capacity)
        out.append((w, st or st2))
    return tuple(out)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
@pytest.mark.parametrize("flags,capacity", [(3, STRIDE), (3, CAP_SMALL), (2, STRIDE), (2, CAP_SMALL), (1, STRIDE)])
def test_gpu_tx_finish_with_options(cuda, flags, capacity, residues):
    """lnx_tx_finish_batch: the whole buffer (every byte outside the finished
    frames included), the new lengths and the statuses; capacity 4224 fits
    every frame, 4000 gives ErrShortBuffer on the 4000-byte payloads."""
    import torch
    names, frames = matrix()
    n = len(frames)
    want = want_finish(flags, capacity)
    short = [i for i, (_, s) in enumerate(want) if s == O.ERR_SHORT_BUFFER]
    if flags & 2 and capacity == CAP_SMALL:
        assert len(short) >= 66 and all(len(frames[i]) + 4 > capacity for i in short)
        assert max(range(n), key=lambda i: len(frames[i])) in short
    else:
        assert not short
    image = _flat(cuda, "rx", frames)
    after = on_device(cuda, ("finish image", flags, capacity), lambda: _image(frames, [w for w, _ in want]))
    starts = torch.arange(n, dtype=torch.int64, device=cuda) * STRIDE
    lens = _dev(cuda, _lens(frames).astype(np.int32))
    want_len = np.array([len(w) for w, _ in want], dtype=np.int32)
    for r in residues:
        d, dl = place(image, r), lens.clone()
        st = L.tx_finish_batch(d, starts, dl, capacity, flags=flags).cpu().numpy()
        nbad, bad = _report(names, st, [s for _, s in want])
        assert not nbad, (r, nbad, bad)
        nbad, bad = _report(names, dl.cpu().numpy(), want_len)
        assert not nbad, (r, nbad, bad)
        diff = _first_diff(d, after, names)
        assert diff is None, (r, diff)


@pytest.mark.gpu
@pytest.mark.parametrize("residues", RESIDUE_GROUPS)
def test_gpu_tx_checksum_then_fcs_append_is_tx_finish(cuda, residues):
    """lnx_fcs_append_batch after lnx_tx_checksum_batch leaves the buffer, the
    lengths and the statuses of lnx_tx_finish_batch with both steps."""
    import torch
    names, frames = matrix()
    n = len(frames)
    image = _flat(cuda, "rx", frames)
    after = on_device(cuda, ("finish image", 3, STRIDE), lambda: _image(frames, [w for w, _ in want_finish(3, STRIDE)]))
    starts = torch.arange(n, dtype=torch.int64, device=cuda) * STRIDE
    lens = _dev(cuda, _lens(frames).astype(np.int32))
    for r in residues:
        a, la = place(image, r), lens.clone()
        st = L.tx_finish_batch(a, starts, la, STRIDE, flags=3)
        b, lb = place(image, r), lens.clone()
        c1 = L.tx_checksum_batch(b, starts, lb)
        c2 = L.fcs_append_batch(b, starts, lb, STRIDE)
        diff = _first_diff(b, after, names)
        assert diff is None, (r, diff)
        assert torch.equal(a, b) and torch.equal(la, lb) and torch.equal(st, torch.where(c1 != 0, c1, c2)), r


# ---- the ring's kernels on host memory (zero copy: the HOST = true instantiations)
@functools.lru_cache(maxsize=None)
def ring_subset(form):
    """rx: the valid, option-flipped, transport-flipped and trailing frames with their FCS (a byte flipped
    in a third); tx: the transmit forms."""
    names, frames = matrix()
    if form == "tx":
        idx = [i for i, nm in enumerate(names) if nm.startswith("tx/")]
        return tuple(names[i] for i in idx), tuple(frames[i] for i in idx)
    idx = [i for i, nm in enumerate(names) if nm.rsplit("/", 1)[1] in ("valid", "optflip", "l4flip", "trail")]
    with_fcs = fcs_frames()
    return tuple(names[i] for i in idx), tuple(with_fcs[i] for i in idx)


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 1, 2, 3), (4, 5, 6, 7)])
def test_gpu_ring_ingress_zero_copy_with_options(cuda, offsets):
    """RxRing.ingress on the ring's pinned slots (zero copy, host threshold 0):
    the frame of slot k starts `offset` bytes into it, which is its address
    modulo 8."""
    names, frames = ring_subset("rx")
    n = len(frames)
    flags = L.VERIFY_ICMP | L.VERIFY_EVIL_BIT
    want_ok = np.array([int(O.crc32(f) == O.CRC32_RESIDUE) for f in frames], np.uint8)
    want_v = want_verdicts(tuple(f[:-4] for f in frames), flags, None)
    assert 0.6 < want_ok.mean() < 0.7 and set(want_v.tolist()) >= {0, 2, 3}
    base, lens = slots(frames), _lens(frames)
    ring = L.RxRing(n, slot_cap=STRIDE, batch_slots=1024, depth=3, host_threshold=0)
    try:
        ring.set_zero_copy(True)
        assert ring.slots.ctypes.data % 16 == 0
        for offset in offsets:
            ring.slots[:, :offset] = 0xEE
            ring.slots[:, offset:] = base[:, :STRIDE - offset]
            ring.lengths[:] = lens + offset
            s0 = ring.stats()
            ok, verdict = ring.ingress(0, n, offset=offset, flags=flags)
            nbad, bad = _report(names, ok, want_ok)
            assert not nbad, ("fcs_ok", offset, nbad, bad)
            nbad, bad = _report(names, verdict, want_v)
            assert not nbad, ("verdict", offset, nbad, bad)
            assert ring.stats()["zero_copy_frames"] - s0["zero_copy_frames"] == n
    finally:
        ring.close()


@pytest.mark.gpu
@pytest.mark.parametrize("offsets", [(0, 1, 2, 3), (4, 5, 6, 7)])
def test_gpu_ring_egress_zero_copy_with_options(cuda, offsets):
    """egress_packets on views of the ring's slots (patched in place, host
    threshold 0): sizes, statuses and every byte of every slot."""
    names, frames = ring_subset("tx")
    n = len(frames)
    base, lens = slots(frames), _lens(frames)
    ring = L.RxRing(n, slot_cap=STRIDE, batch_slots=1024, depth=3, host_threshold=0)
    try:
        ring.set_zero_copy(True)
        for offset in offsets:
            capacity = STRIDE - 8
            want = []
            for f, (g, st) in zip(frames, want_tx(frames)):
                w, st2 = O.fcs_append(g, capacity)
                want.append((w, st or st2))
            ring.slots[:, :offset] = 0xEE
            ring.slots[:, offset:] = base[:, :STRIDE - offset]
            after = ring.slots.copy()
            for i, (w, _) in enumerate(want):
                after[i, offset:offset + len(w)] = np.frombuffer(w, np.uint8)
            s0 = ring.stats()
            sizes, status = ring.egress_packets([ring.slots[i] for i in range(n)], lens, offset=offset,
                                                capacity=capacity)
            nbad, bad = _report(names, status, [s for _, s in want])
            assert not nbad, (offset, nbad, bad)
            nbad, bad = _report(names, sizes, [len(w) for w, _ in want])
            assert not nbad, (offset, nbad, bad)
            rows = np.nonzero((ring.slots != after).any(axis=1))[0]
            assert rows.size == 0, (offset, int(rows.size), [(int(i), names[i], int(np.nonzero(
                ring.slots[i] != after[i])[0][0]) - offset) for i in rows[:10]])
            assert ring.stats()["zero_copy_frames"] - s0["zero_copy_frames"] == n
    finally:
        ring.close()
