"""The checksum kernels at the 16-bit length limits and with saturated sums.

lneto's stack accepts any IPv4 total length and IPv6 payload length up to 65535
(internet/stack-ip4.go:100-107, internet/stack-ip6.go:86-138).  Parts of the
receive-verdict, pcap and transmit kernels are correct only up to a 16-bit or
64 KiB bound (DESIGN.md §3.13 "limits pinned"): the half-word sums of the qword
rows must not wrap 2^32, tx_finish shifts its CRC correction by Z_k with
k < 2^16, the checksum step answers 15 from L - 14 / L - 54 = 65536 on, and the
receive check sorts a 513-line frame into the last length class beside runts.
tests/framegen.py limit_frames() puts frames on those bounds, with payloads of
all 0xFF, all 0x00, FF 00 and 00 FF (the byte sums E and O at their maximum and
minimum, separately) and random bytes, and every entry is compared with the
oracle on every one of them: integer equality, no tolerances.

The oracle's own sum is anchored on a closed form first: n bytes of 0xFF (n
even) add (n / 2) * 0xFFFF to the running uint32 sum."""
import ctypes
import collections
import functools
import struct

import numpy as np
import pytest

from oracle import oracle as O
from tests import framegen as G

import lneto_amd as L

CAPACITY = 65600  # transmit slots and ring slots: the longest frame the step accepts (65589 B) + FCS, and some room


# ---------------------------------------------------------------- the frames
@functools.lru_cache(maxsize=None)
def limit():
    pairs = G.limit_frames()
    return tuple(n for n, _ in pairs), tuple(f for _, f in pairs)


def _filters(name):
    from tests.test_rx_filter import _pair
    return _pair(name) if name else (None, None)


@functools.lru_cache(maxsize=None)
def want_verdicts(frames, flags, filt):
    """oracle.ingress_verdict of every frame of the tuple `frames` (computed once per argument set)."""
    of, _ = _filters(filt)
    return np.array([O.ingress_verdict(f, flags, of) for f in frames], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def want_pcap(frames):
    return np.array([O.pcap_checksums(f) for f in frames], dtype=np.uint8)


@functools.lru_cache(maxsize=None)
def want_tx(frames):
    return tuple(O.tx_checksum(f) for f in frames)


def _with_fcs(f: bytes) -> bytes:
    return f + struct.pack("<I", O.crc32(f))


@functools.lru_cache(maxsize=None)
def runts():
    """Valid 60-byte frames (IPv4 UDP / TCP / ICMP echo, padded), verdict 0."""
    out = [G.ether(0x0800, G.ipv4(17, G.udp(b"limit-runt-payload"))),
           G.ether(0x0800, G.ipv4(6, G.tcp(b"runt"))) + bytes(2),
           G.ether(0x0800, G.ipv4(1, G.icmp(8, b"echo-runt-payload!")))]
    assert all(len(f) == 60 for f in out)
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fillers():
    """15 valid frames of 60..1800 B, one in each 128-byte length class the receive
    check sorts by (rx_verify_kernel.hip rv_rows: classes 1..13 and the clamped
    14), with their FCS: nine of them take the 8-lane rows (class < 10)."""
    rng = np.random.default_rng(1800)
    out = []
    for k, n in enumerate((60, 200, 330, 460, 590, 700, 830, 960, 1090, 1200, 1350, 1500, 1600, 1700, 1796)):
        pay = rng.integers(0, 256, n - (62 if k % 2 else 42), dtype=np.uint8).tobytes()
        f = G.ether(0x86DD, G.ipv6(17, G.udp(pay))) if k % 2 else G.ether(0x0800, G.ipv4(17, G.udp(pay)))
        assert len(f) == n
        out.append(f)
    classes = [min((len(f) + 4 + 127) >> 7, 14) for f in out]
    assert classes == list(range(1, 15)) + [14] and sum(c < 10 for c in classes) >= 8
    return tuple(out)


@functools.lru_cache(maxsize=None)
def mixed(fcs: bool):
    """Every limit frame followed by the 15 fillers (a group of the receive check
    is a run of consecutive frames: every group holds limit frames, every length
    class and enough short frames for the 8-lane rows).  fcs: each frame carries
    its LE FCS, valid on two thirds of them, one byte flipped in the rest."""
    _, frames = limit()
    seq = []
    for f in frames:
        seq.append(f)
        seq.extend(fillers())
    if not fcs:
        return tuple(seq)
    rng = np.random.default_rng(33)
    out = []
    for i, f in enumerate(seq):
        b = bytearray(_with_fcs(f))
        if i % 3 == 2:
            b[int(rng.integers(0, len(b)))] ^= 1 << int(rng.integers(0, 8))
        out.append(bytes(b))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def want_rx(fcs: bool):
    frames = mixed(fcs)
    if not fcs:
        return np.ones(len(frames), np.uint8), want_verdicts(frames, 0, None)
    ok = np.array([int(O.crc32(f) == O.CRC32_RESIDUE) for f in frames], np.uint8)
    return ok, want_verdicts(tuple(f[:-4] for f in frames), 0, None)


def _pack(frames, base_pad):
    parts, offs, pos = [b"\xAA" * base_pad], [base_pad], base_pad
    for f in frames:
        parts.append(f)
        pos += len(f)
        offs.append(pos)
    return np.frombuffer(b"".join(parts) + b"\xBB" * 24, dtype=np.uint8).copy(), np.array(offs, dtype=np.int64)


def _pack_reversed(frames):
    """Frames back to back in decreasing address order, off = [a0, b0, a1, b1, ...]
    with a_{k+1} < b_k: frame 2k is frames[k], frame 2k + 1 (end below start) is empty."""
    pos, at, parts = {}, 3, [b"\x5a" * 3]
    for k in reversed(range(len(frames))):
        pos[k] = at
        parts.append(frames[k])
        at += len(frames[k])
    off = np.array([x for k, f in enumerate(frames) for x in (pos[k], pos[k] + len(f))], dtype=np.int64)
    assert (off[2::2] < off[1:-1:2]).all()
    return np.frombuffer(b"".join(parts) + b"\xBB" * 24, dtype=np.uint8).copy(), off


def _report(names_or_frames, got, want):
    bad = np.nonzero(np.asarray(got) != np.asarray(want))[0]
    return [(int(i), names_or_frames[i] if isinstance(names_or_frames[i], str) else len(names_or_frames[i]),
             int(got[i]), int(want[i])) for i in bad[:10]]


# ------------------------------------------------------------------ CPU tests
def test_generator_covers_every_kind_length_fill_and_outcome():
    names, frames = limit()
    assert len(set(names)) == len(names)
    for kinds, lengths, variants in ((G.LIMIT_KINDS4, G.LIMIT_TL4, G.LIMIT_VARIANTS4),
                                     (G.LIMIT_KINDS6, G.LIMIT_PL6, G.LIMIT_VARIANTS6)):
        for kind in kinds:
            for length in lengths:
                for fill in G.LIMIT_FILLS:
                    f = frames[names.index(f"rx/{kind}/{length}/{fill}/asis")]
                    v6 = kind.endswith("6")
                    assert len(f) == length + (54 if v6 else 14)
                    assert struct.unpack(">H", f[18:20] if v6 else f[16:18])[0] == length
                    assert f[14] == (0x60 if v6 else 0x4F if kind == "tcp4opt" else 0x45)
                    assert O.ingress_verdict(f, 3) == 0 and O.pcap_checksums(f) == 0, (kind, length, fill)
                    got, st = O.tx_checksum(f)  # the step reproduces a valid frame as it stands
                    assert st == 0 and got == f
            for fill in G.LIMIT_FILLS:
                assert f"tx/{kind}/65535/{fill}" in names
            assert sum(n.startswith(f"tx/{kind}/65536/") for n in names) == 1
        fam = [n for n in names if n.startswith("rx/") and n.split("/")[1] in kinds]
        seen = collections.Counter(n.split("/")[-1] for n in fam)
        assert set(seen) == set(variants) | {"asis"}, seen
        # every variant meets every fill
        assert {(n.split("/")[3], n.split("/")[4]) for n in fam} >= {(fl, v) for fl in G.LIMIT_FILLS for v in variants
                                                                  if v != "udp_len_plus1"}
    rx = [i for i, n in enumerate(names) if n.startswith("rx/")]
    v = want_verdicts(frames, 0, None)
    assert (v[rx] == 0).sum() * 2 >= len(rx)
    for code in (O.ERR_BAD_CRC, O.ERR_TRUNCATED_FRAME, O.ERR_INVALID_LENGTH_FIELD):
        assert (v[rx] == code).sum() > 0, code
    assert max(len(frames[i]) for i in rx) > 65536 + 14 + 4000  # trailing bytes: frames past 64 KiB + 14
    # pcap reports a broken header sum apart from a good transport sum, and both
    p = want_pcap(frames)
    assert all(p[i] == O.PCAP_IP_HDR_BAD for i, n in enumerate(names) if n.endswith("/bad_hdr"))
    assert (p == (O.PCAP_IP_HDR_BAD | O.PCAP_PROTO_BAD)).sum() > 0
    st = collections.Counter(s for _, s in want_tx(frames))
    assert st[0] > 100 and st[O.ERR_INVALID_LENGTH_FIELD] >= 7 + 20 and set(st) == {0, O.ERR_INVALID_LENGTH_FIELD}
    for i, n in enumerate(names):
        if n.startswith("tx/"):
            over = n.split("/")[2] == "65536"
            assert len(frames[i]) - (54 if n.split("/")[1].endswith("6") else 14) == (65536 if over else 65535)
            got, s = want_tx(frames)[i]
            assert s == (O.ERR_INVALID_LENGTH_FIELD if over else 0) and (got == frames[i]) == over, n
            if not over:
                assert O.ingress_verdict(got, 3) == 0, n


def test_generator_checksum_field_twins():
    names, frames = limit()
    a, b = frames[names.index("twin/tcp4/65535/sum_0000")], frames[names.index("twin/tcp4/65535/sum_ffff")]
    assert len(a) == 65549 and a[50:52] == b"\0\0" and b[50:52] == b"\xff\xff" and a[:50] + a[52:] == b[:50] + b[52:]
    for f in (a, b):
        assert O.ingress_verdict(f) == 0 and O.pcap_checksums(f) == 0
        assert O.tx_checksum(f) == (a, 0)  # the correct checksum is 0x0000 (TCP has no NeverZeroSum)
    for kind, at, n in (("udp4", 40, 65549), ("udp6", 60, 65589)):
        f = frames[names.index(f"twin/{kind}/65535/sum_zero")]
        assert len(f) == n and f[at:at + 2] == b"\xff\xff" and O.ingress_verdict(f) == 0
        zeroed = f[:at] + b"\0\0" + f[at + 2:]
        seed = O.ipv4_udp_pseudo(f[14:], n - 34) if kind == "udp4" else O.ipv6_pseudo(f[14:54])
        assert seed.payload_sum16(zeroed[at - 6:]) == 0  # the computed sum is 0: the step writes 0xFFFF
        g = frames[names.index(f"tx/{kind}/65535/sum_zero")]
        assert g[at:at + 2] != b"\xff\xff" and O.tx_checksum(g) == (f, 0)


def all_ff_sum(seed: int, n: int) -> int:
    """sum16 of the running sum after n bytes of 0xFF: n // 2 words of 0xFFFF
    and, for odd n, the last byte << 8 (crc.go:52-59), modulo 2^32."""
    return O.sum16((seed + (n // 2) * 0xFFFF + (n & 1) * 0xFF00) & 0xFFFFFFFF)


FF_SEEDS = (0, 1, 0xFFFF0000, 0xFFFFFFFF)


@pytest.mark.parametrize("seed", FF_SEEDS)
@pytest.mark.parametrize("n", [65534, 1 << 17, (1 << 25) + (1 << 18)])
def test_oracle_all_ff_closed_form(n, seed):
    """The anchor that does not come from the oracle's own loop: both
    restatements against the closed form.  At n = 2^25 + 2^18 the running sum
    wraps 2^32 whatever the seed."""
    assert ((n // 2) * 0xFFFF >= 1 << 32) == (n > 1 << 17)
    buf = b"\xff" * n
    assert O.c_payload_sum16(seed, buf) == all_ff_sum(seed, n)
    assert O.payload_sum16(seed, buf) == all_ff_sum(seed, n)


def _host_verdict(frame, flags, cfilt):
    return L.lib.lnx_ingress_verdict(frame, len(frame), flags, ctypes.byref(cfilt) if cfilt is not None else None)


@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 3])
def test_host_verdicts_at_the_limits(flags, filt):
    names, frames = limit()
    _, cf = _filters(filt)
    got = [_host_verdict(f, flags, cf) for f in frames]
    bad = _report(names, got, want_verdicts(frames, flags, filt))
    assert not bad, bad


def test_host_pcap_at_the_limits():
    names, frames = limit()
    bad = _report(names, [L.pcap_checksums(f) for f in frames], want_pcap(frames))
    assert not bad, bad


def test_host_tx_checksum_at_the_limits():
    names, frames = limit()
    for n, f, (want, wst) in zip(names, frames, want_tx(frames)):
        buf = (ctypes.c_uint8 * len(f)).from_buffer_copy(f)
        st = L.lib.lnx_tx_checksum(buf, len(f))
        assert st == wst and bytes(buf) == want, (n, st, wst)


@pytest.mark.parametrize("slack", [0, 1])
def test_host_fcs_append_at_the_limits(slack):
    """Capacity L + 4 (exact fit) and L + 3 (ErrShortBuffer, frame and length untouched)."""
    names, frames = limit()
    for n, f in zip(names, frames):
        cap = len(f) + 4 - slack
        buf = (ctypes.c_uint8 * (len(f) + 4))()
        ctypes.memmove(buf, f, len(f))
        ln = ctypes.c_uint32(len(f))
        st = L.lib.lnx_fcs_append(buf, ctypes.byref(ln), cap)
        want, wst = O.fcs_append(f, cap)
        assert wst == (6 if slack else 0)
        assert st == wst and ln.value == len(want) and bytes(buf)[:ln.value] == want, (n, cap, st, wst)
        assert bytes(buf)[len(want):] == bytes(len(f) + 4 - len(want)), n


# the sum16 segments: lengths around 2^16 and 2^17, 1 MiB + 1, and 2^25 + 2^18 + 3, where the even-offset
# byte sum E of an all-0xFF segment (255 * 2^24 and more) wraps 2^32 itself, as does the reference's running sum
SUM16_LENGTHS = (65535, 65536, 131071, (1 << 20) + 1, (1 << 25) + (1 << 18) + 3)
SUM16_FILLS = ("ff", "ff00", "00ff", "rand")
SUM16_ALIGNS = tuple(range(0, 128, 8)) + tuple(range(1, 128, 8))  # 0, 8, .. 120 and 1, 9, .. 121: both parities


def _rand_seed(k):
    return int(np.random.default_rng(900 + k).integers(0, 1 << 32))


@functools.lru_cache(maxsize=None)
def sum16_case():
    """(data, off, len, seed, fill of each segment): every length x fill at start
    alignment 5 with the four seeds, and the segments up to 131071 B at 16 more
    start alignments spread over 0..127 (the seeds in rotation).  Each (length,
    fill) has its bytes once, in a region that starts on a 128-byte line and
    keeps 128 spare bytes after the last segment."""
    rng = np.random.default_rng(16)
    parts, offs, lens, seeds, fills, pos = [], [], [], [], [], 0
    for fill in SUM16_FILLS:
        for n in SUM16_LENGTHS:
            body = G.limit_fill(fill, n + 256, rng)
            base = pos + (-pos) % 128  # the region starts on a line
            parts.append(bytes(base - pos) + body)
            pos = base + len(body)
            four = (0, 0xFFFFFFFF, 0xFFFF0000, _rand_seed(len(offs)))
            for sd in four:
                offs.append(base + 5), lens.append(n), seeds.append(sd), fills.append(fill)
            if n <= 131071:
                for k, a in enumerate(SUM16_ALIGNS):
                    offs.append(base + a), lens.append(n), seeds.append(four[k % 4]), fills.append(fill)
    data = np.frombuffer(b"".join(parts) + bytes(256), dtype=np.uint8).copy()
    return (data, np.array(offs, dtype=np.uint64), np.array(lens, dtype=np.uint32), np.array(seeds, dtype=np.uint32),
            tuple(fills))


@functools.lru_cache(maxsize=None)
def sum16_want():
    data, off, ln, seed, fills = sum16_case()
    want = O.sum16_segments(data, off, ln, seed)
    for i, fill in enumerate(fills):  # the closed form, where there is one
        if fill == "ff":
            assert int(want[i]) == all_ff_sum(int(seed[i]), int(ln[i])), i
    assert sum(f == "ff" for f in fills) == len(fills) // 4
    return want


def test_host_sum16_at_the_limits():
    """lnx_sum16_payload on the segments of the GPU sum16 test (each length x fill
    x seed once, the alignments being the device's concern)."""
    data, off, ln, seed, fills = sum16_case()
    want = sum16_want()
    raw = data.ctypes.data
    done = set()
    for i in range(len(off)):
        key = (fills[i], int(ln[i]), int(seed[i]))
        if key in done:
            continue
        done.add(key)
        got = L.lib.lnx_sum16_payload(int(seed[i]), ctypes.cast(ctypes.c_void_p(raw + int(off[i])), ctypes.POINTER(ctypes.c_uint8)),
                                      int(ln[i]))
        assert got == int(want[i]), (key, got, int(want[i]))
    assert len(done) >= len(SUM16_LENGTHS) * len(SUM16_FILLS) * 4


# ------------------------------------------------------------------ GPU tests
def _dev(cuda, *arrays):
    import torch
    return [torch.from_numpy(np.ascontiguousarray(a)).to(cuda) for a in arrays]


@pytest.mark.gpu
@pytest.mark.parametrize("base_pad", range(8))
@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 3])
def test_gpu_ingress_rows_at_the_limits(cuda, flags, filt, base_pad):
    """lnx_ingress_verify_batch on the limit frames alone: the mean length is
    far past 1280 B (api.cpp kIngressShortMean), so the ingress rows run."""
    names, frames = limit()
    assert sum(len(f) for f in frames) / len(frames) >= 1280
    _, cf = _filters(filt)
    d, o = _dev(cuda, *_pack(frames, base_pad))
    got = L.ingress_verify_batch(d, o, flags=flags, filter=cf).cpu().numpy()
    bad = _report(names, got, want_verdicts(frames, flags, filt))
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("filt", [None, "plain"])
@pytest.mark.parametrize("flags", [0, 3])
def test_gpu_ingress_short_route_at_the_limits(cuda, flags, filt):
    """The same entry with 55 valid 60-byte runts after every limit frame: the
    mean is under 1280 B and the receive check without its CRC runs
    (rx_verify_kernel), one limit frame among the runts of each group."""
    _, frames = limit()
    seq, idx = [], []
    for k, f in enumerate(frames):
        idx.append(len(seq))
        seq.append(f)
        seq.extend(runts()[(k + j) % 3] for j in range(55))
    assert sum(len(f) for f in seq) / len(seq) < 1280
    _, cf = _filters(filt)
    want = np.tile(np.uint8(0), len(seq))
    rv = want_verdicts(runts(), flags, filt)
    for k in range(len(frames)):
        for j in range(55):
            want[idx[k] + 1 + j] = rv[(k + j) % 3]
    want[idx] = want_verdicts(frames, flags, filt)
    d, o = _dev(cuda, *_pack(seq, 3))
    got = L.ingress_verify_batch(d, o, flags=flags, filter=cf).cpu().numpy()
    bad = _report(seq, got, want)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("base_pad", range(8))
def test_gpu_rx_verify_at_the_limits(cuda, base_pad):
    """lnx_rx_verify_batch: the limit frames with their FCS (a byte flipped in a
    third), each followed by frames of 60..1800 B of every length class."""
    frames = mixed(True)
    d, o = _dev(cuda, *_pack(frames, base_pad))
    ok, verdict = L.rx_verify_batch(d, o)
    want_ok, want_v = want_rx(True)
    assert 0.6 < want_ok.mean() < 0.7
    bad = _report(frames, ok.cpu().numpy(), want_ok) + _report(frames, verdict.cpu().numpy(), want_v)
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_rx_verify_no_fcs_at_the_limits(cuda):
    frames = mixed(False)
    d, o = _dev(cuda, *_pack(frames, 5))
    ok, verdict = L.rx_verify_batch(d, o, flags=L.RX_NO_FCS)
    want_ok, want_v = want_rx(False)
    bad = _report(frames, ok.cpu().numpy(), want_ok) + _report(frames, verdict.cpu().numpy(), want_v)
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("base_pad", range(8))
def test_gpu_pcap_at_the_limits(cuda, base_pad):
    frames = mixed(False)
    d, o = _dev(cuda, *_pack(frames, base_pad))
    got = L.pcap_verify_batch(d, o).cpu().numpy()
    bad = _report(frames, got, want_pcap(frames))
    assert not bad, bad


@pytest.mark.gpu
def test_gpu_rx_verify_and_pcap_reversed_address_order(cuda):
    """The same frames laid out in decreasing address order, off = [a0, b0, a1,
    b1, ...]: no group's frames lie inside [off[first], off[last]), so the
    per-frame paths see the limits too.  Every second frame is empty."""
    for fcs in (True, False):
        frames = mixed(fcs)
        d, o = _dev(cuda, *_pack_reversed(frames))
        if fcs:
            ok, verdict = L.rx_verify_batch(d, o)
            want_ok, want_v = want_rx(True)
            ok, verdict = ok.cpu().numpy(), verdict.cpu().numpy()
            bad = _report(frames, ok[0::2], want_ok) + _report(frames, verdict[0::2], want_v)
            assert not bad, bad
            assert not ok[1::2].any() and (verdict[1::2] == O.ERR_TRUNCATED_FRAME).all()
        else:
            got = L.pcap_verify_batch(d, o).cpu().numpy()
            bad = _report(frames, got[0::2], want_pcap(frames))
            assert not bad, bad
            assert (got[1::2] == O.ERR_TRUNCATED_FRAME << 2).all()


# ---- transmit
@functools.lru_cache(maxsize=None)
def tx_runts():
    """60-byte transmit inputs (IPv4 UDP / TCP / ICMP) with garbage in the fields the step writes."""
    rng = np.random.default_rng(60)
    out = []
    for kind in ("udp4", "tcp4", "icmp4"):
        out.append(G._limit_garble(G._limit_packet(kind, 26, "rand", rng, fix_l4=False), kind, rng))
    assert all(len(f) == 60 for f in out)
    return tuple(out)


def _layout(frames, lead, room, order=None):
    """Frames at starts = 8 k + lead in a junk-filled buffer, frame i with
    max(len, room) bytes and 8..15 more before the next one; `order`: the frames'
    order in memory (default: as given).  Returns (buffer, starts, lengths)."""
    order = range(len(frames)) if order is None else order
    starts = np.zeros(len(frames), dtype=np.int64)
    pos = 0
    for i in order:
        starts[i] = pos + lead
        pos += (max(len(frames[i]), room) + lead + 15) & ~7
    buf = np.random.default_rng(len(frames) + lead).integers(0, 256, pos + 8, dtype=np.uint8)
    for i, f in enumerate(frames):
        buf[starts[i]:starts[i] + len(f)] = np.frombuffer(f, np.uint8)
    return buf, starts, np.array([len(f) for f in frames], dtype=np.int32)


def _image(buf, starts, results):
    """The buffer the call must leave: `results[i]` at starts[i], every other byte as it was."""
    img = buf.copy()
    for s, w in zip(starts, results):
        img[s:s + len(w)] = np.frombuffer(w, np.uint8)
    return img


def _first_diff(got, want, starts):
    bad = np.nonzero(got != want)[0]
    if bad.size == 0:
        return None
    k = int(np.searchsorted(np.sort(starts), bad[0], side="right")) - 1
    return (int(bad.size), int(bad[0]), "frame at rank", k, int(bad[0]) - int(np.sort(starts)[max(k, 0)]))


@pytest.mark.gpu
@pytest.mark.parametrize("base_pad", [0, 3])
@pytest.mark.parametrize("route", ["generate_rows", "tx_finish"])
def test_gpu_tx_checksum_both_routes_at_the_limits(cuda, route, base_pad):
    """lnx_tx_checksum_batch on the limit frames alone (the generate rows) and
    with 96 runts around each (the 64 sampled lengths, all runts', average under 896 B,
    api.cpp kTxChecksumShortMean: tx_finish's checksum step); the whole buffer
    image, the lengths and the statuses against the oracle."""
    names, frames = limit()
    seq = list(frames)
    if route == "tx_finish":
        # periods of 97 frames, the limit frame at a place in the period that none of the 64 sampled indices has
        n = 97 * len(frames)
        at = min(set(range(97)) - {((i * n) >> 6) % 97 for i in range(64)}, key=lambda x: abs(x - 48))
        seq = []
        for k, f in enumerate(frames):
            r = [tx_runts()[(k + j) % 3] for j in range(96)]
            seq.extend(r[:at] + [f] + r[at:])
    n = len(seq)
    sampled = [len(seq[(i * n) >> 6]) for i in range(64)]
    assert (sum(sampled) < 64 * 896) == (route == "tx_finish"), sum(sampled)
    rw = want_tx(tx_runts())
    ws = {id(f): w for f, w in zip(frames, want_tx(frames))}
    ws.update({id(f): w for f, w in zip(tx_runts(), rw)})
    want = [ws[id(f)] for f in seq]
    buf, starts, lens = _layout(seq, base_pad, 0)
    d, ds, dl = _dev(cuda, buf, starts, lens)
    st = L.tx_checksum_batch(d, ds, dl).cpu().numpy()
    assert np.array_equal(dl.cpu().numpy(), lens)
    bad = _report(seq, st, [s for _, s in want])
    assert not bad, bad
    diff = _first_diff(d.cpu().numpy(), _image(buf, starts, [w for w, _ in want]), starts)
    assert diff is None, diff


@functools.lru_cache(maxsize=None)
def want_finish(flags, capacity):
    """(bytes, status) of oracle.tx_checksum then oracle.fcs_append on every limit
    frame; capacity < 0: each frame's exact fit max(L, 60) + 4, less -capacity - 1."""
    _, frames = limit()
    out = []
    for f, (g, st) in zip(frames, want_tx(frames)):
        w, st = (g, st) if flags & 1 else (f, 0)
        st2 = 0
        if flags & 2:
            w, st2 = O.fcs_append(w, capacity if capacity >= 0 else max(len(f), 60) + 4 + capacity + 1)
        out.append((w, st or st2))
    return tuple(out)


def _finish(cuda, frames, want, flags, capacity, lead, order=None, two_calls=False):
    import torch
    buf, starts, lens = _layout(frames, lead, capacity, order)
    d, ds, dl = _dev(cuda, buf, starts, lens)
    st = L.tx_finish_batch(d, ds, dl, capacity, flags=flags)
    bad = _report(frames, st.cpu().numpy(), [s for _, s in want])
    assert not bad, bad
    bad = _report(frames, dl.cpu().numpy(), [len(w) for w, _ in want])
    assert not bad, bad
    diff = _first_diff(d.cpu().numpy(), _image(buf, starts, [w for w, _ in want]), starts)
    assert diff is None, diff
    if two_calls:
        b, lb = _dev(cuda, buf, lens)
        c1 = L.tx_checksum_batch(b, ds, lb)
        c2 = L.fcs_append_batch(b, ds, lb, capacity)
        assert torch.equal(d, b) and torch.equal(dl, lb) and torch.equal(st, torch.where(c1 != 0, c1, c2))
    return st.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("lead", range(8))
@pytest.mark.parametrize("flags", [3, 2, 1])
def test_gpu_tx_finish_at_the_limits(cuda, flags, lead):
    """lnx_tx_finish_batch with capacity 65600 on every limit frame, each frame
    starting at `lead` modulo 8 (both address parities; the IPv6 maximum frames,
    L = 65589, shift their CRC correction by Z_k with k = 65461: bit 15 of k):
    statuses, lengths and the whole buffer image against oracle.tx_checksum
    followed by oracle.fcs_append; with both steps, the same as
    lnx_tx_checksum_batch followed by lnx_fcs_append_batch."""
    names, frames = limit()
    assert sum(len(f) == 65589 and n.startswith("tx/") for n, f in zip(names, frames)) >= 15
    want = want_finish(flags, CAPACITY)
    st = _finish(cuda, frames, want, flags, CAPACITY, lead, two_calls=flags == 3)
    if flags & 1:
        assert (st == 15).sum() >= 27
    assert (st == 0).sum() > 200
    if flags == 2:
        assert (st == 6).sum() >= 10  # (the frames near 64 KiB with 4097 trailing bytes do not fit)


@pytest.mark.gpu
@pytest.mark.parametrize("slack", [0, 1])
@pytest.mark.parametrize("flags", [3, 2])
def test_gpu_tx_finish_exact_fit_at_the_limits(cuda, flags, slack):
    """cap = max(L, 60) + 4 (exact fit) and one byte less (status 6, the length
    untouched and, without the checksum step, the frame too): the limit frames
    of each length in one call, back to back at a stride of cap bytes in a
    buffer that ends with the last one."""
    import torch
    _, frames = limit()
    want = want_finish(flags, -1 - slack)
    for n in sorted({len(f) for f in frames}):
        idx = [i for i, f in enumerate(frames) if len(f) == n]
        cap = n + 4 - slack
        buf = np.random.default_rng(n).integers(0, 256, cap * len(idx), dtype=np.uint8)
        starts = np.arange(len(idx), dtype=np.int64) * cap
        for k, i in enumerate(idx):
            buf[starts[k]:starts[k] + n] = np.frombuffer(frames[i], np.uint8)
        d, ds, dl = _dev(cuda, buf, starts, np.full(len(idx), n, dtype=np.int32))
        st = L.tx_finish_batch(d, ds, dl, cap, flags=flags).cpu().numpy()
        w = [want[i] for i in idx]
        assert st.tolist() == [s for _, s in w], (n, st.tolist())
        assert dl.cpu().numpy().tolist() == [len(x) for x, _ in w]
        if slack:
            assert all(s == 6 or (flags & 1 and s == 15) for s in st) and all(len(x) == n for x, _ in w)
        diff = _first_diff(d.cpu().numpy(), _image(buf, starts, [x for x, _ in w]), starts)
        assert diff is None, (n, diff)
        if slack and flags == 2:
            assert np.array_equal(d.cpu().numpy(), buf)


@pytest.mark.gpu
def test_gpu_tx_finish_reversed_address_order(cuda):
    """The limit frames laid out in decreasing address order (reversed d_start)."""
    _, frames = limit()
    _finish(cuda, frames, want_finish(3, CAPACITY), 3, CAPACITY, 5, order=list(reversed(range(len(frames)))),
            two_calls=True)


# ---- sum16
@pytest.mark.gpu
def test_gpu_sum16_at_the_limits(cuda):
    """lnx_sum16_batch on segments of 65535 B to 2^25 + 2^18 + 3 B against
    oracle.sum16_segments (and, for the all-0xFF segments, the closed form)."""
    data, off, ln, seed, fills = sum16_case()
    d, do, dlen, dseed = _dev(cuda, data, off.view(np.int64), ln.view(np.int32), seed.view(np.int32))
    got = L.sum16_batch(d, do, dlen, dseed).cpu().numpy().view(np.uint16)
    want = sum16_want()
    bad = [(int(i), fills[i], int(ln[i]), int(off[i]) % 128, hex(int(seed[i])), int(got[i]), int(want[i]))
           for i in np.nonzero(got != want)[0][:10]]
    assert not bad, bad
    for i in [i for i, f in enumerate(fills) if f == "ff"]:
        assert int(got[i]) == all_ff_sum(int(seed[i]), int(ln[i]))


# ---- the ring
@pytest.mark.gpu
@pytest.mark.parametrize("zero_copy", [True, False])
@pytest.mark.parametrize("where", ["host", "device"])
def test_gpu_ring_packets_at_the_limits(cuda, where, zero_copy):
    """RxRing(nslots=64, slot_cap=65600): lnx_ingress_packets and
    lnx_egress_packets over the limit frames, 40 at a time, on the ring's own
    slots; below the default host threshold (the host path) and with threshold
    0 (the kernels), zero copy on and off.  The frames with 4097 trailing bytes
    do not fit a slot and stay out (every other one is compared)."""
    names, frames = limit()
    rx_all = mixed(True)[::16]  # the limit frames with their FCS, a third broken
    want_ok, want_v = (a[::16] for a in want_rx(True))
    fit = [i for i, f in enumerate(rx_all) if len(f) <= CAPACITY]
    assert len(fit) >= len(frames) - 25
    ring = L.RxRing(64, slot_cap=CAPACITY, host_threshold=None if where == "host" else 0)
    try:
        ring.set_zero_copy(zero_copy)
        s0 = ring.stats()
        for c0 in range(0, len(fit), 40):
            idx = fit[c0:c0 + 40]
            views = []
            for k, i in enumerate(idx):
                ring.slots[k, :len(rx_all[i])] = np.frombuffer(rx_all[i], np.uint8)
                views.append(ring.slots[k, :len(rx_all[i])])
            ok, verdict = ring.ingress_packets(views)
            bad = _report([names[i] for i in idx], ok, want_ok[idx]) + \
                _report([names[i] for i in idx], verdict, want_v[idx])
            assert not bad, (where, zero_copy, bad)
        want = want_finish(3, CAPACITY)
        txi = [i for i, f in enumerate(frames) if len(f) <= CAPACITY]
        for c0 in range(0, len(txi), 40):
            idx = txi[c0:c0 + 40]
            junk = np.random.default_rng(c0).integers(0, 256, (len(idx), CAPACITY), dtype=np.uint8)
            ring.slots[:len(idx)] = junk
            for k, i in enumerate(idx):
                ring.slots[k, :len(frames[i])] = np.frombuffer(frames[i], np.uint8)
            sizes, status = ring.egress_packets([ring.slots[k] for k in range(len(idx))], [len(frames[i]) for i in idx],
                                                capacity=CAPACITY)
            for k, i in enumerate(idx):
                w, st = want[i]
                assert int(status[k]) == st and int(sizes[k]) == len(w), (names[i], int(status[k]), st)
                assert ring.slots[k, :len(w)].tobytes() == w, names[i]
                assert np.array_equal(ring.slots[k, len(w):], junk[k, len(w):]), names[i]
        s1 = ring.stats()
        total = len(fit) + len(txi)
        if where == "host":
            assert s1["device_batches"] == s0["device_batches"] and s1["host_frames"] - s0["host_frames"] == total
        else:
            assert s1["device_frames"] - s0["device_frames"] == total
            assert s1["zero_copy_frames"] - s0["zero_copy_frames"] == (total if zero_copy else 0)
    finally:
        ring.close()
