"""lnx_crc32_search_batch's product kernel at its own edges
(crc32_search_o_kernel, search_kernel.hip): eight captures a wave, eight lanes
a capture, 1536-byte blocks of eight 192-byte lane segments, each four 48-byte
chains; the register carried from lane 7 into the next block; the group buffer
descriptor when the eight captures lie inside [off[8q], off[8q + 8]) and
guarded per-capture loads otherwise; the hit window [min_off, L - 4], which
alone keeps the next capture's bytes (real bytes on the descriptor path) from
giving a hit.  Every result is compared with the C oracle's per-byte search of
the capture's own bytes (-1 stated directly for min_off past L - 4), by integer
equality, and every case list asserts on the CPU that its classes are there.

The host function's limits run in a program of its own under ASan + UBSan."""
import os
import struct
import subprocess

import numpy as np
import pytest

from oracle import oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CHAIN, SEG, BLOCK, OCT = 48, 192, 1536, 8
I64_MIN, I64_MAX = -2**63, 2**63 - 1


def fcs(b: bytes) -> bytes:
    return struct.pack("<I", O.crc32(b))


def want_of(cap: bytes, m: int) -> int:
    """-1 stated for every min_off above len - 4, the oracle's search otherwise."""
    if max(m, 0) > len(cap) - 4:
        return -1
    return O.c_crc32_search(cap, m)


def edge_cuts(edges, top, lo=-6, hi=2):
    return sorted({e * k + d for e in edges for k in range(top // e + 1) for d in range(lo, hi + 1)
                   if 0 <= e * k + d <= top})


def group_is_fast(offs, q):
    """The kernel's rule for reading group q through one descriptor, restated."""
    n = len(offs) - 1
    ga, gb = OCT * q, min(OCT * q + OCT, n)
    gs, ge = int(offs[ga]), int(offs[gb])
    if ge < gs or ge - (gs & ~3) + 3 >= 2**31:
        return False
    return all(int(offs[c + 1]) <= int(offs[c]) or (int(offs[c]) >= gs and int(offs[c + 1]) <= ge)
               for c in range(ga, gb))


def all_groups_fast(offs):
    return all(group_is_fast(offs, q) for q in range((len(offs) + OCT - 2) // OCT))


def no_group_fast(offs):
    """No full group of eight reads through the descriptor (a last group of one or
    two captures may: it holds no step back)."""
    full = (len(offs) - 1) // OCT
    return full > 0 and not any(group_is_fast(offs, q) for q in range(full))


def pack(caps, pad=0):
    """The captures one after the other from byte `pad` (no gaps: what follows a
    capture is the next capture's first byte), 8 spare bytes behind."""
    offs = np.zeros(len(caps) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in caps])
    return b"\xa5" * pad + b"".join(caps) + b"\0" * 8, offs + pad


def caps_of(blob, offs):
    return [bytes(blob[int(s):int(e)]) if e > s else b"" for s, e in zip(offs[:-1], offs[1:])]


def search(cuda, blob, offs, mins, view=0):
    import torch
    import lneto_amd as L
    d = torch.from_numpy(np.frombuffer(bytes(blob), dtype=np.uint8).copy()).to(cuda)
    o = torch.from_numpy(np.asarray(offs, dtype=np.int64) - view).to(cuda)
    m = None if mins is None else torch.tensor(list(mins), dtype=torch.int64, device=cuda)
    out = torch.full((len(offs) - 1,), -7, dtype=torch.int64, device=cuda)  # -7: no result is below -1
    got = L.crc32_search_batch(d[view:] if view else d, o, m, out=out)
    return got.cpu().numpy().tolist()


def assert_equal(got, want, info):
    bad = [i for i, (g, w) in enumerate(zip(got, want)) if g != w]
    assert not bad, [(i, got[i], want[i], info(i)) for i in bad[:10]]
    assert len(got) == len(want)


# ------------------------------------------------------------- the host function
def test_host_search_limits_under_sanitizers(tmp_path):
    """tests/cpp/test_crc_search_limits.cpp: lnx_crc32_search on captures of 0, 3,
    4, 7 and 200 bytes with min_off from INT64_MIN to 2^63 - 1, in a program of
    its own, the host sources compiled with ASan + UBSan.  Before the fix the
    length guard's min_off + 4 wrapped and the function read 2^63 bytes."""
    exe = tmp_path / "test_crc_search_limits"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_crc_search_limits.cpp"),
                    os.path.join(ROOT, "lneto_amd", "csrc", "cpu_path.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_oracle_search_limits():
    """The C oracle and the Python one give -1 past len - 4 up to 2^63 - 1 (the C
    one computed min_off + 4 too)."""
    cap = b"abcdefgh" + fcs(b"abcdefgh") + b"xy"
    for m in (I64_MAX, I64_MAX - 3, I64_MAX - 4, 2**32 + 8, 2**31 + 8, len(cap) - 3, 9):
        assert O.c_crc32_search(cap, m) == -1 and O.crc32_search(cap, m) == -1, m
    for m in (I64_MIN, -1, 0, 8):
        assert O.c_crc32_search(cap, m) == 8 and O.crc32_search(cap, m) == 8, m
    assert O.c_crc32_search(b"", I64_MAX) == -1 and O.c_crc32_search(b"abc", I64_MAX - 3) == -1


# ------------------------------------------------------------------ 1. group shapes
GROUP_LENGTHS = [0, 3, 4, 40, 191, 192, 1535, 1536, 1537, 3100, 4700]


@pytest.mark.gpu
@pytest.mark.parametrize("n", [8, 9, 15, 16, 17, 63, 64, 65, 127, 128, 129])
def test_group_shapes(cuda, n):
    """Eight captures a wave, 128 a workgroup: every count around both, the
    captures of one wave ending in different 1536-byte blocks, hits and misses
    mixed, the last wave partly live."""
    rng = np.random.default_rng(300 + n)
    caps, mins = [], []
    for i in range(n):
        ln = GROUP_LENGTHS[(i * 7 + n) % len(GROUP_LENGTHS)]  # 7 is coprime to 11: every length, mixed in a wave
        cap = bytearray(rng.bytes(ln))
        if i % 3 != 2 and ln >= 4:
            cut = int(rng.integers(0, ln - 3))
            cap[cut:cut + 4] = fcs(bytes(cap[:cut]))
        caps.append(bytes(cap))
        mins.append(int(rng.choice([0, 0, 1, ln // 2])))
    want = [want_of(c, m) for c, m in zip(caps, mins)]
    assert sum(w >= 0 for w in want) >= 2 and sum(w < 0 for w in want) >= 2
    for q in range((n + OCT - 1) // OCT):  # every wave holds captures of different block counts
        group = caps[OCT * q:OCT * q + OCT]
        assert len(group) < 3 or len({(len(c) + BLOCK - 1) // BLOCK for c in group}) >= 2, q
    blob, offs = pack(caps)
    assert all_groups_fast(offs)
    assert_equal(search(cuda, blob, offs, mins), want, lambda i: (len(caps[i]), mins[i]))


# -------------------------------------------------------------------- 2. edge sweep
SWEEP_CUTS = sorted(set(range(0, 401)) | set(edge_cuts((CHAIN, SEG, BLOCK), 4700)))
TRAILS = [0, 1, 5, 40]


@pytest.fixture(scope="module")
def sweep_bodies():
    rng = np.random.default_rng(310)
    return rng.bytes(4800), rng.bytes(64)


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_edge_sweep(cuda, sweep_bodies, pad):
    """An FCS at every offset 0..400 and six bytes below to two above every
    48-byte chain, 192-byte segment and 1536-byte block edge up to 4700, so that
    off, off + 3 and off + 4 fall on each side of each edge; 0, 1, 5 or 40
    trailing bytes; min_off 0, cut and cut + 1; the batch at each base alignment
    and the captures' own starts at every alignment."""
    body, tail = sweep_bodies
    caps, mins, cuts = [], [], []
    for ci, cut in enumerate(SWEEP_CUTS):
        for mk in range(3):
            tr = TRAILS[(ci + mk + pad) % 4]
            caps.append(body[:cut] + fcs(body[:cut]) + tail[:tr])
            mins.append((0, cut, cut + 1)[mk])
            cuts.append(cut)
    assert len(caps) < 10_000
    want = [want_of(c, m) for c, m in zip(caps, mins)]
    blob, offs = pack(caps, pad)
    # the classes: hits, -1, every alignment of a capture's start, hits inside each edge window
    assert sum(w >= 0 for w in want) >= 2 * len(SWEEP_CUTS) - 4
    assert sum(w < 0 for w in want) >= len(SWEEP_CUTS) - 4
    assert min(np.bincount(offs[:-1] & 3, minlength=4)) >= 300
    for edge, least in ((CHAIN, 1500), (SEG, 400), (BLOCK, 50)):
        for d in range(-6, 3):
            k = sum(1 for w, c in zip(want, cuts) if w == c and c >= edge - 6 and (c - d) % edge == 0)
            assert k >= least // 9, (edge, d, k)
    assert all_groups_fast(offs)
    assert_equal(search(cuda, blob, offs, mins), want, lambda i: (cuts[i], len(caps[i]), mins[i]))


# ------------------------------------------------- 3. nothing outside the window
def lay_decreasing(units, pad):
    """Each unit's captures stay contiguous and in order; the units themselves
    lie in decreasing address order, so the entry between two units is an empty
    capture (end below start) and no group of eight lies inside
    [off[8q], off[8q + 8])."""
    blob = bytearray(b"\xa5" * pad)
    pos = {}
    for u in reversed(range(len(units))):
        pos[u] = len(blob)
        blob += b"".join(units[u])
    blob += b"\0" * 8
    offs = []
    for u, caps in enumerate(units):
        p = pos[u]
        for c in caps:
            offs.append(p)
            p += len(c)
        offs.append(p)  # the last capture's end; [p, next unit's start) is empty
    return bytes(blob), np.array(offs, dtype=np.int64)


@pytest.fixture(scope="module")
def window_cases():
    """(units, mins, wants, kinds): a unit is one capture or a pair whose second
    capture starts with the bytes the first one lacks."""
    rng = np.random.default_rng(320)
    body, tail = rng.bytes(4800), rng.bytes(40)
    cuts = sorted(set(edge_cuts((CHAIN,), 800)) | set(edge_cuts((SEG,), 1800)) | set(edge_cuts((BLOCK,), 4700)))
    units, mins, kinds = [], [], []
    for ci, cut in enumerate(cuts):
        f = fcs(body[:cut])
        for k in range(4):  # the capture ends after k of the 4 FCS bytes; the rest open the next one
            units.append([body[:cut] + f[:k], f[k:] + tail[:5 + (ci + k) % 9]])
            mins.append([0, 0])
            kinds.append("split%d" % k)
        units.append([body[:cut] + f + tail[:7]])  # min_off = cut + 1, no later hit
        mins.append([cut + 1])
        kinds.append("min_above")
        ln = cut + 4
        units.append([body[:cut] + f])             # the hit exactly at L - 4 = min_off
        mins.append([ln - 4])
        kinds.append("min_at_end")
        units.append([body[:cut] + f])             # min_off = L - 3
        mins.append([ln - 3])
        kinds.append("min_past_end")
    wants = [[want_of(c, m) for c, m in zip(u, ms)] for u, ms in zip(units, mins)]
    first = {k: [w[0] for w, kk in zip(wants, kinds) if kk == k] for k in set(kinds)}
    for k in ("split0", "split1", "split2", "split3", "min_above", "min_past_end"):
        assert len(first[k]) == len(cuts) and sum(w == -1 for w in first[k]) >= len(cuts) - 2, k
    assert all(w >= 0 for w in first["min_at_end"])
    assert len(cuts) > 200 and sum(len(u) for u in units) < 10_000
    return units, mins, wants, kinds


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_nothing_outside_the_window_descriptor_path(cuda, window_cases, pad):
    """Packed in order: the bytes behind a capture are the next capture's real
    bytes, the rest of its FCS among them, and only the hit window keeps them
    out; min_off just above the hit, at L - 4 and at L - 3."""
    units, mins, wants, kinds = window_cases
    caps = [c for u in units for c in u]
    blob, offs = pack(caps, pad)
    assert all_groups_fast(offs)
    flat_m, flat_w = [m for ms in mins for m in ms], [w for ws in wants for w in ws]
    assert_equal(search(cuda, blob, offs, flat_m), flat_w, lambda i: (len(caps[i]), flat_m[i]))


@pytest.mark.gpu
@pytest.mark.parametrize("pad", [0, 1, 2, 3])
def test_nothing_outside_the_window_guarded_path(cuda, window_cases, pad):
    """The same captures in decreasing address order (guarded loads): the bytes
    behind a capture are still there in memory and must read as nothing."""
    units, mins, wants, kinds = window_cases
    blob, offs = lay_decreasing(units, pad)
    flat_m, flat_w = [], []
    for ms, ws in zip(mins, wants):
        flat_m += list(ms) + [0]   # the empty capture between two units
        flat_w += list(ws) + [-1]
    flat_m, flat_w = flat_m[:-1], flat_w[:-1]
    assert len(offs) - 1 == len(flat_w)
    assert no_group_fast(offs)
    own = caps_of(blob, offs)
    assert [c for c in own if c] == [c for u in units for c in u if c]
    assert_equal(search(cuda, blob, offs, flat_m), flat_w, lambda i: (len(own[i]), flat_m[i]))


# ------------------------------------------------------------------ 4. several hits
def two_hits(rng, ln, p1, p2):
    cap = bytearray(rng.bytes(ln))
    cap[p1:p1 + 4] = fcs(bytes(cap[:p1]))
    cap[p2:p2 + 4] = fcs(bytes(cap[:p2]))
    return bytes(cap)


@pytest.mark.gpu
def test_several_hits(cuda):
    """Two FCS positions in one lane's different chains, in different lanes of
    one block and in different blocks; min_off picks the first, the second or
    neither.  a + crc(a) followed by the CRC of that; four leading zero bytes."""
    rng = np.random.default_rng(330)
    caps, mins, want_kind = [], [], []
    places = []
    for blk in range(3):
        for lane in range(OCT):
            base = BLOCK * blk + SEG * lane
            places.append(("chains", base + 5 + lane, base + CHAIN * (1 + lane % 3) + 9))  # one lane, two chains
            places.append(("lanes", base + 17, BLOCK * blk + SEG * ((lane + 1 + blk) % OCT) + 100))
            places.append(("blocks", base + 44, BLOCK * (blk + 1 + lane % 2) + SEG * (7 - lane) + 3 * lane))
    for kind, a, b in places:
        p1, p2 = min(a, b), max(a, b)
        assert p2 >= p1 + 4
        if kind == "chains":
            assert p1 // SEG == p2 // SEG and p1 // CHAIN != p2 // CHAIN
        elif kind == "lanes":
            assert p1 // BLOCK == p2 // BLOCK and p1 // SEG != p2 // SEG
        else:
            assert p1 // BLOCK != p2 // BLOCK
        cap = two_hits(rng, p2 + 4 + int(rng.integers(0, 300)), p1, p2)
        for m, k in ((0, "first"), (p1, "first"), (p1 + 1, "second"), (p2, "second"), (p2 + 1, "neither")):
            caps.append(cap)
            mins.append(m)
            want_kind.append((k, p1, p2))
    for n_a in (0, 1, 44, 188, 1532, 1533):  # a + crc(a), then the CRC of that: both are hits
        a = rng.bytes(n_a)
        f1 = a + fcs(a)
        cap = f1 + fcs(f1) + rng.bytes(10)
        for m, k in ((0, "first"), (n_a + 1, "second"), (n_a + 4, "second"), (n_a + 5, "neither")):
            caps.append(cap)
            mins.append(m)
            want_kind.append((k, n_a, n_a + 4))
    zeros = b"\0\0\0\0" + rng.bytes(200)  # CRC32(nil) == 0: off 0 matches
    caps += [zeros, zeros]
    mins += [0, 1]
    want = [want_of(c, m) for c, m in zip(caps, mins)]
    assert want[-2] == 0 and want[-1] != 0
    for w, (k, p1, p2) in zip(want, want_kind):
        assert w == {"first": p1, "second": p2, "neither": -1}[k], (w, k, p1, p2)
    assert {k for k, _, _ in want_kind} == {"first", "second", "neither"}
    blob, offs = pack(caps, 1)
    assert_equal(search(cuda, blob, offs, mins), want, lambda i: (len(caps[i]), mins[i]))


# -------------------------------------------------------------- 5. min_off extremes
@pytest.mark.gpu
def test_min_off_extremes(cuda):
    """Every int64 min_off above L - 4 gives -1, up to 2^63 - 1 (the sum
    min_off + 4 wrapped there and the first hit anywhere came back), and a
    min_off of 2^31 or 2^32 more than a valid one does not become it.
    d_min_off = None is an array of zeros."""
    rng = np.random.default_rng(340)
    caps, mins, want = [], [], []
    for ln, cut in ((0, None), (3, None), (4, 0), (7, 0), (7, 3), (200, 0), (200, 100), (200, 196), (1600, 1530),
                    (3100, 9), (3100, 3096), (4700, 3000)):
        cap = bytearray(rng.bytes(ln))
        if cut is not None:
            cap[cut:cut + 4] = fcs(bytes(cap[:cut]))
        c = cut or 0
        for m in (I64_MIN, -1, 0, ln - 4, ln - 3, 2**31, 2**32, I64_MAX - 4, I64_MAX - 3, I64_MAX,
                  2**32 + c, 2**31 + c, 2**32 + c - 1, 2**63 - 2**32 + c, c, c + 1):
            caps.append(bytes(cap))
            mins.append(m)
            want.append(-1 if max(m, 0) > ln - 4 else O.c_crc32_search(bytes(cap), m))
    huge = [i for i, m in enumerate(mins) if m >= 2**31]
    assert len(huge) >= 100 and all(want[i] == -1 for i in huge)
    assert sum(1 for i in huge if want_of(caps[i], 0) >= 0) >= 80  # on captures that do hold a hit
    assert sum(w >= 0 for w in want) >= 30
    blob, offs = pack(caps, 2)
    assert_equal(search(cuda, blob, offs, mins), want, lambda i: (len(caps[i]), mins[i]))
    zero = [want_of(c, 0) for c in caps]
    got_none = search(cuda, blob, offs, None)
    assert got_none == search(cuda, blob, offs, [0] * len(caps))
    assert_equal(got_none, zero, lambda i: len(caps[i]))


# ---------------------------------------------------------------- 6. long captures
@pytest.mark.gpu
@pytest.mark.parametrize("ln", [65_541, (1 << 20) + 3, 3 * (1 << 20) + 1])
def test_long_captures(cuda, ln):
    """A capture of 43 to 2049 blocks with its hit at L - 4, in (or against) the
    last partial block, or absent, in every position of its octet beside empty, short,
    early-hit and no-hit captures: the block loop runs until the last one ends."""
    rng = np.random.default_rng(350)
    body = rng.bytes(ln)
    last_block = (ln - 1) // BLOCK * BLOCK
    # in the last partial block; 3 MiB + 1 has one byte there: the FCS then fills the last four bytes of the
    # last whole block, and the hit at L - 4 straddles the edge
    cut2 = last_block + 1 if ln - last_block >= 6 else last_block - 4
    assert ln % BLOCK != 0 and last_block - 4 <= cut2 < ln - 4
    variants = []
    for cut in (ln - 4, cut2, None):
        cap = bytearray(body)
        if cut is not None:
            cap[cut:cut + 4] = fcs(bytes(cap[:cut]))
        variants.append((bytes(cap), want_of(bytes(cap), 0)))
    assert [v[1] for v in variants] == [ln - 4, cut2, -1]
    short = rng.bytes(77)
    early = short[:30] + fcs(short[:30]) + rng.bytes(2000)
    mates = [b"", short, early, rng.bytes(1600), b"abc", early[:34], rng.bytes(3100)]
    mate_want = [want_of(c, 0) for c in mates]
    assert sorted(set(mate_want)) == [-1, 30]
    caps, mins, want = [], [], []
    for cap, w0 in variants:
        for pos in range(OCT):
            group = mates[:pos] + [cap] + mates[pos:]
            assert len(group) == OCT and group[pos] is cap
            caps += group
            mins += [0] * OCT
            want += mate_want[:pos] + [w0] + mate_want[pos:]
    blob, offs = pack(caps, 3)
    assert all_groups_fast(offs)
    assert_equal(search(cuda, blob, offs, mins), want, lambda i: (i % OCT, len(caps[i])))


# --------------------------------------------------------------------- 7. addressing
@pytest.fixture(scope="module")
def addressed():
    rng = np.random.default_rng(360)
    caps = []
    for i in range(800):
        body = rng.bytes(int(rng.choice([0, 3, 20, 60, 200, 700, 1600, 3100])) + int(rng.integers(0, 9)))
        if i % 4 != 3:
            cut = int(rng.integers(0, len(body) + 1))
            body = body[:cut] + fcs(body[:cut]) + body[cut:cut + int(rng.integers(0, 40))]
        caps.append(body)
    blob, offs = pack(caps, 3)
    return rng, caps, blob, offs


def check_own_bytes(cuda, blob, offs, mins, view=0):
    own = caps_of(blob, offs)
    want = [want_of(c, m) for c, m in zip(own, mins)]
    assert_equal(search(cuda, blob, offs, mins, view), want, lambda i: (int(offs[i]), len(own[i]), mins[i]))
    return want


@pytest.mark.gpu
def test_addressing_in_order_and_shifted_views(cuda, addressed):
    """The batch in order, d_bytes at its base and as a view shifted by 1, 2 and
    3 bytes (the descriptor's base and every word load move)."""
    rng, caps, blob, offs = addressed
    mins = [int(rng.choice([0, 1, len(c) // 2])) for c in caps]
    assert all_groups_fast(offs)
    want = check_own_bytes(cuda, blob, offs, mins)
    assert sum(w >= 0 for w in want) >= 300 and sum(w < 0 for w in want) >= 200
    for view in (1, 2, 3):
        assert offs[0] >= view
        check_own_bytes(cuda, blob, offs, mins, view)


@pytest.mark.gpu
def test_addressing_overlapping_windows_inside_the_group(cuda, addressed):
    """The inner seven offsets of every group shuffled: captures overlap, span
    several of the packed ones or are empty, the offsets are unordered, and
    every capture still lies inside [off[8q], off[8q + 8]) (descriptor path)."""
    rng, caps, blob, offs = addressed
    o = offs.copy()
    for q in range(len(caps) // OCT):
        o[OCT * q + 1:OCT * q + OCT] = rng.permutation(o[OCT * q + 1:OCT * q + OCT])
    assert all_groups_fast(o)
    s, e = o[:-1], o[1:]
    assert (e < s).sum() >= 150                              # unordered
    overl = sum(1 for i in range(len(s) - 1) for j in range(i + 1, min(i // OCT * OCT + OCT, len(s)))
                if min(e[i], e[j]) > max(s[i], s[j]))
    assert overl >= 300                                      # windows that share bytes
    want = check_own_bytes(cuda, blob, o, [0] * len(caps))
    assert sum(w >= 0 for w in want) >= 150


@pytest.mark.gpu
def test_addressing_one_capture_outside_sends_the_wave_to_guarded_loads(cuda, addressed):
    """One offset of every group points into another group: that capture lies
    outside [off[8q], off[8q + 8]) and the whole wave takes the guarded loads."""
    rng, caps, blob, offs = addressed
    o = offs.copy()
    ng = len(caps) // OCT
    for q in range(ng):
        j = 1 + q % (OCT - 1)
        far = (q + ng // 2) % ng
        o[OCT * q + j] = offs[OCT * far + j]
    assert no_group_fast(o)
    mins = [int(rng.choice([0, 1])) for _ in caps]
    want = check_own_bytes(cuda, blob, o, mins)
    assert sum(w >= 0 for w in want) >= 300
