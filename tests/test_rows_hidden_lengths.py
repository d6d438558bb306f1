"""The product rows kernel (crc32_kernel.hip, instance kRowsOffsets) on frame
lengths its dispatch sample does not see.

dispatch.hpp slice_kind gives a workgroup slice to the rows kernel when the 64
frames it samples lie within kUniformSpread bytes of each other and the slice's
mean length span / nf is one the rows kernel is faster at; the rows kernel then
picks its row width from that mean.  The sample says who owns the slice and
nothing about the lengths of the frames it skips, so the batches here are
contiguous, in-order frames in slices of 160 (the sample reads slice-local
positions 0, 2, ..., 126, each as the pair (2k, 2k + 1)): positions 0-127 of
every slice hold the base length, positions 128-159 of slice w hold hidden set
w % 7 (HIDDEN).  The rows kernel then folds

  * lean line rows (lines_body) with every line count from 1 to past three
    items of ksl = 13 lines, where every step is predicated ("lines");
  * empty and 1-3-byte frames, and FCS verify of runts and of a 4-byte frame,
    in 4-lane, lean, 16-lane and 32-lane slots ("runts", "empties");
  * frames of a length the row width was not chosen for: 4-lane rows on
    1500-byte frames, lean rows on 4000-byte frames, 16-lane and 32-lane rows
    on 1500-byte frames beside frames of 65 539, 200 000 and 500 000 bytes
    ("up1500", "up4000", "long", "one500k").

slice_kind and the width choice of crc32_rows_kernel are restated here
(owner_width) and the table of who folds each (base, set) at which width is
asserted on the CPU for several CU counts, so that a pattern cannot go hollow
on another chip's partition.  Two cells (base 1024: runts, empties; mean 819
B, between the rows kernel's two length bands) are the staged kernel's:
they stay in the batch and are the only slices the rows kernel does not own.

The GPU tests compare crc32_batch, fcs_verify_batch (both with their
short_frames=True form, where the staged kernel folds every slice: a second
opinion) and crc32_update_batch bit for bit with oracle.crc32_frames / zlib over
the final bytes.  The three entries of a base length share one buffer: every
frame of 4 bytes and more carries its little-endian FCS, every third frame one
flipped bit (first byte, middle byte, last FCS byte in turn), every hidden
4-byte frame is 00 00 00 00 (the FCS of an empty payload: verifies).  Both
verify outcomes must occur among the hidden frames of every rows-owned set that
has a frame of 4 bytes or more ("empties" has none: all its frames give 0)."""
import functools
import struct
import zlib

import numpy as np
import pytest

from oracle import oracle as O
from tests.test_offsets_any_order import CUS, plant_fcs, sampled_pairs, slice_plan

BASES = (256, 1024, 1500, 2048, 4096, 9000)
PER = 160     # frames per slice
AT = 128      # first hidden slice-local position
LEAD = 3      # the first frame's start
SPARE = 8     # bytes after the last frame
ENTRIES = ("crc", "verify", "update")

HIDDEN = (
    ("runts", [0, 1, 2, 3, 4, 5, 7, 8] * 4),
    ("empties", [0] * 32),
    ("lines", [1, 127, 128, 129, 255, 1407, 1408, 1409, 1535, 1536, 1537, 1663, 1664, 1665, 1791, 1792, 1793,
               3199, 3200, 3201, 3327, 3328, 3329, 3455, 4991, 4992, 4993] + [0] * 5),
    ("long", [9000, 65535, 65539, 200000] + [0] * 28),
    ("up1500", [1500] * 32),
    ("up4000", [4000] * 32),
    ("one500k", [500000] + [0] * 31),
)
SETS = tuple(name for name, _ in HIDDEN)
assert all(len(lens) == PER - AT for _, lens in HIDDEN)

# who folds the slices of each (base, set), and at which row width
ROWS4, LEAN, ROWS16, ROWS32, STAGED = "4-lane rows", "lean rows", "one-word 16-lane rows", "32-lane rows", "staged"
_ALL = set(SETS)
TABLE = {
    256: {ROWS4: {"runts", "empties", "lines", "up1500"}, LEAN: {"up4000"}, ROWS16: {"long", "one500k"}},
    1024: {LEAN: {"lines", "up1500"}, ROWS16: {"up4000", "long", "one500k"}, STAGED: {"runts", "empties"}},
    1500: {LEAN: {"runts", "empties", "lines", "up1500"}, ROWS16: {"up4000", "long"}, ROWS32: {"one500k"}},
    2048: {ROWS16: _ALL - {"one500k"}, ROWS32: {"one500k"}},
    4096: {ROWS16: {"runts", "empties", "lines", "up1500", "up4000"}, ROWS32: {"long", "one500k"}},
    9000: {ROWS32: _ALL},
}
WANT_OWNER = {(b, s): o for b, cells in TABLE.items() for o, sets in cells.items() for s in sets}
assert len(WANT_OWNER) == len(BASES) * len(SETS)

# dispatch.hpp / crc32_kernel.hip
UNIFORM_SPREAD = 8
GIANT_SPAN, GIANT_MEAN, GIANT_BIG, GIANT_SKEW = (1 << 31) - (1 << 20), 1 << 20, 16 << 20, 8
SHORT_MEAN, LEAN_MEAN, LINE_MEAN = 640, 1600, 4096


# -------------------------------------------------------------------- pattern
@functools.lru_cache(maxsize=None)
def lengths(base, cus):
    """The n = 160 x cus frame lengths of a batch (int64)."""
    lens = np.full((cus, PER), base, dtype=np.int64)
    for w in range(cus):
        lens[w, AT:] = HIDDEN[w % len(HIDDEN)][1]
    lens = lens.reshape(-1)
    lens.setflags(write=False)
    return lens


@functools.lru_cache(maxsize=None)
def offsets(base, cus):
    off = np.empty(PER * cus + 1, dtype=np.int64)
    off[0] = LEAD
    np.cumsum(lengths(base, cus), out=off[1:])
    off[1:] += LEAD
    off.setflags(write=False)
    return off


def set_of(i):
    """The hidden set of frame i's slice."""
    return SETS[(i // PER) % len(HIDDEN)]


def rows_length(mean):
    return mean >= 960 or 176 <= mean < 576


def owner_width(off, fb0, fb1, gmean, sampled):
    """dispatch.hpp slice_kind (plain entries) and crc32_rows_kernel's row width for
    slice [fb0, fb1); sampled: the frames slice_sample reads.  The buffer is
    line-aligned (torch's allocator), so the base's place in its line is
    off[fb0] % 128."""
    nf = fb1 - fb0
    o0, o1 = int(off[fb0]), int(off[fb1])
    span = o1 - o0 if o1 > o0 else 0
    if span + o0 % 128 >= GIANT_SPAN or span >= nf * GIANT_MEAN or \
            (span >= GIANT_BIG and span >= nf * GIANT_SKEW * gmean):
        return "giant"
    seen = [int(off[f + 1]) - int(off[f]) for f in sampled]
    assert min(seen) >= 0
    mean = span // nf
    if not (max(seen) - min(seen) <= UNIFORM_SPREAD and rows_length(mean)):
        return STAGED
    if mean < SHORT_MEAN:
        return ROWS4
    if mean >= LINE_MEAN:
        return ROWS32
    return LEAN if mean < LEAN_MEAN else ROWS16


@functools.lru_cache(maxsize=None)
def owners(base, cus):
    """Per slice: who folds it."""
    off = offsets(base, cus)
    n = len(off) - 1
    assert slice_plan(n, cus) == (cus, PER)
    gmean = (int(off[n]) - int(off[0])) // n
    sampled = {}
    for w, f in sampled_pairs(n, cus):
        sampled.setdefault(w, []).append(f)
    return tuple(owner_width(off, w * PER, (w + 1) * PER, gmean, sampled[w]) for w in range(cus))


# ------------------------------------------------------------------ CPU tests
@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("cus", CUS)
def test_owner_and_width_of_every_base_and_set(cus, base):
    own = owners(base, cus)
    assert "giant" not in own
    for w, o in enumerate(own):
        assert o == WANT_OWNER[base, SETS[w % len(HIDDEN)]], (base, SETS[w % len(HIDDEN)], w, o)
    assert {SETS[w % len(HIDDEN)] for w in range(cus)} == _ALL
    # the staged cells are the only slices the rows kernel does not own
    staged = {(base, SETS[w % len(HIDDEN)]) for w, o in enumerate(own) if o == STAGED}
    assert staged == ({(1024, "runts"), (1024, "empties")} if base == 1024 else set())


@pytest.mark.parametrize("base", BASES)
@pytest.mark.parametrize("cus", CUS)
def test_the_sample_sees_base_lengths_only(cus, base):
    off, lens = offsets(base, cus), lengths(base, cus)
    n = len(lens)
    local = np.arange(n) % PER
    hidden = set(np.nonzero(local >= AT)[0].tolist())
    assert (lens[local < AT] == base).all()
    count = 0
    for w, f in sampled_pairs(n, cus):
        # the sample reads off[f] and off[f + 1]: frame f alone
        assert f not in hidden and f % PER == 2 * (count % 64) and f // PER == w
        assert off[f + 1] >= off[f] and abs(int(off[f + 1] - off[f]) - base) <= UNIFORM_SPREAD
        count += 1
    assert count == 64 * cus
    assert int(off[0]) == LEAD and (np.diff(off) >= 0).all()


@pytest.mark.parametrize("cus", CUS)
def test_hidden_frames_of_rows_slices_reach_every_start_and_end_residue(cus):
    """Over the six batches together, the non-empty hidden frames of slices the rows
    kernel owns start at all four residues mod 4 and end at every residue mod 128
    (of the buffer, which is line-aligned)."""
    starts, ends = set(), set()
    for base in BASES:
        off, lens, own = offsets(base, cus), lengths(base, cus), owners(base, cus)
        i = np.arange(len(lens))
        pick = (i % PER >= AT) & (lens > 0) & np.array([o != STAGED for o in own])[i // PER]
        starts |= set((off[:-1][pick] % 4).tolist())
        ends |= set((off[1:][pick] % 128).tolist())
    assert starts == set(range(4)) and ends == set(range(128)), (sorted(set(range(128)) - ends))


# ----------------------------------------------------------------- references
def flip_plan(off):
    """(byte position, bit) of the flip in every third frame of 1 byte or more: the
    first byte, the middle byte and the last byte (the last FCS byte) in turn."""
    o = off
    i = np.arange(0, len(o) - 1, 3)
    s, e = o[i], o[i + 1]
    k = (i // 3) % 3
    pos = np.where(k == 0, s, np.where(k == 1, s + (e - s) // 2, e - 1))
    live = e > s
    return pos[live], (i[live] % 8).astype(np.uint8)


class Case:
    """One base length's batch at the device's CU count: the shared buffer, its
    references (each computed once, on first use) and its device copies."""

    def __init__(self, base, cus):
        self.base, self.cus = base, cus
        self.off, self.lens, self.own = offsets(base, cus), lengths(base, cus), owners(base, cus)
        n = len(self.lens)
        self.local = np.arange(n) % PER
        self.hidden = self.local >= AT
        self.rows = np.array([o != STAGED for o in self.own])[np.arange(n) // PER]
        data = np.random.default_rng(base).integers(0, 256, int(self.off[-1]) + SPARE, dtype=np.uint8)
        plant_fcs(data, self.off, range(n))
        pos, bit = flip_plan(self.off)
        data[pos] ^= np.uint8(1) << bit
        for i in np.nonzero(self.hidden & (self.lens == 4))[0]:
            data[self.off[i]:self.off[i] + 4] = 0
        data.setflags(write=False)
        self.data = data
        self.seeds = np.random.default_rng(base + 1).integers(0, 2**32, n, dtype=np.uint64).astype(np.uint32)
        self._dev = None

    def frame(self, i):
        return memoryview(self.data)[self.off[i]:self.off[i + 1]]

    @functools.cached_property
    def crc(self):
        return O.crc32_frames(self.data, self.off.astype(np.uint64), threads=16)

    @functools.cached_property
    def ok(self):
        """len >= 4 and crc32(f[:-4]) == LE32(f[-4:])"""
        ok = np.zeros(len(self.lens), dtype=np.uint8)
        for i in np.nonzero(self.lens >= 4)[0]:
            f = self.frame(i)
            ok[i] = zlib.crc32(f[:-4]) == struct.unpack("<I", f[-4:])[0]
        return ok

    @functools.cached_property
    def update(self):
        return np.array([zlib.crc32(self.frame(i), int(self.seeds[i])) for i in range(len(self.lens))],
                        dtype=np.uint32)

    def dev(self, cuda):
        import torch
        if self._dev is None:
            self._dev = (torch.from_numpy(self.data.copy()).to(cuda), torch.from_numpy(self.off.copy()).to(cuda),
                         torch.from_numpy(self.seeds.view(np.int32).copy()).to(cuda))
        return self._dev

    def compare(self, what, got, want):
        """Bit-exact; the message names base, set, slice-local position and length."""
        got, want = np.asarray(got), np.asarray(want)
        assert got.shape == want.shape, (what, got.shape, want.shape)
        bad = np.nonzero(got != want)[0]
        lines = [f"base {self.base} set {set_of(int(i))} slice {int(i) // PER} ({self.own[int(i) // PER]}) "
                 f"local {int(self.local[i])} len {int(self.lens[i])}: got {int(got[i]):#x} want {int(want[i]):#x}"
                 for i in bad[:12]]
        assert bad.size == 0, (what, f"{bad.size} wrong of {len(want)}", lines)


@functools.lru_cache(maxsize=1)  # one batch at a time: up to 400 MB on the host and on the device
def case(base, cus):
    return Case(base, cus)


def test_the_verify_pattern_has_both_outcomes_in_every_rows_owned_set():
    """At 32 CUs (the smallest batches; the GPU test asserts the same at the
    device's count) and the two smallest base lengths."""
    for base in BASES[:2]:
        check_verify_outcomes(Case(base, CUS[0]))


def check_verify_outcomes(cs):
    ok = cs.ok
    assert not ok[cs.lens < 4].any()
    four = cs.hidden & (cs.lens == 4)
    assert ok[four].all() and all(bytes(cs.frame(i)) == bytes(4) for i in np.nonzero(four)[0])
    sets = np.array([(i // PER) % len(HIDDEN) for i in range(len(cs.lens))])
    for k, (name, lens) in enumerate(HIDDEN):
        pick = cs.hidden & cs.rows & (sets == k)
        if WANT_OWNER[cs.base, name] == STAGED:
            assert not pick.any()
            continue
        assert pick.any() and not ok[pick & (cs.lens < 4)].any(), name
        seen = set(ok[pick & (cs.lens >= 4)].tolist())  # among its frames that can verify
        assert seen == ({0, 1} if max(lens) >= 4 else set()), (cs.base, name, seen)
    assert 0.5 <= ok[~cs.hidden].mean() <= 0.75  # a third of the base frames carry a flipped bit


# ------------------------------------------------------------------ GPU tests
def _cus():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


@pytest.mark.gpu
@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("base", BASES)  # (base by base: the three entries of one share its batch)
def test_gpu_hidden_lengths(cuda, base, entry):
    import lneto_amd as L
    cs = case(base, _cus())
    d, o, seeds = cs.dev(cuda)
    if entry == "crc":
        want = cs.crc
        cs.compare("crc32_batch", L.crc32_batch(d, o).cpu().numpy().view(np.uint32), want)
        cs.compare("crc32_batch short_frames", L.crc32_batch(d, o, short_frames=True).cpu().numpy().view(np.uint32),
                   want)
    elif entry == "verify":
        check_verify_outcomes(cs)
        cs.compare("fcs_verify_batch", L.fcs_verify_batch(d, o).cpu().numpy(), cs.ok)
        cs.compare("fcs_verify_batch short_frames", L.fcs_verify_batch(d, o, short_frames=True).cpu().numpy(), cs.ok)
    else:
        want = cs.update
        empty = cs.lens == 0
        assert (empty & cs.hidden).any() and np.array_equal(want[empty], cs.seeds[empty])
        cs.compare("crc32_update_batch", L.crc32_update_batch(d, o, seeds).cpu().numpy().view(np.uint32), want)
