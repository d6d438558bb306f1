"""Running internet checksums on the host side of the boundary (CPU only):
lnx_sum_partial and lnx_sum16_chain against a pure-Python restatement of
lneto's crc.go:17-59 over the concatenated bytes, the new batch entries'
argument checks, the exact list of the lnxs:: kernels in both libraries, the
static audit of their ISA, and the host functions in programs of their own."""
import ctypes
import os
import random
import re
import subprocess
import sys

import pytest

import lneto_amd as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lneto_amd", "csrc", "sum16_chain_kernel.hip")
HIPCC = "/opt/rocm/bin/hipcc"
M32 = 0xFFFFFFFF
LENS = [0, 1, 2, 3, 5, 64, 127, 129]


# ---- the oracle: crc.go restated, nothing shared with the library
def ref_write_even(s, b):
    """sumWriteEven (crc.go:23-28): uint32 wrap-around sum of big-endian words."""
    assert len(b) % 2 == 0
    for i in range(0, len(b), 2):
        s = (s + ((b[i] << 8) | b[i + 1])) & M32
    return s


def ref_raw(s, b):
    """PayloadSum16 (crc.go:52-58) before its last line: the odd last byte << 8."""
    odd = len(b) & 1
    s = ref_write_even(s, b[:len(b) - odd])
    if odd:
        s = (s + (b[-1] << 8)) & M32
    return s


def ref_sum16(s):
    """sum16 (crc.go:17-21)."""
    s = (s & 0xFFFF) + (s >> 16)
    return ~(s + (s >> 16)) & 0xFFFF


def frames(rng, count):
    for i in range(count):
        segs = [rng.randbytes(rng.choice(LENS)) for _ in range(rng.randrange(0, 9))]
        yield (0, M32, rng.getrandbits(32))[i % 3], segs


def test_partial_and_chain_match_the_restatement():
    rng = random.Random(791)
    for seed, segs in frames(rng, 1500):
        whole = b"".join(segs)
        raw = ref_raw(seed, whole)
        assert L.sum16_chain(seed, segs) == ref_sum16(raw), (seed, [len(g) for g in segs])
        s, pos = seed, 0
        for g in segs:  # piece by piece, the phase from the bytes so far
            s = L.sum_partial(s, g, pos & 1)
            pos += len(g)
        assert s == raw, (seed, [len(g) for g in segs])
        assert L.sum_partial(seed, whole, 0) == raw
        assert L.sum_partial(seed, whole, 2) == raw  # only bit 0 of the phase is read
    assert L.sum16_chain(0x12345678, []) == ref_sum16(0x12345678)  # m == 0
    assert L.lib.lnx_sum16_chain(7, None, None, 0) == ref_sum16(7)


def test_partial_is_write_even_and_payload_sum16():
    rng = random.Random(792)
    for n in LENS + [1500, 1501]:
        p = rng.randbytes(n)
        for s in (0, M32, rng.getrandbits(32)):
            if n % 2 == 0:
                assert L.sum_partial(s, p, 0) == L.sum_write_even(s, p) == ref_write_even(s, p)
            assert L.sum16(L.sum_partial(s, p, 0)) == L.payload_sum16(s, p) == ref_sum16(ref_raw(s, p))


def test_two_partial_calls_equal_one_over_the_concatenation():
    rng = random.Random(793)
    for la in LENS + [1499]:
        for lb in LENS + [1500]:
            a, b, s = rng.randbytes(la), rng.randbytes(lb), rng.getrandbits(32)
            one = L.sum_partial(s, a + b, 0)
            assert L.sum_partial(L.sum_partial(s, a, 0), b, la & 1) == one == ref_raw(s, a + b), (la, lb)
            # and behind an odd number of bytes: both pieces shifted by one
            z = ref_raw(s, b"\x5a")
            assert L.sum_partial(L.sum_partial(z, a, 1), b, (la + 1) & 1) == ref_raw(s, b"\x5a" + a + b), (la, lb)


def test_the_wrap_is_the_references():
    """140004 bytes of 0xFF from 0xFFFFFFF0: the unwrapped value is 0x21170EE7E, so
    a 64-bit accumulator (or an end-around carry before the last step) gives
    another checksum."""
    segs = [b"\xff" * 70001, b"\xff" * 3, b"\xff" * 70000]
    assert ref_raw(0xFFFFFFF0, b"".join(segs)) == 0x1170EE7E and ref_sum16(0x1170EE7E) == 17
    s, pos = 0xFFFFFFF0, 0
    for g in segs:
        s = L.sum_partial(s, g, pos & 1)
        pos += len(g)
    assert s == 0x1170EE7E
    assert L.sum16(s) == 17 and L.sum16_chain(0xFFFFFFF0, segs) == 17


# ---- the C-ABI
NEW = ["lnx_sum_partial", "lnx_sum16_chain", "lnx_sum_partial_batch", "lnx_sum16_chain_batch"]


def test_new_declarations_are_exported():
    text = open(os.path.join(ROOT, "include", "lneto_amd.h")).read()
    declared = set(re.findall(r"\b(lnx_[a-z0-9_]+)\s*\(", re.sub(r"/\*.*?\*/", "", text, flags=re.S)))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(lnx_\w+)", out))
    for s in NEW:
        assert s in declared and s in exported, s
    for name in ("sum_partial", "sum16_chain", "sum_partial_batch", "sum16_chain_batch"):
        assert name in L.__all__ and callable(getattr(L, name))


def test_batch_entries_validate_without_gpu():
    lib, E = L.lib, L.LNX_EINVAL
    part, chain = lib.lnx_sum_partial_batch, lib.lnx_sum16_chain_batch
    # zero counts are no-ops whatever the pointers
    assert part(None, None, None, None, None, 0, None, None) == 0
    assert chain(None, None, None, 5, None, 0, None, None, None, None, None) == 0
    buf = (ctypes.c_uint32 * 256)()
    p = ctypes.addressof(buf)
    far = p + 4 * 128  # a second array, 128 dwords on
    # a NULL required pointer with a count
    assert part(None, p, p, None, None, 4, far, None) == E
    assert part(p, None, p, None, None, 4, far, None) == E
    assert part(p, p, None, None, None, 4, far, None) == E
    assert part(p, p, p, None, None, 4, None, None) == E
    assert chain(p, p, p, 4, None, 2, None, far, p, None, None) == E      # d_first
    assert chain(None, p, p, 4, p, 2, None, far, p, None, None) == E      # d_bytes with nseg > 0
    assert chain(p, None, p, 4, p, 2, None, far, p, None, None) == E
    assert chain(p, p, None, 4, p, 2, None, far, p, None, None) == E
    assert chain(p, p, p, 4, p, 2, None, None, p, None, None) == E        # the workspace with nseg > 0
    # both outputs NULL, with and without segments
    assert chain(p, p, p, 4, p, 2, None, far, None, None, None) == E
    assert chain(None, None, None, 0, p, 2, None, None, None, None, None) == E
    # the workspace (2 * nseg dwords) overlapping an output: the same array, one shared byte at either end
    nseg, nframes = 8, 6
    for out16, sum32 in ((far, None), (None, far), (p, far), (far, p)):
        assert chain(p, p, p, nseg, p, nframes, None, far, out16, sum32, None) == E
    assert chain(p, p, p, nseg, p, nframes, None, far, far + 4 * 2 * nseg - 1, None, None) == E
    assert chain(p, p, p, nseg, p, nframes, None, far, None, far + 4 * 2 * nseg - 1, None) == E
    assert chain(p, p, p, nseg, p, nframes, None, far, far - 2 * nframes + 1, None, None) == E
    assert chain(p, p, p, nseg, p, nframes, None, far, None, far - 4 * nframes + 1, None) == E
    # d_seed and d_sum overlapping: the same array, and ranges that share one element
    assert part(p, p, p, far, None, 8, far, None) == E
    assert part(p, p, p, far, None, 8, far + 4 * 7, None) == E
    assert part(p, p, p, far + 4 * 7, None, 8, far, None) == E


# ---- the kernels
def _kernels(path, prefix):
    out = subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, "/dev/stdout"],
                         capture_output=True, check=True).stdout
    return sorted(set(m.decode() for m in re.findall(rb"(" + prefix + rb"\w+)\.kd", out)))


def test_both_libraries_hold_exactly_the_running_sum_kernels():
    """namespace lnxs: sum_bytes_kernel in its planes and partial forms and
    sum_fold_kernel; the research library the same."""
    want = ["_ZN4lnxs15sum_fold_kernelEPKjS1_mPKmmS1_PtPj",
            "_ZN4lnxs16sum_bytes_kernelILNS_8ByteModeE0EEEvPKhPKmPKjS7_S3_mPj",
            "_ZN4lnxs16sum_bytes_kernelILNS_8ByteModeE1EEEvPKhPKmPKjS7_S3_mPj"]
    assert _kernels(L.LIB_PATH, rb"_ZN4lnxs") == want
    assert _kernels(L.RESEARCH_LIB_PATH, rb"_ZN4lnxs") == want


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("build", ["product", "research"])
def test_running_sum_kernels_pass_the_loop_audit(tmp_path, build):
    """tools/prof/audit_loops.py over sum16_chain_kernel.hip, compiled as
    tests/test_kernel_audit.py compiles the other sources: no exec-narrowing
    loop around wide loads, no stale cross-lane source, no scratch."""
    flags = ["-DLNX_RESEARCH"] if build == "research" else []
    subprocess.run([HIPCC, "--offload-arch=gfx950", "-O3", "-std=c++20", "-mllvm",
                    "-amdgpu-atomic-optimizer-strategy=None", "-c", "--save-temps", *flags, "-o", str(tmp_path / "k.o"),
                    SRC], cwd=tmp_path, check=True, capture_output=True)
    asm = next(p for p in os.listdir(tmp_path) if p.endswith("gfx950.s"))
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tools", "prof", "audit_loops.py"), str(tmp_path / asm)],
                       capture_output=True, text=True)
    assert r.returncode == 0, r.stdout
    meta = open(tmp_path / asm).read()
    spills = re.findall(r"\.name:\s+(\S+)\s*\n(?:.*\n)*?\s+\.private_segment_fixed_size:\s+(\d+)", meta)
    assert len(spills) == 3, spills
    assert all(int(b) == 0 for _, b in spills), spills


# ---- programs of their own
def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/sum_chain_host_main.cpp: the two host functions in a program
    with its own main, compiled together with sum_chain_host.cpp under ASan +
    UBSan; nothing is preloaded and nothing is loaded into Python."""
    exe = tmp_path / "sum_chain_host_main"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "sum_chain_host_main.cpp"),
                    os.path.join(ROOT, "lneto_amd", "csrc", "sum_chain_host.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout


def test_cpp_delegates_compile_and_run(tmp_path):
    """tests/cpp/test_sum_chain_api.cpp: the .hpp delegates against the built
    library, built as tests/test_abi.py builds test_host_api.cpp."""
    src = os.path.join(ROOT, "tests", "cpp", "test_sum_chain_api.cpp")
    exe = tmp_path / "test_sum_chain_api"
    subprocess.run(["g++", "-std=c++17", "-O1", "-Wall", "-I", os.path.join(ROOT, "include"), src,
                    "-o", str(exe), "-L", os.path.dirname(L.LIB_PATH), "-llneto_amd",
                    f"-Wl,-rpath,{os.path.dirname(L.LIB_PATH)}"], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
