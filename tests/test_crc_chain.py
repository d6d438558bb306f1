"""Running CRCs on the host side of the boundary (CPU only): lnx_crc32_combine
against zlib and a pure-Python restatement of the register algebra, the new
batch entries' argument checks, the exported symbols, the exact list of the
lnxc:: kernels in both libraries, and the static audits of their ISA."""
import ctypes
import os
import random
import re
import subprocess
import sys
import zlib

import pytest

import lneto_amd as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "lneto_amd", "csrc", "crc32_combine_kernel.hip")
HIPCC = "/opt/rocm/bin/hipcc"

POLY = 0xEDB88320   # reflected IEEE polynomial; bit 31 of a register is x^0
ORDER = 2**32 - 1   # the order of x modulo it
SMALL = [0, 1, 2, 3, 4, 5, 59, 60, 64, 1500, 9000, 70000]
HUGE = [2**31, 2**32 - 1, 2**32, 2**32 + 1, 2**40 + 3, 2**63 + 12345, 2**64 - 1]


# ---- the oracle: the algebra restated, nothing shared with the library
def zbit(r):
    return (r >> 1) ^ (POLY if r & 1 else 0)


def mulmod(a, b):
    """a * b mod P, 32 steps whatever the operands."""
    p = 0
    for i in range(32):
        if a & (0x80000000 >> i):
            p ^= b
        b = zbit(b)
    return p


def xpow(e):
    """x^e mod P by square-and-multiply over the bits of e."""
    r, sq = 0x80000000, 0x40000000
    while e:
        if e & 1:
            r = mulmod(sq, r)
        sq = mulmod(sq, sq)
        e >>= 1
    return r


def z_by_squaring(k):
    """x^(8k): square-and-multiply over the bits of k itself, from x^8."""
    r, sq = 0x80000000, xpow(8)
    while k:
        if k & 1:
            r = mulmod(sq, r)
        sq = mulmod(sq, sq)
        k >>= 1
    return r


def z_by_order(k):
    """x^((8k) mod (2^32 - 1)): the same power through the order of x."""
    return xpow((8 * k) % ORDER)


def combine_ref(a, b, k, zk=z_by_squaring):
    return mulmod(zk(k), a) ^ b


def test_order_of_x():
    assert xpow(ORDER) == 0x80000000
    for q in (3, 5, 17, 257, 65537):
        assert xpow(ORDER // q) != 0x80000000


def test_combine_matches_zlib_concatenation_and_seed():
    rng = random.Random(1)
    for lb in SMALL:
        for la in (0, 1, 7, 1500):
            a, b = rng.randbytes(la), rng.randbytes(lb)
            assert L.crc32_combine(zlib.crc32(a), zlib.crc32(b), lb) == zlib.crc32(a + b), (la, lb)
        seed = rng.getrandbits(32)
        for s in (0, 0xFFFFFFFF, seed):
            assert L.crc32_combine(s, zlib.crc32(b), lb) == zlib.crc32(b, s), (s, lb)
        assert L.crc32_combine(seed, zlib.crc32(b), lb) == combine_ref(seed, zlib.crc32(b), lb)


def test_combine_lengths_no_buffer_can_hold():
    rng = random.Random(2)
    for k in HUGE:
        assert z_by_squaring(k) == z_by_order(k), k  # the two oracles agree first
        for _ in range(4):
            a, b = rng.getrandbits(32), rng.getrandbits(32)
            got = L.crc32_combine(a, b, k)
            assert got == combine_ref(a, b, k), k
            assert got == combine_ref(a, b, k, z_by_order), k


def test_combine_composes():
    rng = random.Random(3)
    for _ in range(200):
        a, b, c = (rng.getrandbits(32) for _ in range(3))
        lb = rng.choice(SMALL + HUGE[:5])
        lc = rng.choice(SMALL + HUGE[:5])
        left = L.crc32_combine(L.crc32_combine(a, b, lb), c, lc)
        right = L.crc32_combine(a, L.crc32_combine(b, c, lc), (lb + lc) % 2**64)
        assert left == right, (lb, lc)
    assert L.crc32_combine(0x12345678, 0, 0) == 0x12345678  # identity (0, 0)


def test_chain_identity_against_zlib():
    """CRC32Update(s, g_0 || ... ) folded pair by pair with the host function, empty segments included."""
    rng = random.Random(4)
    for _ in range(50):
        segs = [rng.randbytes(rng.choice([0, 0, 1, 3, 4, 60, 333])) for _ in range(rng.randrange(0, 9))]
        seed = rng.getrandbits(32)
        acc = seed
        for g in segs:
            acc = L.crc32_combine(acc, zlib.crc32(g), len(g))
        assert acc == zlib.crc32(b"".join(segs), seed)


# ---- the C-ABI
NEW = ["lnx_crc32_combine", "lnx_crc32_combine_batch", "lnx_crc32_update_batch", "lnx_crc32_chain_batch",
       "lnx_fcs_verify_chain_batch"]


def test_new_declarations_are_exported():
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lneto_amd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(lnx_[a-z0-9_]+)\s*\(", src))
    out = subprocess.run(["nm", "-D", "--defined-only", L.LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = set(re.findall(r"\sT\s+(lnx_\w+)", out))
    for s in NEW:
        assert s in declared and s in exported, s
    assert "with crc=0" not in open(os.path.join(ROOT, "include", "lneto_amd.h")).read()


def test_batch_entries_validate_without_gpu():
    lib, E = L.lib, L.LNX_EINVAL
    # zero counts are no-ops whatever the pointers
    assert lib.lnx_crc32_combine_batch(None, None, None, 0, None, None) == 0
    assert lib.lnx_crc32_update_batch(None, None, 0, None, None, None) == 0
    assert lib.lnx_crc32_chain_batch(None, None, None, 5, None, 0, None, None, None, None) == 0
    assert lib.lnx_fcs_verify_chain_batch(None, None, None, 5, None, 0, None, None, None) == 0
    # a NULL required pointer with a count
    buf = (ctypes.c_uint32 * 64)()
    p = ctypes.addressof(buf)
    assert lib.lnx_crc32_combine_batch(None, p, p, 4, p, None) == E
    assert lib.lnx_crc32_combine_batch(p, None, p, 4, p, None) == E
    assert lib.lnx_crc32_combine_batch(p, p, None, 4, p, None) == E
    assert lib.lnx_crc32_combine_batch(p, p, p, 4, None, None) == E
    assert lib.lnx_crc32_update_batch(None, p, 4, None, p, None) == E
    assert lib.lnx_crc32_update_batch(p, None, 4, None, p, None) == E
    assert lib.lnx_crc32_update_batch(p, p, 4, None, None, None) == E
    assert lib.lnx_crc32_chain_batch(p, p, p, 4, None, 2, None, p, p, None) == E      # d_first
    assert lib.lnx_crc32_chain_batch(p, p, p, 4, p, 2, None, p, None, None) == E      # d_crc
    assert lib.lnx_crc32_chain_batch(None, p, p, 4, p, 2, None, p, p, None) == E      # d_bytes with nseg > 0
    assert lib.lnx_crc32_chain_batch(p, None, p, 4, p, 2, None, p, p, None) == E
    assert lib.lnx_crc32_chain_batch(p, p, None, 4, p, 2, None, p, p, None) == E
    assert lib.lnx_crc32_chain_batch(p, p, p, 4, p, 2, None, None, p, None) == E      # the workspace with nseg > 0
    assert lib.lnx_fcs_verify_chain_batch(p, p, p, 4, p, 2, p, None, None) == E       # d_ok
    assert lib.lnx_fcs_verify_chain_batch(p, p, p, 4, None, 2, p, p, None) == E
    # d_seed and d_crc overlapping: the same array, and ranges that share one element
    assert lib.lnx_crc32_update_batch(p, p, 8, p, p, None) == E
    assert lib.lnx_crc32_update_batch(p, p, 8, p, p + 4 * 7, None) == E
    assert lib.lnx_crc32_update_batch(p, p, 8, p + 4 * 7, p, None) == E


# ---- the kernels
def _kernels(path, prefix):
    out = subprocess.run(["objcopy", "-O", "binary", "--only-section=.hip_fatbin", path, "/dev/stdout"],
                         capture_output=True, check=True).stdout
    return sorted(set(m.decode() for m in re.findall(rb"(" + prefix + rb"\w+)\.kd", out)))


def test_both_libraries_hold_exactly_the_running_crc_kernels():
    """namespace lnxc: combine_pairs_kernel in its combine and seed forms,
    chain_fold_kernel in its CRC and verify forms; the research library the same."""
    want = ["_ZN4lnxc17chain_fold_kernelILb0EEEvPKjS2_mPKmmS2_Pv",
            "_ZN4lnxc17chain_fold_kernelILb1EEEvPKjS2_mPKmmS2_Pv",
            "_ZN4lnxc20combine_pairs_kernelILNS_8PairModeE0EEEvPKjS3_PKmmPj",
            "_ZN4lnxc20combine_pairs_kernelILNS_8PairModeE1EEEvPKjS3_PKmmPj"]
    assert _kernels(L.LIB_PATH, rb"_ZN4lnxc") == want
    assert _kernels(L.RESEARCH_LIB_PATH, rb"_ZN4lnxc") == want


@pytest.mark.skipif(not os.path.exists(HIPCC), reason="hipcc not installed")
@pytest.mark.parametrize("build", ["product", "research"])
def test_running_crc_kernels_pass_the_loop_audit(tmp_path, build):
    """tools/prof/audit_loops.py over crc32_combine_kernel.hip, compiled as
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
    assert len(spills) == 4, spills
    assert all(int(b) == 0 for _, b in spills), spills


def test_host_program_under_sanitizers(tmp_path):
    """tests/cpp/test_crc_combine.cpp: lnx_crc32_combine and the .hpp delegate in
    a program of its own, the host sources compiled with ASan + UBSan."""
    exe = tmp_path / "test_crc_combine"
    subprocess.run(["g++", "-std=c++20", "-O1", "-g", "-Wall", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tests", "cpp", "test_crc_combine.cpp"),
                    os.path.join(ROOT, "lneto_amd", "csrc", "cpu_path.cpp"), "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    assert "ok" in r.stdout
