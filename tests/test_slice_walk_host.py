"""The host-compilable part of the slice walk (no GPU): tests/cpp/slice_walk_host.cpp
runs lnx::slice_grid, lnx::slice_bounds and lnx::frame_len
(lneto_amd/csrc/slice_walk.hpp) for chunks of 256 frames under both grid caps
the kernels use, at and around every edge of the grid up to n = 2^32 - 1: the
grid size, the slices in order, disjoint and covering exactly [0, n), whole
chunks, nothing inverted past the end; and a frame's length from a reversed
pair of offsets, a span above 2^31 and a trim larger than the frame — once as a
plain g++ build, once under AddressSanitizer and UBSan with nothing but the
program itself loaded."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "slice_walk_host.cpp")
CASES = 2 * 10   # caps x sizes


@pytest.mark.parametrize("name,flags", [
    ("slice_walk_host", ["-O2"]),
    ("slice_walk_host_san", ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]),
])
def test_slices_and_frame_len(tmp_path, name, flags):
    exe = tmp_path / name
    subprocess.run(["g++", "-std=c++17", "-Wall", "-Wextra", "-Werror", *flags, SRC, "-o", str(exe)], check=True)
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    out = r.stdout
    assert "FAIL" not in out and "frame_len: ok" in out
    assert sum(1 for line in out.splitlines() if line.startswith("n ") and line.endswith(" ok")) == CASES
    assert "n 4294967295 cap 1024: G 1024 ok" in out and "n 0 cap 512: G 1 ok" in out
