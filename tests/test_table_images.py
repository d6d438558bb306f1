"""The staged, receive / transmit and search table images, checked on the host (no GPU).

lneto_amd/csrc/table_images.cpp builds the images the kernels read from HBM
at the offsets of lneto_amd/csrc/table_layout.hpp, which the kernels use too.
tests/cpp/table_images_host.cpp compiles the builders with plain g++ (no HIP,
no library) and applies every region the way its kernel does: each must give
Z_k of 4100 registers, each builder must return exactly the layout's total,
and every 32-column region must agree in all its columns.  A region that one
side moved, a wrong total or a fill into another region's span fails here
rather than as wrong CRCs on a GPU.  The program is built a second time with
AddressSanitizer and UBSan, as tests/test_frame_plan.py builds its program.
(The CRC rows' LDS images have tests/cpp/rows_emulator.cpp, tests/test_abi.py.)"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRCS = [os.path.join(ROOT, "tests", "cpp", "table_images_host.cpp"),
        os.path.join(ROOT, "lneto_amd", "csrc", "table_images.cpp")]


def _run(tmp_path_factory, name, *flags):
    exe = tmp_path_factory.mktemp(name) / name
    subprocess.run(["g++", "-std=c++17", "-Wall", *flags, *SRCS, "-o", str(exe)], check=True)
    return subprocess.run([str(exe)], capture_output=True, text=True)


@pytest.fixture(scope="module")
def plain_output(tmp_path_factory):
    r = _run(tmp_path_factory, "table_images_host", "-O2")
    assert r.returncode == 0, (r.stdout + r.stderr)[-2000:]
    return r.stdout


def test_every_region_gives_its_shift(plain_output):
    assert plain_output.startswith("ok: "), plain_output[-2000:]
    assert "4100 registers each" in plain_output


def test_table_images_under_sanitizers(plain_output, tmp_path_factory):
    """The same program with AddressSanitizer and UBSan: no fill and no lookup
    leaves its image, and the output is the unsanitized build's."""
    r = _run(tmp_path_factory, "table_images_host_san", "-O1", "-g", "-fsanitize=address,undefined",
             "-fno-sanitize-recover=all")
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    assert r.stdout == plain_output
