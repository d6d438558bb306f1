"""The host side of the receive ring's grouping (no GPU): tests/cpp/ring_group_host.cpp
runs lnxd::merge_groups and lnxd::group_records (lneto_amd/csrc/deliver_host.cpp)
against a stable sort of the whole call for 1, 2 and 7 internal batches, empty
batches, every frame in one bucket and every bucket hit once — once as a plain
g++ build that also links the library and checks the argument refusals of the
new entries that need no device, once under AddressSanitizer and UBSan with
nothing but the program itself loaded."""
import os
import subprocess

import lneto_amd as L

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "cpp", "ring_group_host.cpp")


def _run(exe):
    r = subprocess.run([str(exe)], capture_output=True, text=True)
    assert r.returncode == 0, (r.stdout + r.stderr)[-4000:]
    return r.stdout


def test_merge_and_refusals(tmp_path):
    exe = tmp_path / "ring_group_host"
    libdir = os.path.dirname(L.LIB_PATH)
    subprocess.run(["g++", "-std=c++17", "-O2", "-Wall", "-Wno-unknown-pragmas", SRC, "-o", str(exe), "-L", libdir,
                    "-llneto_amd", f"-Wl,-rpath,{libdir}"], check=True)
    out = _run(exe)
    assert "refusals: ok" in out and "every bucket once" in out and "FAIL" not in out
    assert sum(1 for line in out.splitlines() if line.endswith(" ok")) >= 12


def test_merge_under_sanitizers(tmp_path):
    exe = tmp_path / "ring_group_host_san"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-Wall", "-Wno-unknown-pragmas", "-DNO_LIBRARY",
                    "-fsanitize=address,undefined", "-fno-sanitize-recover=all", SRC, "-o", str(exe)], check=True)
    out = _run(exe)
    assert "every bucket once" in out and "FAIL" not in out and "refusals" not in out


def test_new_symbols_and_python_entries():
    for name in ("lnx_rx_verify_deliver_batch", "lnx_rx_ring_set_ports", "lnx_rx_ring_ingress_deliver",
                 "lnx_ingress_packets_deliver"):
        assert hasattr(L.lib, name), name
    assert callable(L.rx_verify_deliver_batch)
    for name in ("set_ports", "ingress_deliver", "ingress_packets_deliver"):
        assert callable(getattr(L.RxRing, name))
    # refused before any device call
    assert L.lib.lnx_rx_verify_deliver_batch(None, None, 5, 0, None, None, None, None, None, None, None, None, None) == L.LNX_EINVAL
    assert L.lib.lnx_rx_ring_ingress_deliver(None, 0, 1, 0, 0, None, None, None, None, None) == L.LNX_EINVAL
