"""One declaration per cross-file function of lneto_amd/csrc (no GPU).

launch.hpp and host_path.hpp declare every function that one csrc file defines
and another calls, and each defining file includes its header, so a drifted
type is a compile error.  C++ does not compare parameter NAMES, though: two
parameters of one type swapped in the definition alone (capacity and flags of
launch_tx_finish) still compile and link.  So here the parameter list of every
declaration must be the definition's, names and order included, the default
arguments must stand in the header only, and no other file may carry a
prototype of its own."""
import glob
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "lneto_amd", "csrc")
HEADERS = ("launch.hpp", "host_path.hpp")
FUNC = r"^(?:hipError_t|uint64_t|uint8_t|int) (\w+)\(([^;{}]*)\)\s*%s"


def _sources():
    paths = [p for pat in ("*.hip", "*.cpp", "*.hpp", "*.inc", "research/*") for p in glob.glob(os.path.join(CSRC, pat))]
    return {os.path.relpath(p, CSRC): open(p).read() for p in sorted(set(paths))}


def _params(text, keep_defaults=False):
    out = []
    for p in text.split(","):
        p = " ".join(p.split())
        out.append(p if keep_defaults else re.sub(r"\s*=.*$", "", p))
    return out


def test_declarations_match_their_definitions():
    src = _sources()
    decls = {}
    for h in HEADERS:
        for name, params in re.findall(FUNC % ";", src[h], re.M):
            assert name not in decls, name
            decls[name] = params
    assert len(decls) >= 30 and {"launch_tx_finish", "launch_ingress_verify", "host_fcs_ok", "device_resources"} <= set(decls)
    defs = {}
    for path, text in src.items():
        for name, params in re.findall(FUNC % r"\{", text, re.M):
            if name in decls:
                assert name not in defs, (name, path, defs[name][0])
                defs[name] = (path, params)
    assert set(defs) == set(decls), sorted(set(decls) ^ set(defs))
    for name, (path, params) in defs.items():
        assert "=" not in params, f"{path}: {name} repeats a default argument"
        assert _params(params) == _params(decls[name]), f"{path}: {name} differs from its declaration"
        hdr = "host_path.hpp" if name.startswith("host_") else "launch.hpp"
        assert re.search(r'#include "(\.\./)?%s"' % re.escape(hdr), src[path]), f"{path} does not include {hdr}"


def test_no_prototype_outside_the_headers():
    for path, text in _sources().items():
        if path in HEADERS:
            continue
        protos = [n for n, _ in re.findall(FUNC % ";", text, re.M)
                  if n.startswith(("launch_", "host_")) or n in ("deliver_ws_bytes", "device_resources", "hip_error")]
        assert not protos, (path, protos)
