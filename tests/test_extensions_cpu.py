"""CPU: the optional parts of the device ABI are stated once per layer — the headers beside include/lasso_hip.h and include/lasso_prover.h, EXTS in
lasso_amd/host/prover_capi.cpp, lasso_amd/_abi.py EXTENSIONS / PROVER_EXTENSIONS, the fragments of tests/cpp/mock_device.cpp — and the layers agree:
  1. the Python tables are the headers, and the product libraries export every function of them (dlopen / dlsym only, no GPU call);
  2. for each extension: absent from the device library it is reported unavailable and the binding refuses in its own words, present it is reported available;
  3. two extensions in one mock: a proof verified with the device decoder AND the table-free MSM, each counted, with the plain mock's verdict;
  4. every mock variant is rebuilt when any host header changes."""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import mockbuild
from lasso_amd import Device, LassoError, _abi
from lasso_amd.prover import HostProver
from test_abi_exports import ROOT, header_functions


# ---- 1. the registry is the headers

@pytest.fixture(scope="module")
def product():
    import __graft_entry__ as g
    g.build()
    return lambda stem, suffix: C.CDLL(os.path.join(ROOT, "lasso_amd", f"{stem}{suffix}.so"))


@pytest.mark.parametrize("stem,table", [("liblasso_hip", _abi.EXTENSIONS), ("liblasso_prover", _abi.PROVER_EXTENSIONS)], ids=["device", "prover"])
def test_tables_are_the_optional_headers(product, stem, table):
    prefix = stem[3:] + "_"
    assert sorted(h for h, _ in table.values()) == sorted(f for f in os.listdir(os.path.join(ROOT, "include")) if f.startswith(prefix)), "an optional header without a row, or a row without a header"
    for name, (header, sig) in table.items():
        assert header_functions(header) == sorted(sig), name
        for suffix in ("", "_bn254"):
            assert _abi.declare_ext(product(stem, suffix), name, table) == sorted(sig)          # AttributeError = declared but not exported


def test_host_table_has_the_same_rows():
    """EXTS in prover_capi.cpp: the names and headers of _abi.EXTENSIONS in the same order, and the entry a refusal names is a function of that header"""
    src = open(os.path.join(ROOT, "lasso_amd", "host", "prover_capi.cpp")).read()
    rows = re.findall(r'^  \{"(\w+)", "(lasso_hip_\w+\.h)", "[^"]+", "(lasso_\w+)", \[\]', src, flags=re.M)
    assert [(n, h) for n, h, _ in rows] == [(n, h) for n, (h, _) in _abi.EXTENSIONS.items()]
    assert all(entry in _abi.EXTENSIONS[n][1] for n, _, entry in rows)
    assert sorted(mockbuild.EXTS) == sorted([*_abi.EXTENSIONS, "custom"])
    for e in mockbuild.EXTS:
        assert os.path.exists(os.path.join(mockbuild.CPP, f"mock_{e}_wrap.cpp")) and f"MOCK_EXT_{e.upper()}\n" in open(os.path.join(mockbuild.CPP, "mock_device.cpp")).read()


# ---- 2. absent means refused, present means taken

_lay = _abi.OperandLayout(2, 2, 0)
_none = np.zeros((0, 4), dtype=np.uint64)
# extension -> (HostProver's stats method, its availability key, a Device call that needs the extension, the refusal's text)
CASES = {
    "wire": ("wire_stats", "device_available", lambda d: d.points_decompress(b""), "this device library does not export lasso_points_decompress (include/lasso_hip_wire.h)"),
    "msm_points": ("msm_stats", "available", lambda d: d.msm_points(np.zeros((0, 8), dtype=np.uint64), _none), "this device library does not export lasso_msm_points (include/lasso_hip_msm.h)"),
    "operands": ("densify_stats", "available", lambda d: d.densify_dim_operands(0, None, 0, _lay, 1, 0, 1, 4, 0, 0, 0, 0),
                 "this device library does not export lasso_densify_dim_operands (include/lasso_hip_operands.h)"),
    "gens": ("gens_stats", "available", lambda d: d.points_from_candidates(_none, []), "this device library does not export lasso_points_from_candidates (include/lasso_hip_gens.h)"),
    "mle": ("mle_stats", "available", lambda d: d.tables_mle([], _none), "this device library does not export lasso_tables_mle (include/lasso_hip_mle.h)"),
    "values": ("values_stats", "available", lambda d: d.lookup_values(None, [], [], False, 0, _abi.VALUES_FR, 0), "this device library does not export lasso_lookup_values (include/lasso_hip_values.h)"),
    "poly": ("poly_stats", "available", lambda d: d.u64_or(0, 0), "this device library does not export lasso_matvec_left_u64_dev (include/lasso_hip_poly.h)"),
}


def _mock(curve, ext):
    lib = C.CDLL(mockbuild.build_mock_prover(curve, ext=ext))
    _abi.declare(lib)          # the mock prover exports the device ABI it was linked with
    return lib


@pytest.mark.parametrize("curve,name", [("curve25519", n) for n in CASES] + [("bn254", "wire")])
def test_absent_is_refused_and_present_is_reported(curve, name):
    assert list(CASES) == list(_abi.EXTENSIONS)
    stats, key, call, text = CASES[name]
    without, with_only = _mock(curve, ()), _mock(curve, (name,))
    hp = HostProver(without, curve=curve)
    try:
        got = getattr(hp, stats)()
        assert got[key] is False and all(v == 0 for k, v in got.items() if k != key)
    finally:
        hp.close()
    dev = Device(lib=without)
    with pytest.raises(LassoError) as e:
        call(dev)
    assert str(e.value) == text
    dev.close()
    hp = HostProver(with_only, curve=curve)
    try:
        assert getattr(hp, stats)()[key] is True
        for other in set(CASES) - set(mockbuild.closure([name])):          # and nothing else came with it
            assert getattr(hp, CASES[other][0])()[CASES[other][1]] is False, other
    finally:
        hp.close()
    assert Device(lib=with_only)._ext(name) is with_only


# ---- 3. two extensions at once.  argv: repository root, the mock with wire and msm_points, the plain mock.  One JSON line: verdicts of the honest proof and of one with
# a flipped commitment-row bit from both libraries, and the first library's counters after the honest verification.
CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import _abi
from lasso_amd.prover import HostProver
both, plain = (HostProver(C.CDLL(p)) for p in sys.argv[2:4])
c, log_m, s = 1, 4, 16
idx = np.random.default_rng(5).integers(0, 1 << log_m, size=(s, c), dtype=np.uint64)
S = _abi.Strategy(_abi.KINDS["and"], c, log_m, 0)
r = plain.gen_random_point(4)
gens = plain.gens(c, s, c, log_m); dense = plain.densify(idx, log_m)
comm = plain.commit(dense, gens); proof = plain.prove(dense, gens, S, r)
bad = bytearray(comm); bad[8 + 2] ^= 0x10
out = {}
for name, hp in (("both", both), ("plain", plain)):
    g = hp.gens(c, s, c, log_m)
    out[name] = [hp.verify(g, S, s, r, proof, comm)]
    out[name + "_stats"] = [hp.wire_stats(), hp.msm_stats()]
    try:
        out[name].append(hp.verify(g, S, s, r, proof, bytes(bad)))
    except Exception as e:
        out[name].append(str(e))
print(json.dumps(out))
"""


def test_decoder_and_table_free_msm_in_one_verification():
    """AND, C = 1, log_m = 4, 2^4 lookups.  LASSO_WIRE_DEVICE_MIN (read once per process; its default keeps so small a batch on the host) is set for the child."""
    both, plain = mockbuild.build_mock_prover(ext=("wire", "msm_points")), mockbuild.build_mock_prover()
    env = dict(os.environ, LASSO_WIRE_DEVICE_MIN="1")
    for k in ("LASSO_VERIFY_DEVICE_POINTS", "LASSO_VERIFY_MSM_POINTS"):
        env.pop(k, None)
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, both, plain], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    out = json.loads(res.stdout.strip().split("\n")[-1])
    wire, msm = out["both_stats"]
    assert wire["device_available"] and wire["device_points"] > 0 and msm["available"] and msm["points_calls"] > 0
    assert out["plain_stats"] == [{"device_points": 0, "device_available": False}, {"points_calls": 0, "available": False}]
    assert out["both"] == out["plain"] and out["both"][0] is True and out["both"][1] is not True


# ---- 4. the builder rebuilds when it should

def test_every_variant_depends_on_every_host_header(tmp_path):
    """inputs() is one list for every variant (build_mock_prover passes it no variant), and holds what the hand-kept lists had lost"""
    rel = [os.path.relpath(f, ROOT) for f in mockbuild.inputs()]
    for f in ("lasso_amd/host/verifier.hpp", "lasso_amd/host/switches.hpp", "lasso_amd/host/prover.hpp", "lasso_amd/host/prover_capi.cpp", "oracle/mock_hip.cpp", "oracle/lasso_oracle.hpp",
              "lasso_amd/csrc/fe29.cuh", "include/lasso_hip.h", "include/lasso_custom_check.h", "tests/cpp/mock_device.cpp", "tests/cpp/slab_threads.cpp",
              *(f"tests/cpp/mock_{e}_wrap.cpp" for e in mockbuild.EXTS), *(f"include/{h}" for t in (_abi.EXTENSIONS, _abi.PROVER_EXTENSIONS) for h, _ in t.values())):
        assert f in rel, f
    # the same function over a copy of the tree's layout: a library goes stale when verifier.hpp is touched
    hdr = tmp_path / "lasso_amd" / "host" / "verifier.hpp"
    hdr.parent.mkdir(parents=True)
    hdr.write_text("")
    so = tmp_path / "lib.so"
    so.write_text("")
    assert mockbuild.inputs(str(tmp_path)) == [str(hdr)]
    os.utime(hdr, (1000, 1000)); os.utime(so, (2000, 2000))
    assert not mockbuild.stale(str(so), mockbuild.inputs(str(tmp_path)))
    os.utime(hdr, (3000, 3000))
    assert mockbuild.stale(str(so), mockbuild.inputs(str(tmp_path)))
    assert mockbuild.stale(str(tmp_path / "missing.so"), [])
