"""CPU: the MSM over caller points (include/lasso_hip_msm.h, lasso_host_msm_points) and the verifier's use of it.
  * the verifier's table-free path (lasso_msm_points resolved through tests/cpp/mock_msm_points_wrap.cpp) against the plain mock's lasso_bases_create + lasso_msm path:
    the same verdict, return code and error text on honest, tampered, swapped and truncated bytes of every built-in strategy's proof; lasso_host_msm_stats proves which
    path ran (one MSM over commitment rows per opening, four openings per proof; 0 with LASSO_VERIFY_MSM_POINTS=0, in a fresh process);
  * msmp_digit (lasso_amd/csrc/msm_points_recode.cuh: what one lane of k_msmp_prepare runs), compiled for the host, against Python big integers;
  * the symbols: both device libraries export the two entry points, include/lasso_hip.h does not declare them, and a device library without them is reported as such."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import msmutil as M
import wireutil as W
from fieldref import L as FR_P
from lasso_amd import _abi
from lasso_amd.device import LassoError
from proverutil import HostProver, build_mock_prover
from test_verifier_cpu import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]
ORDER = {"curve25519": 2**252 + 27742317777372353535851937790883648493, "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617}
OPENINGS = 4      # PolyEvalProofs per proof: proof_derefs (surge.rs) and open_ops, open_mem, open_derefs (memory_checking.rs HashLayerProof), each with one C_LZ = <L, C>
LAZY_BOUND = 2**254 + 2**130      # include/lasso_hip.h: lazily reduced arrays hold representatives below this bound


# ---------------------------------------------------------------- symbols and headers

def _header_functions(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", src)))


def test_msm_header_is_separate_from_the_device_header():
    assert _header_functions("lasso_hip_msm.h") == ["lasso_msm_points", "lasso_msm_points_dev"]
    assert not {"lasso_msm_points", "lasso_msm_points_dev"} & set(_header_functions("lasso_hip.h"))
    assert {"lasso_host_msm_points", "lasso_host_msm_stats"} <= set(_header_functions("lasso_prover.h"))


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_msm_over_points(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_msm_points(dev) == _header_functions("lasso_hip_msm.h")      # AttributeError = not exported
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for name in ("lasso_host_msm_points", "lasso_host_msm_stats"):
        getattr(host, name)


def test_the_mock_of_the_device_header_has_no_msm_over_points():
    from gpuutil import load_mock
    from lasso_amd.device import Device
    mock = load_mock()
    with pytest.raises(AttributeError):
        _abi.declare_msm_points(mock)
    dev = Device(lib=mock)
    with pytest.raises(LassoError, match="does not export lasso_msm_points"):
        dev.msm_points(np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))
    dev.close()


# ---------------------------------------------------------------- the recoding

def _recode_values(curve, c):
    r = ORDER[curve]
    vals = [0, 1, 2**c // 2 - 1, 2**c // 2, r - 1, r - 2, 2**252, 2**252 - 1, LAZY_BOUND - 1, 2**256 - 1, 2**255, 2**c - 1, 2**c, 2**253 - 1]
    rng = np.random.default_rng(20 + c)
    vals += [int.from_bytes(rng.bytes(32), "little") >> int(rng.integers(0, 200)) for _ in range(200)]
    return vals


@pytest.mark.parametrize("flags,tag", [(["-O2"], "plain"), (["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"], "ubsan")])
def test_digit_recoding_against_big_integers(flags, tag):
    """sum_w d_w 2^(c w) == k with every digit in [-2^(c-1), 2^(c-1) - 1] and no carry out of the last window, for the width the kernels are built with and for every
    other width of the design range 8 .. 12; a stand-alone host program (its own main), under UBSan too"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_msm_points_recode_{tag}")
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_msm_points_recode_host.cpp")])
    widths = [8, 9, 10, 11, 12]
    vals = sorted({v for curve in CURVES for c in widths for v in _recode_values(curve, c)})
    path = os.path.join(out_dir, f"msm_points_recode_{tag}.hex")
    with open(path, "w") as f:
        f.write("".join(v.to_bytes(32, "little").hex() + "\n" for v in vals))
    res = subprocess.run([exe, path, *map(str, widths)], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    lines = res.stdout.strip().split("\n")
    assert lines[-1] == f"OK {len(vals)}"
    built = int(lines[0].split()[1])
    assert lines[0].startswith("C ") and built in widths      # the width the kernels instantiate is among those checked
    rows = lines[1:-1]
    assert len(rows) == len(vals) * len(widths)
    for i, v in enumerate(vals):
        for j, c in enumerate(widths):
            got = [int(x) for x in rows[i * len(widths) + j].split()]
            assert got[0] == c
            d = got[1:]
            assert len(d) == (256 + c) // c
            assert all(-(2**(c - 1)) <= x <= 2**(c - 1) - 1 for x in d), (v, c)
            assert sum(x << (c * w) for w, x in enumerate(d)) == v, (v, c)


# ---------------------------------------------------------------- the verifier: table-free path == table path

def _proof_case(hp, kind, c, log_m, log_r, lookups, seed=5):
    s = 1 << max((lookups - 1).bit_length(), 0)
    alpha = 2 * c if kind == "lt" else c
    idx = np.random.default_rng(seed + lookups).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = hp.gen_random_point(max(s.bit_length() - 1, 0))
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = hp.gens(c, s, alpha, log_m)
    dense = hp.densify(idx, log_m)
    comm = hp.commit(dense, gens)
    proof = hp.prove(dense, gens, S, r)
    hp.free(dense)
    return {"s": s, "r": r, "S": S, "gens": gens, "comm": comm, "proof": proof, "alpha": alpha, "c": c}


@pytest.fixture(scope="module", params=CURVES)
def libs(request):
    """per curve: the plain mock build (no lasso_msm_points: today's path) and the wrapped build (the weak reference resolves: the table-free path)"""
    curve = request.param
    plain = HostProver(C.CDLL(build_mock_prover(curve)))
    wrapped = HostProver(C.CDLL(M.build_mock_prover_msm(curve)))
    yield curve, plain, wrapped
    plain.close(); wrapped.close()


def _outcome(hp, gens, pc, proof, comm):
    """True / False, or the error exactly as the C ABI reports it (return code and lasso_host_last_error text)"""
    try:
        return hp.verify(gens, pc["S"], pc["s"], pc["r"], proof, comm)
    except LassoError as e:
        return str(e)


@pytest.mark.parametrize("case", CASES, ids=[f"{c[0]}-c{c[1]}-m{c[2]}-s{c[4]}" for c in CASES])
def test_table_free_verifier_equals_table_verifier(libs, case):
    curve, plain, wrapped = libs
    pc = _proof_case(plain, *case)
    gens_w = wrapped.gens(case[1], pc["s"], pc["alpha"], case[2])

    def same(proof, comm, what):
        a, b = _outcome(plain, pc["gens"], pc, proof, comm), _outcome(wrapped, gens_w, pc, proof, comm)
        assert a == b, f"{what}: table path {a!r}, table-free path {b!r}"
        return a

    try:
        proof, comm = pc["proof"], pc["comm"]
        pts, scs = W.walk_proof(proof, pc["alpha"], pc["c"])
        cpts = W.commitment_points(comm)
        assert plain.msm_stats() == {"points_calls": 0, "available": False}
        wrapped.msm_stats(reset=True)
        assert same(proof, comm, "honest") is True
        assert wrapped.msm_stats() == {"points_calls": OPENINGS, "available": True}      # one C_LZ = <L, C> per opening
        assert plain.msm_stats()["points_calls"] == 0
        # a bit flipped in commitment rows
        seen = []
        for j, o in enumerate(cpts[:: len(cpts) // 6 + 1]):
            bit = (29 * j + 7) % 256
            badc = bytearray(comm); badc[o + bit // 8] ^= 1 << (bit % 8)
            seen.append(same(proof, bytes(badc), f"commitment row at {o} bit {bit}"))
        # (a flip may land on an encoding ark-serialize reads as the same point — the x bits of a BN254 identity row, DESIGN 3.1 — and then BOTH paths accept)
        assert any(v is not True for v in seen), seen
        # ... in L points of the three openings (the proof's last points are open_derefs' L, R, delta, beta; L_vec / R_vec sit between the length prefixes)
        for j, o in enumerate(pts[:: len(pts) // 8 + 1]):
            bit = (37 * j + 251) % 256
            bad = bytearray(proof); bad[o + bit // 8] ^= 1 << (bit % 8)
            same(bytes(bad), comm, f"point at {o} bit {bit}")
        # ... in scalars
        for j, o in enumerate(scs[:: len(scs) // 8 + 1]):
            bit = (61 * j + 3) % 256 if j % 2 else 255
            bad = bytearray(proof); bad[o + bit // 8] ^= 1 << (bit % 8)
            assert same(bytes(bad), comm, f"scalar at {o} bit {bit}") is not True
        # two commitment rows swapped
        if len(cpts) >= 2:
            a, b = cpts[0], cpts[1]
            badc = bytearray(comm); badc[a:a + 32], badc[b:b + 32] = comm[b:b + 32], comm[a:a + 32]
            if bytes(badc) != comm:
                assert same(proof, bytes(badc), "swapped rows") is not True
        # truncated proof and commitment
        for cut in sorted({8, 39, pts[-1] + 5, scs[len(scs) // 2] + 11, len(proof) - 1}):
            if 0 < cut < len(proof):
                assert isinstance(same(proof[:cut], comm, f"proof cut at {cut}"), str)
        assert isinstance(same(proof, comm[:-1], "commitment cut"), str)
        assert same(proof, comm, "honest again") is True
    finally:
        plain.free(None, pc["gens"]); wrapped.free(None, gens_w)


@pytest.mark.parametrize("curve", CURVES)
def test_switch_off_keeps_the_table_path(curve):
    """LASSO_VERIFY_MSM_POINTS is read once per process: a fresh child per setting, on the wrapped build"""
    lib = M.build_mock_prover_msm(curve)
    case = ("and", 2, 4, 0, 16)
    on = M.verify_in_child(lib, curve, case, {"LASSO_VERIFY_MSM_POINTS": "1"})
    off = M.verify_in_child(lib, curve, case, {"LASSO_VERIFY_MSM_POINTS": "0"})
    assert on["honest"] is True and off["honest"] is True
    assert on["stats_honest"] == {"points_calls": OPENINGS, "available": True}
    assert off["stats_honest"] == {"points_calls": 0, "available": True} and off["stats_both"]["points_calls"] == 0
    assert on["tampered"] is not True and on["tampered"] == off["tampered"]
    assert on["proof"] == off["proof"] and on["comm"] == off["comm"]


# ---------------------------------------------------------------- the public entry point

def test_host_entry_point_reports_a_missing_device_entry_and_matches_the_table_path(libs):
    curve, plain, wrapped = libs
    pts = plain.gens_points(plain.gens(1, 16, 1, 4), 0)
    n = pts.shape[0]
    rng = np.random.default_rng(4)
    sc = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64); sc[:, 3] &= np.uint64(2**60 - 1)
    with pytest.raises(LassoError, match="not available"):
        plain.msm_points(pts, sc)
    got = wrapped.msm_points(pts, sc)
    # the same sum through the generators' own tables of the mock device: bases_create + msm, compressed by the oracle
    from gpuutil import compress_points
    from lasso_amd.device import Device
    lib = C.CDLL(os.path.join(ROOT, "oracle", "libmock_hip_bn254.so" if curve == "bn254" else "libmock_hip.so"))
    _abi.declare(lib)
    lib.mock_point_compress.argtypes = [C.c_void_p, C.c_void_p]; lib.mock_point_on_curve.argtypes = [C.c_void_p]; lib.mock_point_on_curve.restype = C.c_int
    dev = Device(lib=lib)
    b = dev.bases_create(pts)
    assert got == compress_points(lib, dev.msm(b, sc))[0]
    # an all-zero entry is the identity; n = 0 and all-skipped give the identity, which is also 0 * P
    half = pts.copy(); half[::2] = 0
    sc0 = sc.copy(); sc0[::2] = 0
    assert wrapped.msm_points(half, sc) == compress_points(lib, dev.msm(b, sc0))[0]
    ident = compress_points(lib, dev.msm(b, np.zeros_like(sc)))[0]
    assert wrapped.msm_points(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)) == ident
    assert wrapped.msm_points(np.zeros_like(pts), sc) == ident
    dev.bases_destroy(b); dev.close()
