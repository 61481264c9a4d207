"""CPU: evaluate_subtable_mle for caller-defined tables as a device call (include/lasso_hip_mle.h, include/lasso_prover_mle.h).

  1. the two new headers declare exactly the four names, the two pinned headers none of them; both device and both prover libraries export them, the plain mock does
     not and Device.tables_mle over it says so;
  2. the accumulate / fold helper of the kernel (lasso_amd/csrc/mle_acc.cuh) as a stand-alone host program, plain and under -fsanitize=undefined, against Python big
     integers: entries 0, 1, 2^32 - 1, p - 1, representatives just below 2^254 + 2^130, runs of more than two fold periods of maximal terms;
  3. lasso_host_tables_mle(where = 0): every subtable of every built-in strategy restated as a descriptor against that built-in's closed form, random and Boolean points;
  4. the verifier's two routes (the device route through tests/cpp/mock_mle_wrap.cpp, the host loop) give the same verdicts, return codes and error texts on honest,
     bit-flipped and truncated bytes, and lasso_host_mle_stats counts the distinct subtables per verify on the device route and nothing on the host route;
  5. the sizes tests/test_gpu_mle.py runs reach both sides of the kernel's own boundaries, derived from the launch plan (tests/cpp/mle_plan_dump.cpp)."""
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

import customutil as U
import mleutil as M
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from lasso_amd.device import LassoError
from test_abi_exports import header_functions

ROOT = M.ROOT
DEVICE_NAMES = ["lasso_tables_mle", "lasso_tables_mle_dev"]
HOST_NAMES = ["lasso_host_mle_stats", "lasso_host_tables_mle"]
LAZY_BOUND = 2**254 + 2**130
CURVES = ["curve25519", "bn254"]


# ---- 1: headers and libraries

def test_new_headers_declare_exactly_the_four_names():
    assert header_functions("lasso_hip_mle.h") == DEVICE_NAMES
    assert header_functions("lasso_prover_mle.h") == HOST_NAMES
    pinned = set(header_functions("lasso_hip.h")) | set(header_functions("lasso_prover.h"))
    assert not pinned & set(DEVICE_NAMES + HOST_NAMES)


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_entries(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_mle(dev) == DEVICE_NAMES
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for n in HOST_NAMES:
        getattr(host, n)


def test_plain_mock_has_no_entry_and_the_binding_says_so():
    from gpuutil import load_mock
    from lasso_amd import Device
    mock = load_mock()
    assert not hasattr(mock, "lasso_tables_mle")
    d = Device(0, lib=mock)
    try:
        with pytest.raises(LassoError, match="does not export lasso_tables_mle"):
            d.tables_mle([np.zeros(4, dtype=np.uint32)], np.zeros((2, 4), dtype=np.uint64))
    finally:
        d.close()


# ---- 2: the accumulate / fold helper on the host

def _helper_exe(curve, san):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_mle_acc_host_{curve}{'_ubsan' if san else ''}")
    flags = (["-DLASSO_BN254"] if curve == "bn254" else []) + (["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"])
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mle_acc_host.cpp")])
    return exe


def _hex(v):
    return f"{v:064x}"


def _helper_cases(p):
    rng = np.random.default_rng(29)
    rand = lambda: int.from_bytes(rng.bytes(40), "little") % p
    top = (LAZY_BOUND - 1) // p * p            # the largest multiple of p below the lazy bound: every residue has a representative in [top - p, LAZY_BOUND)
    lazy = lambda v: v + (LAZY_BOUND - 1 - v) // p * p
    limbs_full = ((p - 1) >> 232 << 232) | (2**232 - 1)          # limbs 0..7 all 2^29 - 1, limb 8 as large as p allows
    if limbs_full >= p:
        limbs_full -= 1 << 232
    edge_e = [0, 1, p - 1, p - 2, 2**232 - 1, limbs_full]
    cases = []
    # u32: the edge entries against edge and random factor words, one term and many
    for lo in (1, p - 1, rand()):
        cases.append(("u32", lo, [(t, e) for t in (0, 1, 2**32 - 1) for e in edge_e + [rand()]]))
        cases.append(("u32", lo, [(2**32 - 1, p - 1)] * 50))                                    # more than three fold periods of maximal terms
        cases.append(("u32", lo, [(2**32 - 1, 2**232 - 1)] * 33))                               # every low limb of e maximal: the widest columns
        cases.append(("u32", lo, [(int(rng.integers(0, 2**32)), rand()) for _ in range(257)]))
    cases.append(("u32", rand(), []))
    cases.append(("u32", rand(), [(2**32 - 1, p - 1)] * 4096))                                  # a long run: column 9 only absorbs
    # Fr: field entries, canonical edges and representatives just below the lazy bound
    for lo in (1, p - 1, rand()):
        cases.append(("fr", lo, [(t, e) for t in (0, 1, p - 1, lazy(0), lazy(p - 1), LAZY_BOUND - 1, top) for e in edge_e[:4] + [rand()]]))
        cases.append(("fr", lo, [(LAZY_BOUND - 1, p - 1)] * 8))                                 # more than two fold periods (3) of maximal terms
        cases.append(("fr", lo, [(lazy(p - 1), p - 1)] * 100))
        cases.append(("fr", lo, [(lazy(rand()), rand()) for _ in range(200)]))
    cases.append(("fr", rand(), [(LAZY_BOUND - 1, p - 1)] * 4096))
    return cases


@pytest.mark.parametrize("san", [False, True], ids=["plain", "ubsan"])
@pytest.mark.parametrize("curve", CURVES)
def test_accumulate_and_fold_helper_against_big_integers(curve, san):
    p = FR_MODULUS[curve]
    cases = _helper_cases(p)
    text = "".join(f"{form} {_hex(lo)} {len(terms)}\n" + "".join((f"{t} " if form == "u32" else f"{_hex(t)} ") + _hex(e) + "\n" for t, e in terms) for form, lo, terms in cases)
    res = subprocess.run([_helper_exe(curve, san)], input=text, capture_output=True, text=True, timeout=120)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
    lines = res.stdout.strip().split("\n")
    assert len(lines) == len(cases) + 1
    u32_period, fr_period = map(int, lines[-1].split()[1:])
    assert max(len(t) for f, _, t in cases if f == "u32") >= 2 * u32_period and max(len(t) for f, _, t in cases if f == "fr") >= 2 * fr_period
    inv = pow(1 << 261, -1, p)
    for (form, lo, terms), line in zip(cases, lines):
        a = sum(t * e for t, e in terms)
        want_inner = a * inv % p
        got_inner, got_prod = (int(x, 16) for x in line.split())
        assert got_inner == want_inner, (form, len(terms))
        assert got_prod == want_inner * lo * inv % p, (form, len(terms))


# ---- 3: lasso_host_tables_mle(where = 0) against the closed forms

@pytest.fixture(scope="module")
def hosts():
    from lasso_amd.prover import HostProver
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = HostProver(C.CDLL(M.build_mock_prover_mle(curve)), curve=curve)
        return made[curve]
    yield get
    for h in made.values():
        h.close()


BUILTINS = [("and", 2, 6, 0), ("or", 2, 6, 0), ("xor", 3, 4, 0), ("lt", 2, 6, 0), ("range", 4, 4, 6), ("spark", 3, 5, 0)]


def _points(hp, log_m, p):
    one = (1 << 256) % p
    rnd = hp.gen_random_point(3 * log_m)
    pts = [rnd[:log_m], rnd[log_m:2 * log_m], rnd[2 * log_m:]]
    for bits in (0, (1 << log_m) - 1, 0b1011011011 & ((1 << log_m) - 1), 1, 1 << (log_m - 1)):
        pts.append(M.int_words([one if (bits >> (log_m - 1 - j)) & 1 else 0 for j in range(log_m)]))
    return pts


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind,c,log_m,log_r", BUILTINS)
def test_host_route_equals_the_closed_forms(hosts, curve, kind, c, log_m, log_r):
    hp = hosts(curve)
    p = FR_MODULUS[curve]
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    cs = U.builtin_as_custom(kind, c, log_m, log_r, curve, host=hp)
    for pt in _points(hp, log_m, p):
        closed = hp.tables_mle(S, pt)
        looped = hp.tables_mle(cs, pt, where=0)
        assert closed.shape == looped.shape == (cs.num_subtables, 4)
        assert np.array_equal(closed, looped)
        chi = M.chi_int(pt, p)
        assert M.word_ints(looped) == [M.mle_int(t, chi, p, cs.field) for t in cs.tables]          # ... and both equal the big-integer dot product
        assert np.array_equal(hp.tables_mle(cs, pt, where=1), looped)                              # the mock-backed device entry: the literal statement
    with pytest.raises(LassoError, match="log_m coordinates"):
        hp.tables_mle(cs, np.zeros((log_m + 1, 4), dtype=np.uint64))


def test_device_route_is_refused_without_the_entry():
    from lasso_amd.prover import HostProver
    hp = HostProver(C.CDLL(U.build_mock_prover_custom("curve25519")))
    try:
        cs = U.lte_strategy(2, 4)
        pt = hp.gen_random_point(4)
        assert hp.mle_stats() == {"device_tables": 0, "available": False}
        with pytest.raises(LassoError, match="lasso_tables_mle, include/lasso_hip_mle.h"):
            hp.tables_mle(cs, pt, where=1)
        assert hp.tables_mle(cs, pt, where=0).shape == (2, 4)
    finally:
        hp.close()


# ---- 4: the verifier's routes

SPECS = [{"make": "lte", "args": [2, 4]}, {"make": "field", "args": [2, 4, 5]}] + [{"make": "builtin", "args": list(b)} for b in
         [("and", 2, 4, 0), ("or", 1, 4, 0), ("xor", 2, 2, 0), ("lt", 2, 4, 0), ("range", 3, 4, 6), ("spark", 2, 4, 0)]]


@pytest.mark.parametrize("curve", CURVES)
def test_verifier_routes_agree_on_honest_tampered_and_truncated_bytes(curve):
    lib = M.build_mock_prover_mle(curve)
    devs = M.verify_in_child(lib, curve, SPECS, 40, {"LASSO_MLE_DEVICE_MIN": "0"})
    hosts_ = M.verify_in_child(lib, curve, SPECS, 40, {"LASSO_MLE_DEVICE_MIN": "0", "LASSO_VERIFY_DEVICE_MLE": "0"})       # a fresh process: its stats stay 0
    highs = M.verify_in_child(lib, curve, SPECS, 40, {"LASSO_MLE_DEVICE_MIN": str(1 << 20)})                              # the threshold keeps a small strategy on the host
    for spec, dev, host, high in zip(SPECS, devs, hosts_, highs):
        assert dev["proof"] == host["proof"] and dev["comm"] == host["comm"] and dev["available"] and host["available"]
        assert [r["name"] for r in dev["results"]] == [r["name"] for r in host["results"]] and len(dev["results"]) >= 13
        for a, b, c in zip(dev["results"], host["results"], high["results"]):
            assert a["verdict"] == b["verdict"] == c["verdict"], (spec, a, b, c)                       # verdict, return code and error text alike
            assert b["device_tables"] == 0 and c["device_tables"] == 0
            assert a["device_tables"] in (0, dev["distinct"])                                          # one call for all distinct subtables, or rejected before rand_mem
        assert dev["results"][0] == {"name": "honest", "verdict": True, "device_tables": dev["distinct"]}
        assert all(r["verdict"] is not True for r in dev["results"][1:]), spec
        assert dev["results"][-1] == {"name": "one table entry changed", "verdict": False, "device_tables": dev["distinct"]}, "the changed table was not caught by the device route's MLE"
        assert any(isinstance(r["verdict"], str) for r in dev["results"][1:]), "no variant exercised an error text"


# ---- 5: the GPU test's sizes reach the kernel's boundaries

def _plan(*strips):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "mle_plan_dump")
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "mle_plan_dump.cpp")])
    return [json.loads(l) for l in subprocess.check_output([exe, *map(str, strips)], text=True).strip().split("\n")]


def test_gpu_sizes_reach_both_sides_of_the_launch_plan_boundaries():
    rows = _plan(M.STRIP_TEST_LEN)
    whole = {r["log_m"]: r for r in rows if "log_m" in r and r["strip"] == 0}
    assert sorted(whole) == list(range(1, 31))
    for r in whole.values():
        assert r["hi_bits"] == (r["log_m"] + 1) // 2 and r["hi_bits"] + r["lo_bits"] == r["log_m"] and r["hi_bits"] <= 15
        assert r["nx"] <= r["max_nx_cap"] and r["nx"] * r["block"] >= r["tasks"] and r["rows_per_task"] * (r["tasks"] >> r["lo_bits"]) >= r["rows"] == 1 << r["hi_bits"]
    first_many = min(m for m, r in whole.items() if r["nx"] > 1)                         # one workgroup -> many
    first_runs = min(m for m, r in whole.items() if r["rows"] > r["rows_per_task"])      # one run of rows per column -> several: the workgroup tile's row extent
    for edge in (first_many, first_runs):
        assert edge - 1 in M.LOG_MS and edge in M.LOG_MS, (edge, M.LOG_MS)
    assert {1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 20} <= set(M.LOG_MS)
    assert whole[1]["lo_bits"] == 0 and whole[2]["lo_bits"] == 1                          # the degenerate factor tables: no variable, one variable
    src = open(os.path.join(ROOT, "lasso_amd", "csrc", "mle_acc.cuh")).read()
    period = max(int(re.search(r"#define MLE_FOLD_EVERY (\d+)u", src).group(1)), int(re.search(r"#define MLE_FR_FOLD_EVERY (\d+)u", src).group(1)))
    for m in M.FOLD_LOG_MS:                                                               # every lane of those shapes walks at least two fold periods of either form
        assert whole[m]["rows"] % whole[m]["rows_per_task"] == 0 and whole[m]["rows_per_task"] >= 2 * period
    strips = [r for r in rows if r.get("strip") == M.STRIP_TEST_LEN]
    assert len(strips) == 4 and strips[-1]["e1"] - strips[-1]["e0"] < M.STRIP_TEST_LEN     # a 2^10-entry table: three whole strips and a ragged one
    assert any(r["e0"] % (1 << r["lo_bits"]) for r in strips), "no strip begins inside a row"
    assert all(r["nx"] <= r["max_nx"] for r in strips)
    assert rows[-1] == {"strip_default_32_fr": 65536, "strip_default_1_u32": 16777216}     # 64 MiB of strips whatever the table count: the scratch bound the header states
