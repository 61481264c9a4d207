"""CPU: label-derived generators with the candidates' arithmetic behind the device ABI (include/lasso_hip_gens.h, lasso_host_points_from_candidates, the device
route of lasso_host_gens_new).
  * pt_from_candidate (lasso_amd/csrc/fe29.cuh, bn254_fe29.cuh: what one lane of k_points_from_candidates runs), compiled for the host, against the host prover's own
    point_from_candidate inside a stand-alone program (tests/cpp/test_gens_host.cpp: 64- and 32-bit limb forms, under UBSan), and both against a big-integer statement
    written from ark-ec's rules (tests/gensutil.py) on crafted candidates and on the first 2000 candidates of the label's stream — the stream itself held to an
    independent statement of SHAKE256 / ChaCha20 / Fq::rand;
  * lasso_host_gens_new through a mock that has the entry (tests/cpp/mock_gens_wrap.cpp: the device route on the CPU) against the plain mock's host route and against
    the oracle's own generators: the three sets byte for byte, commitment and proof bytes, the counter, the switches (in child processes: they are read once);
  * the symbols: both device libraries export lasso_points_from_candidates, include/lasso_hip.h does not declare it, and a device library without it is reported as such."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

import gensutil as G
from lasso_amd import _abi
from lasso_amd.device import LassoError
from proverutil import HostProver, build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]
SHAPES = [(1, 1 << 4, 1, 4), (4, 1 << 10, 4, 8), (2, 1 << 12, 4, 8)]      # (c, s, memories, log_m)
STREAM = 2000


# ---------------------------------------------------------------- symbols and headers

def _header_functions(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", src)))


def test_gens_header_is_separate_from_the_device_header():
    assert _header_functions("lasso_hip_gens.h") == ["lasso_points_from_candidates"]
    assert "lasso_points_from_candidates" not in _header_functions("lasso_hip.h")
    assert {"lasso_host_points_from_candidates", "lasso_host_gens_stats"} <= set(_header_functions("lasso_prover.h"))


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_entry(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_gens(dev) == _header_functions("lasso_hip_gens.h")      # AttributeError = not exported
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for name in ("lasso_host_points_from_candidates", "lasso_host_gens_stats"):
        getattr(host, name)


def test_the_mock_of_the_device_header_has_no_such_entry():
    from gpuutil import load_mock
    with pytest.raises(AttributeError):
        _abi.declare_gens(load_mock())


# ---------------------------------------------------------------- the arithmetic

def _run_host_program(curve, flags, tag):
    """tests/cpp/test_gens_host.cpp on the crafted candidates and the first STREAM candidates of the label: (crafted results, stream rows); the program itself has
    compared pt_from_candidate with point_from_candidate on every one of them (exit status 1 on a difference)"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_gens_host_{curve}_{tag}")
    cflags = ["-DLASSO_BN254"] if curve == "bn254" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *cflags, *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_gens_host.cpp")])
    cases = G.crafted(curve)
    path = os.path.join(out_dir, f"gens_candidates_{curve}_{tag}.txt")
    with open(path, "w") as f:
        f.write("".join(f"{v.to_bytes(32, 'little').hex()} {g}\n" for _, v, g, _ in cases))
    res = subprocess.run([exe, path, str(STREAM), G.LABEL.decode()], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    lines = res.stdout.strip().split("\n")
    assert lines[-1].startswith(f"OK {len(cases)} {STREAM} ")
    crafted = [(int(s), bytes.fromhex(a)) for s, a in (ln.split() for ln in lines[:len(cases)])]
    stream = [ln.split()[1:] for ln in lines[len(cases):-1]]
    assert len(stream) == STREAM
    return crafted, stream


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("flags,tag", [(["-O2"], "limbs64"), (["-O2", "-DLASSO_HOST_LIMBS32"], "limbs32"), (["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"], "ubsan")])
def test_candidate_arithmetic_against_host_and_big_integers(curve, flags, tag):
    """status and affine limbs of pt_from_candidate == point_from_candidate's (inside the program) == the big-integer statement's, on every crafted candidate and on the
    stream's first 2000; the stream is the one the independent statement draws; under UBSan no limb or column leaves its container on the way"""
    crafted, stream = _run_host_program(curve, flags, tag)
    for (name, v, g, st), got in zip(G.crafted(curve), crafted):
        assert got == G.from_candidate(curve, v, g), name
        assert got[0] == st, name      # the reference itself gives the status the case was crafted for
    limbs, greatest = G.stream_candidates(curve, STREAM)
    ok = 0
    for i, (lhex, g, st, ahex) in enumerate(stream):
        assert (bytes.fromhex(lhex), int(g)) == (limbs[i].tobytes(), int(greatest[i])), f"stream candidate {i}"
        if tag == "limbs64" or i < 200:      # the big-integer statement costs a millisecond per candidate: all of them once, a prefix in the other builds
            assert (int(st), bytes.fromhex(ahex)) == G.from_candidate(curve, G.limbs_int(limbs[i]), int(g)), f"stream candidate {i}"
        ok += int(st) == G.OK
    assert 0.4 * STREAM < ok < 0.6 * STREAM      # half of the candidates carry a point


# ---------------------------------------------------------------- the host library: device route == host route == oracle

@pytest.fixture(scope="module", params=CURVES)
def libs(request):
    """per curve: the plain mock build (no device entry: the host route) and the wrapped build (entry present; threshold 1 so that the smallest sets take the device route)"""
    curve = request.param
    old = os.environ.get("LASSO_GENS_DEVICE_MIN")
    os.environ["LASSO_GENS_DEVICE_MIN"] = "1"       # read once per library, at its first generator set
    plain = HostProver(C.CDLL(build_mock_prover(curve)))
    wired = HostProver(C.CDLL(G.build_mock_prover_gens(curve)))
    yield curve, plain, wired
    plain.close(); wired.close()
    if old is None:
        os.environ.pop("LASSO_GENS_DEVICE_MIN", None)
    else:
        os.environ["LASSO_GENS_DEVICE_MIN"] = old


@pytest.mark.parametrize("shape", SHAPES, ids=[f"c{c}-s{s}-mem{m}-m{lm}" for c, s, m, lm in SHAPES])
def test_sets_do_not_depend_on_the_route_and_equal_the_oracle(libs, shape):
    curve, plain, wired = libs
    oracle = G.load_oracle(curve)
    gp, gw = plain.gens(*shape), wired.gens(*shape)
    before = wired.gens_stats()["device_candidates"]
    try:
        gw2 = wired.gens(*shape)
        drawn = wired.gens_stats()["device_candidates"] - before
        sets_p = [plain.gens_points(gp, w) for w in range(3)]
        sets_w = [wired.gens_points(gw, w) for w in range(3)]
        largest = max(a.shape[0] for a in sets_p)
        assert 2 * largest <= drawn      # at least two candidates per point went through the device entry
        want = G.oracle_gens(oracle, largest)
        for w in range(3):
            assert sets_p[w].tobytes() == sets_w[w].tobytes() == wired.gens_points(gw2, w).tobytes(), f"set {w}"
            n = sets_p[w].shape[0]
            assert np.array_equal(sets_p[w], want[:n]), f"set {w} against the oracle"      # every set is a prefix of the one stream
        assert plain.gens_stats() == {"device_candidates": 0, "available": False}
        assert wired.gens_stats()["available"] is True
    finally:
        plain.free(None, gp); wired.free(None, gw); wired.free(None, gw2)


@pytest.mark.parametrize("kind,c,log_m,lookups", [("and", 4, 4, 16), ("lt", 4, 4, 16)])
def test_commitment_and_proof_bytes_do_not_depend_on_the_route(libs, kind, c, log_m, lookups):
    curve, plain, wired = libs
    s = lookups
    alpha = 2 * c if kind == "lt" else c
    idx = np.random.default_rng(3).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
    got = []
    for hp in (plain, wired):
        before = hp.gens_stats()["device_candidates"]
        r = hp.gen_random_point(s.bit_length() - 1)
        gens = hp.gens(c, s, alpha, log_m); dense = hp.densify(idx, log_m)
        comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, S, r)
        assert hp.verify(gens, S, s, r, proof, comm) is True
        got.append((comm, proof, hp.gens_stats()["device_candidates"] - before))
        hp.free(dense, gens)
    assert got[0][:2] == got[1][:2]
    assert got[0][2] == 0 and got[1][2] > 0


def test_host_entry_point_equals_reference_and_wrapped_device_path(libs):
    """lasso_host_points_from_candidates: where = 0 (the host's point_from_candidate) == the big-integer statement == where = 1 through the wrapped mock (the product's
    pt_from_candidate); NULL out is allowed; the counter counts where = 1 only; the plain mock says that the entry is missing"""
    curve, plain, wired = libs
    limbs, greatest = G.batch(curve, 120, seed=1)
    a_ref, s_ref = G.reference(curve, limbs, greatest)
    assert set(int(x) for x in s_ref) == {G.OK, G.NONCANONICAL, G.NO_POINT}
    a0, s0 = plain.points_from_candidates(limbs, greatest, where=0)
    assert np.array_equal(s0, s_ref) and np.array_equal(a0, a_ref)
    before = wired.gens_stats()["device_candidates"]
    a1, s1 = wired.points_from_candidates(limbs, greatest, where=1)
    assert np.array_equal(s1, s_ref) and np.array_equal(a1, a_ref)
    assert wired.gens_stats() == {"device_candidates": before + 120, "available": True}
    st = np.zeros(120, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    g8 = np.ascontiguousarray(greatest, dtype=np.uint8)
    wired._chk(wired.lib.lasso_host_points_from_candidates(wired.h, vp(limbs), vp(g8), 120, 1, None, vp(st)))
    assert np.array_equal(st, s_ref)
    assert wired.points_from_candidates(np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint8), where=1)[1].shape == (0,)
    with pytest.raises(LassoError, match="not available"):
        plain.points_from_candidates(limbs[:1], greatest[:1], where=1)
    assert plain.gens_stats() == {"device_candidates": 0, "available": False}


@pytest.mark.parametrize("curve", CURVES)
def test_switches_in_child_processes(curve):
    """LASSO_GENS_DEVICE_BATCH=7: the same sets through many device calls; LASSO_GENS_DEVICE=0: the host route, the counter stays at 0; the default threshold keeps
    sets below it on the host"""
    wired, plain = G.build_mock_prover_gens(curve), build_mock_prover(curve)
    jobs = [{"shape": list(sh), "head": 0, "prove": None} for sh in SHAPES]
    host = G.gens_in_child(plain, curve, jobs, {})
    one = G.gens_in_child(wired, curve, jobs, {"LASSO_GENS_DEVICE_MIN": "1"})
    many = G.gens_in_child(wired, curve, jobs, {"LASSO_GENS_DEVICE_MIN": "1", "LASSO_GENS_DEVICE_BATCH": "7"})
    off = G.gens_in_child(wired, curve, jobs, {"LASSO_GENS_DEVICE_MIN": "1", "LASSO_GENS_DEVICE": "0"})
    high = G.gens_in_child(wired, curve, jobs, {"LASSO_GENS_DEVICE_MIN": "131"})      # one more than the widest set here
    dflt = G.gens_in_child(wired, curve, jobs, {})                                      # the default threshold is the headline's set: these sets stay on the host
    for k in range(len(jobs)):
        assert host[k]["sha256"] == one[k]["sha256"] == many[k]["sha256"] == off[k]["sha256"] == high[k]["sha256"], SHAPES[k]
        assert host[k]["count"] == one[k]["count"]
    assert [r["stats"]["device_candidates"] for r in host] == [0] * len(jobs) and host[0]["stats"]["available"] is False
    assert [r["stats"]["device_candidates"] for r in off] == [0] * len(jobs) and off[0]["stats"]["available"] is True
    assert [r["stats"]["device_candidates"] for r in high] == [0] * len(jobs) and max(host[-1]["count"]) == 130
    assert [r["stats"]["device_candidates"] for r in dflt] == [0] * len(jobs) and [r["sha256"] for r in dflt] == [r["sha256"] for r in host]
    c_one = [r["stats"]["device_candidates"] for r in one]; c_many = [r["stats"]["device_candidates"] for r in many]
    assert all(b > a for a, b in zip([0] + c_one, c_one)) and all(b > a for a, b in zip([0] + c_many, c_many))
    assert c_many[0] % 7 == 0 and c_many[0] >= 2 * max(one[0]["count"])      # whole batches of seven, and no fewer candidates than points need
    assert c_many[-1] <= c_one[-1]      # small batches stop as soon as the set is full: they never draw more than the one large batch
