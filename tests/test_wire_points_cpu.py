"""CPU: the reading half of the wire format — ark-serialize compressed points decoded and validated (include/lasso_hip_wire.h, lasso_host_points_decompress).
  * pt_decompress (lasso_amd/csrc/fe29.cuh, bn254_fe29.cuh: what one lane of k_points_decompress runs), compiled for the host, against a big-integer decoder written from
    ark-ec's rules (tests/wireutil.py) and against the verifier's own host decoder (lasso_host_points_decompress, where = 0): status, affine limbs and canonical bytes;
  * the verifier's batched path (one lasso_points_decompress call per proof) through a mock that has the decoder (tests/cpp/mock_wire_wrap.cpp) against the plain mock's
    sequential path: the same verdict, return code and error text on honest, tampered, truncated and extended bytes, and on the committed artefacts;
  * the symbols: both device libraries export lasso_points_decompress, include/lasso_hip.h does not declare it, and a device library without it is reported as such."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import wireutil as W
from lasso_amd import _abi
from lasso_amd.device import LassoError
from proverutil import HostProver, build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]
# every built-in strategy; (kind, C, log_m, log_r, lookups)
CASES = [("lt", 4, 4, 0, 16), ("and", 4, 4, 0, 16), ("range", 3, 8, 12, 16), ("xor", 3, 4, 0, 11), ("or", 2, 6, 0, 40), ("spark", 2, 4, 0, 32), ("and", 1, 16, 0, 1 << 10)]


# ---------------------------------------------------------------- symbols and headers

def _header_functions(name):
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", name)).read(), flags=re.S)
    return sorted(set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", src)))


def test_wire_header_is_separate_from_the_device_header():
    assert _header_functions("lasso_hip_wire.h") == ["lasso_points_decompress"]
    assert "lasso_points_decompress" not in _header_functions("lasso_hip.h")
    assert {"lasso_host_points_decompress", "lasso_host_wire_stats"} <= set(_header_functions("lasso_prover.h"))


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_decoder(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_wire(dev) == _header_functions("lasso_hip_wire.h")      # AttributeError = not exported
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for name in ("lasso_host_points_decompress", "lasso_host_wire_stats"):
        getattr(host, name)


def test_the_mock_of_the_device_header_has_no_decoder():
    from gpuutil import load_mock
    with pytest.raises(AttributeError):
        _abi.declare_wire(load_mock())


# ---------------------------------------------------------------- the arithmetic

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
    """per curve: the plain mock build (no device decoder), the wrapped build (decoder present, threshold 1 so that the smallest proofs take the batched path too), and
    proofs of every built-in strategy made once with the plain build"""
    curve = request.param
    old = os.environ.get("LASSO_WIRE_DEVICE_MIN")
    os.environ["LASSO_WIRE_DEVICE_MIN"] = "1"       # read once per library, at its first verify
    plain = HostProver(C.CDLL(build_mock_prover(curve)))
    wired = HostProver(C.CDLL(W.build_mock_prover_wire(curve)))
    cases = []
    for case in CASES:
        pc = _proof_case(plain, *case)
        pc["gens_wired"] = wired.gens(case[1], pc["s"], pc["alpha"], case[2])
        cases.append(pc)
    yield curve, plain, wired, cases
    for pc in cases:
        plain.free(None, pc["gens"]); wired.free(None, pc["gens_wired"])
    plain.close(); wired.close()
    if old is None:
        os.environ.pop("LASSO_WIRE_DEVICE_MIN", None)
    else:
        os.environ["LASSO_WIRE_DEVICE_MIN"] = old


def _encodings(curve, cases):
    enc = [(n, b) for n, b, _ in W.crafted(curve)]
    for k, pc in enumerate(cases):       # row commitments of real proofs: the commitment's rows and comm_derefs (the proof's first vector)
        rows = [pc["comm"][o:o + 32] for o in W.commitment_points(pc["comm"])]
        pts, _ = W.walk_proof(pc["proof"], pc["alpha"], pc["c"])
        rows += [pc["proof"][o:o + 32] for o in pts]
        if len(rows) > 48:
            rows = rows[:: len(rows) // 48 + 1]
        enc += [(f"case{k}-row{i}", b) for i, b in enumerate(rows)]
    return enc


def _run_host_program(curve, flags, enc, tag):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_wire_host_{curve}_{tag}")
    cflags = ["-DLASSO_BN254"] if curve == "bn254" else []
    subprocess.check_call(["g++", "-std=c++17", "-Wno-unknown-pragmas", *cflags, *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_wire_host.cpp")])
    path = os.path.join(out_dir, f"wire_encodings_{curve}_{tag}.hex")
    with open(path, "w") as f:
        f.write("".join(b.hex() + "\n" for _, b in enc))
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    lines = res.stdout.strip().split("\n")
    assert lines[-1] == f"OK {len(enc)}"
    return [(int(s), bytes.fromhex(a), bytes.fromhex(c)) for s, a, c in (ln.split() for ln in lines[:-1])]


@pytest.mark.parametrize("flags,tag", [(["-O2"], "limbs64"), (["-O2", "-DLASSO_HOST_LIMBS32"], "limbs32"), (["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"], "ubsan")])
def test_decoder_arithmetic_against_big_integers(libs, flags, tag):
    """status, affine limbs and canonical bytes of pt_decompress == the big-integer decoder's, on every crafted encoding and on rows of real proofs; under UBSan no limb or
    column leaves its container on the way (the power chain, the subgroup ladder)"""
    curve, plain, wired, cases = libs
    enc = _encodings(curve, cases)
    got = _run_host_program(curve, flags, enc, tag)
    for (name, b), g in zip(enc, got):
        assert g == W.decode(curve, b), name
    for name, b, st in W.crafted(curve):
        assert W.decode(curve, b)[0] == st, name      # the reference itself gives the status the case was crafted for


def test_host_entry_point_equals_reference_and_wrapped_device_path(libs):
    """lasso_host_points_decompress: where = 0 (today's verifier decoder) == the big-integer decoder == where = 1 through the wrapped mock (the product's pt_decompress);
    NULL outputs are allowed; the counter counts where = 1 only"""
    curve, plain, wired, cases = libs
    enc = _encodings(curve, cases)
    blob = b"".join(b for _, b in enc)
    want = [W.decode(curve, b) for _, b in enc]
    a0, c0, s0 = plain.points_decompress(blob, where=0)
    for i, (name, _) in enumerate(enc):
        assert (int(s0[i]), a0[i].tobytes(), c0[i].tobytes()) == want[i], name
    before = wired.wire_stats()["device_points"]
    a1, c1, s1 = wired.points_decompress(blob, where=1)
    assert np.array_equal(a0, a1) and np.array_equal(c0, c1) and np.array_equal(s0, s1)
    assert wired.wire_stats() == {"device_points": before + len(enc), "device_available": True}
    st = np.zeros(len(enc), dtype=np.uint8)
    wired._chk(wired.lib.lasso_host_points_decompress(wired.h, blob, len(enc), 1, None, None, st.ctypes.data_as(C.c_void_p)))
    assert np.array_equal(st, s0)
    assert wired.points_decompress(b"", where=1)[2].shape == (0,)


def test_plain_mock_reports_the_decoder_missing_and_still_verifies(libs):
    curve, plain, wired, cases = libs
    assert plain.wire_stats() == {"device_points": 0, "device_available": False}
    with pytest.raises(LassoError, match="not available"):
        plain.points_decompress(cases[0]["comm"][8:40], where=1)
    pc = cases[0]
    assert plain.verify(pc["gens"], pc["S"], pc["s"], pc["r"], pc["proof"], pc["comm"]) is True
    assert plain.wire_stats()["device_points"] == 0


# ---------------------------------------------------------------- the verifier: batched path == sequential path

def _outcome(hp, gens, pc, proof, comm):
    """True / False, or the error exactly as the C ABI reports it (return code and lasso_host_last_error text)"""
    try:
        return hp.verify(gens, pc["S"], pc["s"], pc["r"], proof, comm)
    except LassoError as e:
        return str(e)


def _same(plain, wired, pc, proof, comm, what):
    a, b = _outcome(plain, pc["gens"], pc, proof, comm), _outcome(wired, pc["gens_wired"], pc, proof, comm)
    assert a == b, f"{what}: sequential {a!r}, batched {b!r}"
    return a


@pytest.mark.parametrize("k", range(len(CASES)), ids=[f"{c[0]}-c{c[1]}-m{c[2]}-s{c[4]}" for c in CASES])
def test_batched_verifier_equals_sequential_verifier(libs, k):
    curve, plain, wired, cases = libs
    pc = cases[k]
    proof, comm = pc["proof"], pc["comm"]
    pts, scs = W.walk_proof(proof, pc["alpha"], pc["c"])
    cpts = W.commitment_points(comm)
    before = wired.wire_stats()["device_points"]
    assert _same(plain, wired, pc, proof, comm, "honest") is True
    assert wired.wire_stats()["device_points"] == before + len(pts) + len(cpts) > before      # every point of proof and commitment went through the one device call
    seen = set()
    # one flipped bit in every point of the proof (a stride when there are many), the flag bits and coordinate bits alike; then some scalars; then commitment rows
    stride = len(pts) // 40 + 1
    for j, o in enumerate(pts[::stride]):
        bit = (37 * j + 251) % 256 if j % 3 else 255 - (j // 3) % 2      # every third flip hits a flag bit
        bad = bytearray(proof); bad[o + bit // 8] ^= 1 << (bit % 8)
        seen.add(str(_same(plain, wired, pc, bytes(bad), comm, f"point at {o} bit {bit}")))
    for j, o in enumerate(scs[:: len(scs) // 10 + 1]):
        bit = (61 * j + 3) % 256 if j % 2 else 255
        bad = bytearray(proof); bad[o + bit // 8] ^= 1 << (bit % 8)
        seen.add(str(_same(plain, wired, pc, bytes(bad), comm, f"scalar at {o} bit {bit}")))
    for j, o in enumerate(cpts[:: len(cpts) // 8 + 1]):
        bit = (29 * j + 7) % 256
        badc = bytearray(comm); badc[o + bit // 8] ^= 1 << (bit % 8)
        seen.add(str(_same(plain, wired, pc, proof, bytes(badc), f"commitment row at {o} bit {bit}")))
    assert any("invalid point encoding" in s for s in seen) or curve == "bn254", seen      # the flips did reach the decoder's rejections
    # a length prefix in front of points
    bad = bytearray(proof); bad[0] ^= 1
    _same(plain, wired, pc, bytes(bad), comm, "length prefix")
    # two commitment rows swapped
    if len(cpts) >= 2:
        a, b = cpts[0], cpts[1]
        badc = bytearray(comm); badc[a:a + 32], badc[b:b + 32] = comm[b:b + 32], comm[a:a + 32]
        if bytes(badc) != comm:
            assert _same(plain, wired, pc, proof, bytes(badc), "swapped rows") is not True
    # truncation at several offsets (inside a point, inside a scalar, inside a prefix, at the end), trailing bytes, both for proof and commitment
    for cut in sorted({1, 7, 8, 9, 39, 40, pts[-1] + 5, scs[len(scs) // 2] + 11, len(proof) - 33, len(proof) - 1}):
        if 0 < cut < len(proof):
            assert isinstance(_same(plain, wired, pc, proof[:cut], comm, f"proof cut at {cut}"), str)
    assert isinstance(_same(plain, wired, pc, proof + b"\0", comm, "proof + 1 byte"), str)
    assert isinstance(_same(plain, wired, pc, proof + bytes(32), comm, "proof + 32 bytes"), str)
    for cut in (7, 8 + 31, len(comm) - 1):
        assert isinstance(_same(plain, wired, pc, proof, comm[:cut], f"commitment cut at {cut}"), str)
    assert isinstance(_same(plain, wired, pc, proof, comm + b"\0", "commitment + 1 byte"), str)
    # an error in the proof precedes an error in the commitment, whichever path found them
    bad = bytearray(proof); bad[pts[0]] ^= 1
    _same(plain, wired, pc, bytes(bad) + b"\0", comm[:-1], "both broken")
    assert _same(plain, wired, pc, proof, comm, "honest again") is True


@pytest.mark.parametrize("name,curve", [("artefact_and_c1_2p10", "curve25519"), ("artefact_bn254_and_c4_2p8", "bn254"), ("artefact_and_c1_2p24", "curve25519")])
def test_committed_artefacts_verify_through_the_batched_path(name, curve, monkeypatch):
    monkeypatch.setenv("LASSO_WIRE_DEVICE_MIN", "1")      # the small artefacts have fewer points than the default threshold (read once per library, at its first verify)
    d = os.path.join(ROOT, "tests", "golden", name)
    meta = json.load(open(os.path.join(d, "meta.json")))
    files = {k: open(os.path.join(d, k), "rb").read() for k in ("proof.bin", "commitment.bin", "point.bin")}
    for k, v in files.items():
        assert hashlib.sha256(v).hexdigest() == meta["sha256"][k]
    p = {"curve25519": 2**252 + 27742317777372353535851937790883648493, "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617}[curve]
    pt = files["point.bin"]
    r = np.array([[(int.from_bytes(pt[i:i + 32], "little") << 256) % p >> (64 * k) & (2**64 - 1) for k in range(4)] for i in range(0, len(pt), 32)], dtype=np.uint64).reshape(-1, 4)
    comm = files["commitment.bin"][:-24]
    S = _abi.Strategy(_abi.KINDS[meta["strategy"]], meta["C"], meta["log_m"], meta["log_r"])
    hp = HostProver(C.CDLL(W.build_mock_prover_wire(curve)))
    try:
        gens = hp.gens(meta["C"], meta["s"], meta["num_memories"], meta["log_m"], label=meta["gens_label"].encode())
        assert hp.verify(gens, S, meta["s"], r, files["proof.bin"], comm, transcript=meta["transcript_label"].encode()) is True
        n_points = len(W.walk_proof(files["proof.bin"], meta["num_memories"], meta["C"])[0]) + len(W.commitment_points(comm))
        assert hp.wire_stats()["device_points"] == n_points > 0
        hp.free(None, gens)
    finally:
        hp.close()
