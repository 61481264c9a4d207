"""Helpers of the tests of label-derived generators on the device (tests/test_gens_device_cpu.py, tests/test_gpu_gens_device.py): the candidate stream of a label
written from rand_chacha / ark-ff's rules in Python (SHAKE256 seed, ChaCha20 words, Fq::rand's masking and rejection, the bool) — NOT from the product's C++ —, a
big-integer statement of "candidate to point" written from ark-ec's get_point_from_y_unchecked / get_point_from_x_unchecked followed by the cofactor, crafted
candidates for both curves, and the CPU build of the host prover against the mock with lasso_points_from_candidates added (tests/cpp/mock_gens_wrap.cpp)."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

import wireutil as W
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OK, NONCANONICAL, NO_POINT = range(3)
LABEL = b"gens_sparse_poly"
MODULUS = {"curve25519": W.P25, "bn254": W.Q254}
MASK_BITS = {"curve25519": 255, "bn254": 254}       # Fq::rand keeps the modulus' bit length of the drawn limbs


# ---------------------------------------------------------------- the stream

def _chacha20_words(key32, nblocks):
    """the first 16 * nblocks output words of ChaCha20 (64-bit block counter from 0, stream 0), all blocks at once"""
    k = np.frombuffer(key32, dtype="<u4").astype(np.uint32)
    ctr = np.arange(nblocks, dtype=np.uint64)
    st = np.zeros((16, nblocks), dtype=np.uint32)
    st[0], st[1], st[2], st[3] = 0x61707865, 0x3320646E, 0x79622D32, 0x6B206574
    for i in range(8):
        st[4 + i] = k[i]
    st[12] = (ctr & np.uint64(0xFFFFFFFF)).astype(np.uint32); st[13] = (ctr >> np.uint64(32)).astype(np.uint32)
    x = st.copy()

    def rl(v, c):
        return (v << np.uint32(c)) | (v >> np.uint32(32 - c))

    def qr(a, b, c, d):
        x[a] += x[b]; x[d] = rl(x[d] ^ x[a], 16); x[c] += x[d]; x[b] = rl(x[b] ^ x[c], 12)
        x[a] += x[b]; x[d] = rl(x[d] ^ x[a], 8); x[c] += x[d]; x[b] = rl(x[b] ^ x[c], 7)

    with np.errstate(over="ignore"):
        for _ in range(10):
            qr(0, 4, 8, 12); qr(1, 5, 9, 13); qr(2, 6, 10, 14); qr(3, 7, 11, 15)
            qr(0, 5, 10, 15); qr(1, 6, 11, 12); qr(2, 7, 8, 13); qr(3, 4, 9, 14)
        x += st
    return x.T.reshape(-1)


def generator_encoding(curve):
    """serialize_compressed of the group's generator: what MultiCommitGens::new absorbs after the label (commitments.rs:24-27)"""
    return W.enc254((1, 2)) if curve == "bn254" else W.enc25(W.BASE25)


_STREAMS = {}


def stream_candidates(curve, n, label=LABEL):
    """the first n candidates `Projective::rand` draws on the ChaCha20 stream of `label`: (limbs (n, 4) uint64 — taken as the Montgomery representation, masked, rejected
    when not below the modulus —, greatest (n,) uint8 — the top bit of the next 32-bit word).  Computed once per (curve, label) and extended on demand."""
    key = (curve, label)
    have = _STREAMS.get(key)
    if have is None or have[0].shape[0] < n:
        seed = hashlib.shake_256(label + generator_encoding(curve)).digest(32)
        want = max(n, 2048)
        words = _chacha20_words(seed, (want * 13) // 16 + 64)      # 9 words per accepted candidate; BN254 rejects about one masked draw in four (8 words each): 11.6 on average
        p, mask = MODULUS[curve], (1 << MASK_BITS[curve]) - 1
        limbs, greatest, pos = [], [], 0
        by = words.astype("<u4").tobytes()
        while len(limbs) < want:
            v = int.from_bytes(by[4 * pos: 4 * pos + 32], "little") & mask; pos += 8
            if v >= p:
                continue
            greatest.append(int(words[pos]) >> 31); pos += 1
            limbs.append([(v >> (64 * k)) & (2**64 - 1) for k in range(4)])
        assert pos <= words.shape[0]
        have = (np.array(limbs, dtype=np.uint64), np.array(greatest, dtype=np.uint8))
        _STREAMS[key] = have
    return have[0][:n].copy(), have[1][:n].copy()


# ---------------------------------------------------------------- candidate -> point, in big integers

def limbs_int(row):
    return sum(int(w) << (64 * k) for k, w in enumerate(row))


def int_limbs(v):
    return [(v >> (64 * k)) & (2**64 - 1) for k in range(4)]


def from_candidate(curve, v, greatest):
    """(status, affine 64 bytes): v = the 256-bit integer the limbs spell (the Montgomery representation of the coordinate), greatest = the root choice"""
    p = MODULUS[curve]
    if v >= p:
        return NONCANONICAL, bytes(64)
    c = v * pow(2**256, -1, p) % p
    if curve == "bn254":
        # ark-ec short_weierstrass get_point_from_x_unchecked: y^2 = x^3 + b, the (smaller, larger) root; cofactor 1
        rhs = (c * c * c + 3) % p
        y = pow(rhs, (p + 1) // 4, p)
        if y * y % p != rhs:
            return NO_POINT, bytes(64)
        y = max(y, (p - y) % p) if greatest else min(y, (p - y) % p)
        return OK, W.mont_words(c, p) + W.mont_words(y, p)
    # ark-ec twisted_edwards get_point_from_y_unchecked: x^2 = (1 - y^2) / (a - d y^2), a = -1, the (smaller, larger) root; then mul_by_cofactor (x 8)
    den = (-1 - W.D25 * c * c) % p
    if den == 0:
        return NO_POINT, bytes(64)
    x = W.sqrt25((1 - c * c) * pow(den, -1, p))
    if x is None:
        return NO_POINT, bytes(64)
    x = max(x, (p - x) % p) if greatest else min(x, (p - x) % p)
    assert W.ed_on_curve(x, c)
    X, Y = W.ed_mul(8, (x, c))
    return OK, W.mont_words(X, p) + W.mont_words(Y, p)


def crafted(curve):
    """(label, integer the limbs spell, greatest, expected status) — the cases every implementation must agree on"""
    p = MODULUS[curve]
    R = 2**256 % p
    out = []
    for name, v in (("zero", 0), ("one", 1), ("p-1", p - 1), ("p", p), ("2^255-1", 2**255 - 1), ("2^256-1", 2**256 - 1), ("p+1", p + 1)):
        for g in (0, 1):
            out.append((f"{name}-g{g}", v, g, NONCANONICAL if v >= p else None))
    if curve == "curve25519":
        for name, y in (("y=1", 1), ("y=-1", p - 1), ("y=0", 0)):      # small-order points: times 8 the identity, which leaves as (0, 1)
            for g in (0, 1):
                out.append((f"{name}-g{g}", y * R % p, g, OK))
    c, found = 1, 0
    while found < 2:                                   # coordinates without a point
        c += 1
        if from_candidate(curve, c * R % p, 0)[0] == NO_POINT:
            out.append((f"nonresidue-{c}-g{found}", c * R % p, found, NO_POINT)); found += 1
    c, found = 1, 0
    while found < 2:                                   # both roots over one coordinate
        c += 1
        if from_candidate(curve, c * R % p, 0)[0] == OK:
            out.append((f"coordinate-{c}-smaller", c * R % p, 0, OK)); out.append((f"coordinate-{c}-larger", c * R % p, 1, OK)); found += 1
    return [(n, v, g, st if st is not None else from_candidate(curve, v, g)[0]) for n, v, g, st in out]


def crafted_arrays(curve):
    cases = crafted(curve)
    return np.array([int_limbs(v) for _, v, _, _ in cases], dtype=np.uint64), np.array([g for _, _, g, _ in cases], dtype=np.uint8)


def batch(curve, n, seed):
    """n candidates: the stream's first n with every crafted candidate (as far as n allows) scattered in"""
    limbs, greatest = stream_candidates(curve, n)
    cl, cg = crafted_arrays(curve)
    at = np.random.default_rng(seed).permutation(n)[: cl.shape[0]]
    limbs[at] = cl[: at.shape[0]]; greatest[at] = cg[: at.shape[0]]
    return limbs, greatest


def reference(curve, limbs, greatest):
    """from_candidate over arrays: (affine (n, 8) uint64, status (n,) uint8)"""
    res = [from_candidate(curve, limbs_int(row), int(g)) for row, g in zip(limbs, greatest)]
    aff = np.frombuffer(b"".join(a for _, a in res), dtype="<u8").reshape(-1, 8) if res else np.zeros((0, 8), dtype=np.uint64)
    return aff.astype(np.uint64), np.array([s for s, _ in res], dtype=np.uint8)


_ORACLES = {}


def load_oracle(curve):
    """the CPU oracle of `curve` (oracle/Makefile decides staleness), whatever curve the session's `oracle` fixture was asked for"""
    import ctypes
    if curve not in _ORACLES:
        name = "liblasso_oracle_bn254.so" if curve == "bn254" else "liblasso_oracle.so"
        subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), name])
        lib = ctypes.CDLL(os.path.join(ROOT, "oracle", name))      # RTLD_LOCAL: the two builds export the same names
        assert lib.orc_curve_id() == (1 if curve == "bn254" else 0)
        _ORACLES[curve] = lib
    return _ORACLES[curve]


def oracle_gens(oracle, count, label=LABEL):
    """the first `count` points of the label's stream by the oracle's own point_rand (orc_gens: canonical coordinates), converted to Montgomery limbs: (count, 8) uint64"""
    import ctypes
    p = MODULUS["bn254" if oracle.orc_curve_id() == 1 else "curve25519"]
    out = (ctypes.c_uint64 * (8 * count))()
    assert oracle.orc_gens(label, ctypes.c_size_t(count - 1), out) == 0
    flat = [limbs_int(out[4 * i: 4 * i + 4]) for i in range(2 * count)]
    return np.array([int_limbs((v << 256) % p) for v in flat], dtype=np.uint64).reshape(count, 8)


# ---------------------------------------------------------------- builds and child processes

def build_mock_prover_gens(curve="curve25519"):
    """the host prover over the mock with lasso_points_from_candidates (tests/cpp/mock_gens_wrap.cpp: the product's pt_from_candidate on the host), so
    lasso_host_gens_new takes the device route on the CPU"""
    return build_mock_prover(curve, ext=("gens",))


# Generator sets (and optionally one proof) in a FRESH process: the LASSO_GENS_* switches are read once per process.  argv: repository root, library ("" = the product
# library of `curve`), curve, then a JSON list of jobs {"shape": [c, s, memories, log_m], "head": points of every set to return in full (0 = none),
# "prove": [kind, c, log_m, log_r, lookups] or null}.  Prints one JSON line: per job the sha256 and point count of each of the three sets, the head points (hex), the
# commitment and proof (hex) if asked for, and the gens_stats after the job.
CHILD = r"""
import ctypes as C, hashlib, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import _abi
from lasso_amd.prover import HostProver
lib, curve, jobs = sys.argv[2], sys.argv[3], json.loads(sys.argv[4])
hp = HostProver(C.CDLL(lib) if lib else None, curve=curve)
out = []
for job in jobs:
    c, s, mem, log_m = job["shape"]
    gens = hp.gens(c, s, mem, log_m)
    sets = [hp.gens_points(gens, w) for w in range(3)]
    res = {"sha256": [hashlib.sha256(a.tobytes()).hexdigest() for a in sets], "count": [int(a.shape[0]) for a in sets],
           "head": [a[: job["head"]].tobytes().hex() for a in sets] if job.get("head") else None}
    if job.get("prove"):
        kind, pc, plog_m, log_r, lookups = job["prove"]
        idx = np.random.default_rng(7 + lookups).integers(0, 1 << plog_m, size=(lookups, pc), dtype=np.uint64)
        r = hp.gen_random_point(max(s.bit_length() - 1, 0))
        S = _abi.Strategy(_abi.KINDS[kind], pc, plog_m, log_r)
        dense = hp.densify(idx, plog_m)
        res["comm"] = hp.commit(dense, gens).hex(); res["proof"] = hp.prove(dense, gens, S, r).hex()
        hp.free(dense)
    res["stats"] = hp.gens_stats()
    out.append(res)
    hp.free(None, gens)
hp.close()
print("GENS_RESULT " + json.dumps(out))
"""


def gens_in_child(lib, curve, jobs, env_extra, timeout=600):
    env = dict(os.environ)
    for k in ("LASSO_GENS_DEVICE", "LASSO_GENS_DEVICE_MIN", "LASSO_GENS_DEVICE_BATCH"):
        env.pop(k, None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib or "", curve, json.dumps(jobs)], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    line = [ln for ln in res.stdout.split("\n") if ln.startswith("GENS_RESULT ")][-1]
    return json.loads(line[len("GENS_RESULT "):])
