"""Helpers of the subtable-MLE tests (tests/test_mle_cpu.py, tests/test_gpu_mle.py): the CPU build of the host prover against the mock with lasso_tables_mle added
(tests/cpp/mock_mle_wrap.cpp), Python big-integer references, and a child-process verifier for the settings that are read once per process."""
import json
import os
import subprocess
import sys

import numpy as np
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mock_prover_mle(curve="curve25519"):
    """the host prover over the mock with lasso_tables_mle (tests/cpp/mock_mle_wrap.cpp: the mock's literal eq table and dot products), so the verifier takes its
    device route, and with caller-defined strategies provable on the CPU"""
    return build_mock_prover(curve, ext=("custom", "mle"))


# ---- big-integer references (memory words are value * 2^256 mod p)

R = 1 << 256


def word_ints(rows):
    flat = np.asarray(rows, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in flat]


def int_words(vals):
    return np.array([[(int(v) >> (64 * k)) & (2**64 - 1) for k in range(4)] for v in vals], dtype=np.uint64).reshape(-1, 4)


def chi_int(point_words, p):
    """EqPolynomial(point).evals() on Python ints from the point's memory words (any representative)"""
    from customutil import eq_evals_int
    rinv = pow(R, -1, p)
    return eq_evals_int([w * rinv % p for w in word_ints(point_words)], p)


def mle_int(table, chi, p, field):
    """the memory word of sum_i T[i] chi_i: `table` = 1-D integers, or (n, 4) memory words of any representative"""
    if field:
        rinv = pow(R, -1, p)
        vals = [w * rinv % p for w in word_ints(table)]
    else:
        vals = [int(v) for v in np.asarray(table).reshape(-1)]
    return sum(v * c for v, c in zip(vals, chi) if v) % p * R % p


# ---- a verify in a FRESH process: LASSO_VERIFY_DEVICE_MLE and LASSO_MLE_DEVICE_MIN are read once per process
# argv: root, library ("" = the product library of `curve`), curve, strategy specs (JSON list of {"make": name, "args": [...]}), lookups.  Per spec:
# Proves the instance, then verifies the honest proof and every tampered variant (single-bit flips spread over eval_final, the hash-layer claims and a commitment row;
# truncated bytes) and the honest bytes against the strategy with one table entry changed, printing one JSON line: per variant the verdict (True / False / the error text) and the mle_stats delta of that verify; the bytes go back in hex.
CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import _abi
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver
import mleutil
lib, curve, specs, lookups, few = sys.argv[2], sys.argv[3], json.loads(sys.argv[4]), int(sys.argv[5]), sys.argv[6] == "few"
hp = HostProver(C.CDLL(lib) if lib else None, curve=curve)
assert hp.mle_stats()["device_tables"] == 0
out = []
for spec in specs:
    cs = mleutil.make_strategy(spec, curve, hp)
    c, log_m = cs.c, cs.log_m
    s = 1 << max((lookups - 1).bit_length(), 0)
    idx = mleutil.child_indices(cs, lookups)
    r = hp.gen_random_point(max(s.bit_length() - 1, 0))
    gens = hp.gens(c, s, cs.num_memories, log_m)
    dense = hp.densify(idx, log_m)
    comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, cs, r)
    results = []
    def run(name, p, cm, strategy=None):
        before = hp.mle_stats()["device_tables"]
        try:
            v = hp.verify(gens, strategy or cs, s, r, p, cm)
        except LassoError as e:
            v = str(e)
        results.append({"name": name, "verdict": v, "device_tables": hp.mle_stats()["device_tables"] - before})
    run("honest", proof, comm)
    for name, p, cm in mleutil.tampered(proof, comm, cs, few):
        run(name, p, cm)
    other = mleutil.make_strategy(spec, curve, hp)          # the STATEMENT changed: one entry of the first table the memories use — only the subtable MLE can tell
    k0 = cs.memory_map(0)[0]
    if other.field: other.tables[k0][3][0] ^= np.uint64(1)
    else: other.tables[k0][3] ^= np.uint32(1)
    run("one table entry changed", proof, comm, other)
    out.append({"results": results, "distinct": len({cs.memory_map(i)[0] for i in range(cs.num_memories)}), "available": hp.mle_stats()["available"],
                "proof": proof.hex(), "comm": comm.hex(), "r": np.asarray(r).tolist()})
    hp.free(dense, gens)
print(json.dumps(out))
hp.close()
"""


def child_indices(cs, lookups):
    """the lookups CHILD proves for strategy `cs`"""
    return np.ascontiguousarray(np.random.default_rng(11 + lookups).integers(0, 1 << cs.log_m, size=(lookups, cs.c), dtype=np.uint64))


# what tests/test_gpu_mle.py runs, here so that tests/test_mle_cpu.py can hold it against the launch plan without importing a GPU module
LOG_MS = [1, 2, 3, 4, 5, 8, 9, 12, 13, 14, 15, 16, 17, 20]
FOLD_LOG_MS = [12, 16]          # shapes at which every lane walks at least two fold periods
STRIP_TEST_LEN = 300            # LASSO_MLE_STRIP for a 2^10-entry table: three whole strips and one of 124 entries, none but the first on a row boundary


def make_strategy(spec, curve, host=None):
    """{"make": "lte" | "field" | "builtin", "args": [...]} -> the CustomStrategy (the child and the parent build the same object from the same spec)"""
    import customutil as U
    if spec["make"] == "lte":
        return U.lte_strategy(*spec["args"], curve=curve)
    if spec["make"] == "field":
        return U.field_square_strategy(*spec["args"], curve=curve)
    kind, c, log_m, log_r = spec["args"]
    return U.builtin_as_custom(kind, c, log_m, log_r, curve, host=host)


def proof_layout(proof, cs):
    """byte offsets inside a proof (lasso_amd/host/verifier.hpp read_proof): the first of the four arrays eval_dim, eval_read, eval_final (C scalars each) and
    eval_derefs_hash (num_memories scalars), found from the END: behind them only the three openings remain, each two point vectors, two points and two scalars"""
    def dpl_len_backwards(end):
        # [u64 k][k pts][u64 k][k pts][pt][pt][sc][sc] with both vectors of one length k: end - 128 - 2 * (8 + 32 k); k is read from the front of the block, so try sizes
        for k in range(0, 64):
            start = end - 128 - 2 * (8 + 32 * k)
            if start >= 0 and int.from_bytes(proof[start:start + 8], "little") == k and int.from_bytes(proof[start + 8 + 32 * k:start + 16 + 32 * k], "little") == k:
                return start
        raise AssertionError("proof layout: no opening found")
    pos = len(proof)
    for _ in range(3):
        pos = dpl_len_backwards(pos)
    alpha, c = cs.num_memories, cs.c
    hash0 = pos - 32 * alpha
    final0 = hash0 - 32 * c
    return {"eval_final": final0, "eval_derefs_hash": hash0, "eval_read": final0 - 32 * c, "eval_dim": final0 - 64 * c, "tail": pos}


def tampered(proof, comm, cs, few=False):
    """[(name, proof bytes, commitment bytes)]: single-bit flips spread over eval_final, over the hash-layer claims (eval_dim / eval_read / eval_derefs_hash) and over one
    commitment row, and the proof cut short at three places; few: every fourth of them (the GPU tests, where a verify costs 60 - 100 ms)"""
    lay = proof_layout(proof, cs)
    out = []

    def flip(buf, pos, bit):
        b = bytearray(buf); b[pos] ^= 1 << bit; return bytes(b)
    c, alpha = cs.c, cs.num_memories
    for j in sorted({0, c - 1}):
        for byte, bit in ((0, 0), (13, 5), (31, 2)):
            out.append((f"eval_final[{j}] byte {byte} bit {bit}", flip(proof, lay["eval_final"] + 32 * j + byte, bit), comm))
    for name, n in (("eval_dim", c), ("eval_read", c), ("eval_derefs_hash", alpha)):
        for j in sorted({0, n - 1}):
            out.append((f"{name}[{j}] byte 7 bit 3", flip(proof, lay[name] + 32 * j + 7, 3), comm))
    rows = int.from_bytes(comm[:8], "little")
    for byte, bit in ((2, 4), (17, 0)):
        out.append((f"commitment row {rows // 2} byte {byte} bit {bit}", proof, flip(comm, 8 + 32 * (rows // 2) + byte, bit)))
    for cut in (lay["eval_final"] + 5, lay["tail"], len(proof) - 1):
        out.append((f"proof cut at {cut}", proof[:cut], comm))
    return out[::4] if few else out


def verify_in_child(lib, curve, specs, lookups, env_extra, timeout=300, few=False):
    """run CHILD over the list `specs` with env_extra added to the environment; returns the decoded JSON line: one entry per spec"""
    env = dict(os.environ)
    for k in ("LASSO_VERIFY_DEVICE_MLE", "LASSO_MLE_DEVICE_MIN", "LASSO_MLE_STRIP"):
        env.pop(k, None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib or "", curve, json.dumps(specs), str(lookups), "few" if few else "all"], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])
