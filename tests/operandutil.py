"""Helpers of the tests of densify from operand columns (tests/test_operands_cpu.py, tests/test_gpu_operands.py): the Python big-integer statement of the layout
(include/lasso_hip_operands.h), the CPU builds of the host prover against the mock with lasso_densify_dim_operands added (tests/cpp/mock_operands_wrap.cpp), the slab
harness densifying from operands (tests/cpp/slab_threads_operands.cpp), and a child process for LASSO_DENSIFY_OPERANDS, which is read once per process."""
import json
import os
import subprocess
import sys

import numpy as np
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the layout on Python integers: the statement every implementation is held to

def py_chunk(v, j, b):
    return 0 if j * b >= 64 else (v >> (j * b)) & ((1 << b) - 1)


def py_index(layout, x, y, c, dim):
    operands, b, msb = layout
    j = c - 1 - dim if msb else dim
    return (py_chunk(x, j, b) << b) | py_chunk(y, j, b) if operands == 2 else py_chunk(x, j, b)


def py_fits(v, c, b):
    return c * b >= 64 or v < (1 << (c * b))


def py_indices(layout, x, y, c):
    y = [0] * len(x) if y is None else y
    return np.array([[py_index(layout, int(a), int(bb), c, d) for d in range(c)] for a, bb in zip(x, y)], dtype=np.uint64).reshape(len(x), c)


def builtin_layout(kind, log_m):
    """and.rs / or.rs / xor.rs, lt.rs:60-69, range_check.rs:78-86 as (operands, chunk_bits, msb_first)"""
    return {"and": (2, log_m // 2, 0), "or": (2, log_m // 2, 0), "xor": (2, log_m // 2, 0), "lt": (2, log_m // 2, 1), "range": (1, log_m, 0)}[kind]


def operands_for(layout, c, n, rng, mode="rand"):
    """n operand pairs that fit c chunks of the layout (y None for one operand); mode: rand, same (one hot address), sorted"""
    operands, b, _ = layout
    bits = min(64, c * b)
    def col():
        v = rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)   # all 64 bits
        v = v if bits == 64 else v & np.uint64((1 << bits) - 1)
        if mode == "same":
            v[:] = v[0]
        if mode == "sorted":
            v = np.sort(v)
        return np.ascontiguousarray(v)
    return col(), (col() if operands == 2 else None)


# ---- builds

def build_mock_prover_operands(curve="curve25519"):
    """the host prover over the mock WITH lasso_densify_dim_operands (and the custom-strategy wrappers): lasso_host_densify_operands takes its device path"""
    return build_mock_prover(curve, ext=("operands",))


def build_slab_lib_operands(curve="curve25519", with_entry=True):
    """tests/cpp/slab_threads_operands.cpp over the mock with the entry (with_entry) or the plain one (the fallback)"""
    return build_mock_prover(curve, ext=("operands",) if with_entry else (), harness=["slab_threads_operands.cpp"], extra_flags=["-pthread"])


# ---- LASSO_DENSIFY_OPERANDS in a fresh process.  argv: repository root, library ("" = the product library of `curve`), curve, JSON list of cases
# [kind, c, log_m, log_r, lookups, seed].  OPERANDS_CHILD_CAPACITY=1 in the environment: capacity mode on.  Prints one JSON line: per case the sha256 of commitment + proof
# after densify_operands and after densify(operand_indices(...)), the verdict, the stats and whether the representation is in capacity mode's compact form.
CHILD = r"""
import ctypes as C, hashlib, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import _abi
from lasso_amd.prover import HostProver
import operandutil as U
lib, curve, cases = sys.argv[2], sys.argv[3], json.loads(sys.argv[4])
hp = HostProver(C.CDLL(lib) if lib else None, curve=curve)
if os.environ.get("OPERANDS_CHILD_CAPACITY") == "1":
    hp.set_capacity(True)
out = []
for kind, c, log_m, log_r, lookups, seed in cases:
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    lay = hp.operand_layout(S)
    x, y = U.operands_for((lay.operands, lay.chunk_bits, lay.msb_first), c, lookups, np.random.default_rng(seed))
    if kind == "range":
        x = x & np.uint64((1 << log_r) - 1)
    s = 1 << max((lookups - 1).bit_length(), 0)
    r = hp.gen_random_point(max(s.bit_length() - 1, 0))
    gens = hp.gens(c, s, 2 * c if kind == "lt" else c, log_m)
    hp.densify_stats(reset=True)
    dense = hp.densify_operands(x, y, layout=lay, c=c, log_m=log_m)
    st = hp.densify_stats()
    compact = hp.dense_info(dense)["compact"]
    comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, S, r)
    hp.free(dense)
    dense = hp.densify(hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m), log_m)
    compact_index = hp.dense_info(dense)["compact"]
    comm_i = hp.commit(dense, gens); proof_i = hp.prove(dense, gens, S, r)
    out.append({"digest": hashlib.sha256(comm + proof).hexdigest(), "digest_index": hashlib.sha256(comm_i + proof_i).hexdigest(), "verify": hp.verify(gens, S, s, r, proof, comm), "stats": st,
                "compact": [compact, compact_index]})
    hp.free(dense, gens)
print(json.dumps(out))
hp.close()
"""


def case_operands(hp, kind, c, log_m, log_r, lookups, seed):
    """the operands CHILD proves for a case, and the built-in layout"""
    from lasso_amd import _abi
    lay = hp.operand_layout(_abi.Strategy(_abi.KINDS[kind], c, log_m, log_r))
    x, y = operands_for((lay.operands, lay.chunk_bits, lay.msb_first), c, lookups, np.random.default_rng(seed))
    if kind == "range":
        x = x & np.uint64((1 << log_r) - 1)
    return lay, x, y


def run_child(lib, curve, cases, env_extra, timeout=300):
    env = dict(os.environ); env.pop("LASSO_DENSIFY_OPERANDS", None); env.update(env_extra)
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib or "", curve, json.dumps(cases)], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])
