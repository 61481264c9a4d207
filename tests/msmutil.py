"""Helpers of the tests of the MSM over caller points (tests/test_msm_points_cpu.py, tests/test_gpu_msm_points.py): the CPU build of the host prover against the mock with
lasso_msm_points added (tests/cpp/mock_msm_points_wrap.cpp), and a child-process verifier for the settings that are read once per process."""
import json
import os
import subprocess
import sys
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mock_prover_msm(curve="curve25519"):
    """the host prover over the mock with lasso_msm_points (tests/cpp/mock_msm_points_wrap.cpp: the mock's literal MSM)"""
    return build_mock_prover(curve, ext=("msm_points",))


# A verify in a FRESH process: LASSO_VERIFY_MSM_POINTS is read once per process.  argv: library ("" = the product library of `curve`), curve, kind, c, log_m, log_r, lookups.
# Proves the instance, verifies the honest proof and one with a flipped commitment-row bit, and prints one JSON line: verdicts (True / False / the error text), the
# msm_stats after the honest verify and after both, and the bytes (hex) so that the parent can hand them to the oracle's verifier (the lookups are child_indices(case)).
CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import _abi
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver
lib, curve, kind, c, log_m, log_r, lookups = sys.argv[2], sys.argv[3], sys.argv[4], *map(int, sys.argv[5:9])
hp = HostProver(C.CDLL(lib) if lib else None, curve=curve)
s = 1 << max((lookups - 1).bit_length(), 0)
alpha = 2 * c if kind == "lt" else c
idx = np.random.default_rng(11 + lookups).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
r = hp.gen_random_point(max(s.bit_length() - 1, 0))
S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
gens = hp.gens(c, s, alpha, log_m)
dense = hp.densify(idx, log_m)
comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, S, r)
def outcome(p, cm):
    try:
        return hp.verify(gens, S, s, r, p, cm)
    except LassoError as e:
        return str(e)
hp.msm_stats(reset=True)
honest = outcome(proof, comm); st1 = hp.msm_stats()
bad = bytearray(comm); bad[8 + 32 * (3 % max(1, (len(comm) - 16) // 64)) + 2] ^= 0x10
tampered = outcome(proof, bytes(bad)); st2 = hp.msm_stats()
print(json.dumps({"honest": honest, "tampered": tampered, "stats_honest": st1, "stats_both": st2, "proof": proof.hex(), "comm": comm.hex(), "bad_comm": bytes(bad).hex(),
                  "r": np.asarray(r).tolist()}))
hp.free(dense, gens); hp.close()
"""


def child_indices(case):
    """the lookups CHILD proves for `case`"""
    import numpy as np
    return np.random.default_rng(11 + case[4]).integers(0, 1 << case[2], size=(case[4], case[1]), dtype=np.uint64)


def verify_in_child(lib, curve, case, env_extra, timeout=120):
    """run CHILD for `case` = (kind, c, log_m, log_r, lookups) with env_extra added to the environment; returns the decoded JSON line"""
    env = dict(os.environ); env.update(env_extra)
    res = subprocess.run([sys.executable, "-c", CHILD, ROOT, lib or "", curve, case[0], *map(str, case[1:])], capture_output=True, text=True, timeout=timeout, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])
