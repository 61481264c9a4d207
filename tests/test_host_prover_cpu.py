"""CPU: the product's C++ host prover (lasso_amd/host/) driven end-to-end through the device C ABI, with the oracle's mock
of that ABI standing in for the GPU.  Pins the transcript schedule and wire format: proof bytes and commitment bytes must
equal the oracle prover's, and the oracle verifier (restating surge.rs:214-271) must accept them."""
import ctypes as C

import numpy as np
import pytest

from lasso_amd import _abi
from proverutil import HostProver, OracleSession, build_mock_prover, cubic_batched_case

# (kind, C, log_m, log_r, lookups) — the reference's e2e_test.rs configurations first
CASES = [("lt", 4, 4, 0, 16), ("lt", 4, 4, 0, 128), ("and", 4, 4, 0, 16), ("range", 3, 8, 40, 16),
         ("and", 1, 4, 0, 64), ("xor", 2, 4, 0, 32), ("or", 2, 4, 0, 8), ("and", 1, 16, 0, 1 << 10), ("and", 1, 4, 0, 2), ("xor", 3, 4, 0, 11),
         ("and", 1, 2, 0, 3), ("or", 1, 6, 0, 7), ("lt", 1, 4, 0, 4), ("range", 2, 4, 6, 9), ("and", 3, 2, 0, 4),   # smallest tables / ragged counts / C not a power of two
         ("spark", 1, 4, 0, 16), ("spark", 2, 4, 0, 32), ("spark", 3, 6, 0, 50), ("spark", 4, 4, 0, 256), ("spark", 8, 4, 0, 64), ("spark", 16, 2, 0, 32)]   # "spark" = LASSO_SPARK_UNCONFIRMED: the strategy BASELINE.json configs[4] names, restated (not in the reference snapshot)


@pytest.fixture(scope="module")
def host():
    hp = HostProver(C.CDLL(build_mock_prover()))
    yield hp
    hp.close()


def test_harness_inputs_match_oracle(host, oracle):
    s, m = 100, 1 << 16
    a = host.gen_indices(s, m, 1)[:, 0]
    b = np.empty(s, dtype=np.uint64)
    oracle.orc_gen_indices(C.c_size_t(s), C.c_size_t(m), b.ctypes.data_as(C.c_void_p))
    assert np.array_equal(a, b)
    ra = host.gen_random_point(20)
    rb = np.empty((20, 4), dtype=np.uint64)
    oracle.orc_gen_random_point(C.c_size_t(20), rb.ctypes.data_as(C.c_void_p))
    assert np.array_equal(ra, rb)


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", CASES)
def test_proof_bytes_equal_oracle_and_verify(host, oracle, kind, c, log_m, log_r, lookups):
    s = 1 << (lookups - 1).bit_length()
    alpha = 2 * c if kind == "lt" else c
    idx = host.gen_indices(lookups, 1 << log_m, c)
    if kind == "xor" and c == 3:       # ragged + distinct per-dimension indices (the harness replicates one draw; exercise the general case too)
        idx = np.random.default_rng(3).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = host.gen_random_point(max(s.bit_length() - 1, 0))
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = host.gens(c, s, alpha, log_m)
    dense = host.densify(idx, log_m)
    comm = host.commit(dense, gens)
    proof = host.prove(dense, gens, S, r)
    host.free(dense, gens)
    orc = OracleSession(oracle, _abi.KINDS[kind], c, log_m, log_r, idx, r)
    try:
        assert comm == orc.commit()
        assert proof == orc.prove()
        assert orc.verify(proof, comm) == 1
        bad = bytearray(proof); bad[len(bad) // 2] ^= 1
        try:
            assert orc.verify(bytes(bad), comm) != 1
        except Exception:
            pass
    finally:
        orc.close()


@pytest.mark.parametrize("k,ell,special", [(1, 1, {}), (2, 3, {}), (3, 5, {0: 0}), (2, 5, {2: 0}), (2, 4, {3: 0}), (2, 5, {1: 1}), (1, 6, {0: 0, 1: 1, 2: 0, 5: 1}), (2, 8, {7: 0}),
                                          (33, 2, {1: 0}), (2, 9, {}), (2, 9, {0: 1, 8: 0}), (2, 12, {}), (3, 12, {2: 0}), (2, 13, {1: 1, 5: 0})])   # ell >= 11: streaming rounds before the resident tail
def test_cubic_batched_scripted_eq_points(host, oracle, k, ell, special):
    cubic_batched_case(host, oracle, k, ell, special, seed=k * 100 + ell)


_SWITCH_SCRIPT_CPU = """
import ctypes as C, hashlib, sys
sys.path.insert(0, "tests")
from lasso_amd import _abi
from proverutil import HostProver, build_mock_prover
hp = HostProver(C.CDLL(build_mock_prover()))
for kind, c, log_m, log_s in (("and", 2, 12, 12), ("xor", 1, 16, 11), ("lt", 2, 4, 9)):
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
    idx = hp.gen_indices(1 << log_s, 1 << log_m, c); r = hp.gen_random_point(log_s)
    gens = hp.gens(c, 1 << log_s, 2 * c if kind == "lt" else c, log_m); dense = hp.densify(idx, log_m)
    print("DIGEST", hashlib.sha256(hp.commit(dense, gens) + hp.prove(dense, gens, S, r)).hexdigest())
"""


@pytest.mark.parametrize("env", [{"LASSO_HOST_TAIL": "0"}, {"LASSO_ROUNDS_AHEAD": "0"}, {"LASSO_HOST_TAIL": "0", "LASSO_ROUNDS_AHEAD": "0", "LASSO_BULLET_AHEAD": "0"},
                                 {"LASSO_HOST_TAIL": "128"}, {"LASSO_HOST_TAIL": "4"}, {"LASSO_CUBIC_TAIL": "0"}, {"LASSO_CUBIC_TAIL": "0", "LASSO_HOST_TAIL": "0"},
                                 {"LASSO_CAPACITY": "1", "LASSO_LEAFLESS_MIN": "64"}, {"LASSO_CAPACITY": "1", "LASSO_LEAFLESS_MIN": "64", "LASSO_HOST_TAIL": "0", "LASSO_ROUNDS_AHEAD": "0"},
                                 {"LASSO_LAYER_AHEAD": "0"}, {"LASSO_LAYER_AHEAD": "1", "LASSO_HOST_TAIL": "0"}, {"LASSO_LAYER_AHEAD": "1", "LASSO_ROUNDS_AHEAD": "0"},
                                 {"LASSO_HOST_IFMA": "0"}, {"LASSO_HOST_IFMA": "0", "LASSO_HOST_TAIL": "128"}, {"LASSO_HOST_IFMA": "1", "LASSO_HOST_TAIL": "512"}, {"LASSO_HOST_IFMA": "1", "LASSO_HOST_TAIL": "8"},
                                 {"LASSO_CUBIC_THREE_SUMS": "1"},      # every streaming layer enqueued ahead turns out to have "another shape": lasso_point_cancel, then the plain path
                                 {"LASSO_CUBIC_THREE_SUMS": "1", "LASSO_LAYER_AHEAD": "0"},
                                 {"LASSO_BULLET_TAIL_AHEAD": "0"},     # round 6: the openings' last fold, heads and delta MSM as separate calls after the last challenge
                                 {"LASSO_SIDE_STREAM": "0"},           # no openings prepared ahead: the block pass on the main context, inside poly_eval_prove_resident
                                 {"LASSO_SIDE_STREAM": "0", "LASSO_CAPACITY": "1", "LASSO_LEAFLESS_MIN": "64"}])
def test_host_schedule_switches_do_not_change_the_bytes(env):
    """Round 5's host-side schedule — rounds launched ahead of their challenge, resident tails that hand their arrays to the host, tree-top layers proved on the host — selects
    WHERE and WHEN the same field arithmetic runs: with every combination of the switches the commitment and proof bytes are those of the default (each setting in its own process:
    the switches are read once).  CPU twin (mock device ABI) of tests/test_gpu_prover.py::test_gpu_ab_switches_do_not_change_the_bytes."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

    def run(extra):
        e = dict(os.environ); e.pop("LASSO_HOST_TAIL", None); e.pop("LASSO_ROUNDS_AHEAD", None); e.pop("LASSO_LAYER_AHEAD", None); e.pop("LASSO_HOST_IFMA", None); e.pop("LASSO_CUBIC_THREE_SUMS", None); e.pop("LASSO_SIDE_STREAM", None); e.update(extra); e["PYTHONPATH"] = root + os.pathsep + e.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", _SWITCH_SCRIPT_CPU], env=e, cwd=root, capture_output=True, text=True, timeout=600)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l.split()[1] for l in out.stdout.splitlines() if l.startswith("DIGEST")]
    want = run({})
    assert len(want) == 3
    assert run(env) == want


@pytest.mark.parametrize("k,ell,special", [(1, 0, {}), (2, 1, {}), (2, 3, {}), (3, 4, {0: 0}), (2, 4, {2: 0}), (2, 4, {3: 1}), (1, 5, {0: 0, 1: 1, 2: 0, 4: 1}), (16, 2, {1: 0}), (2, 5, {0: 1, 4: 0})])
def test_host_rounds_scripted_eq_points(host, oracle, k, ell, special, monkeypatch):
    """Prover::host_cubic_rounds (the rounds the host finishes / the tree tops' layers, prover.hpp) against the oracle's literal prove_cubic_batched at the eq points no transcript
    produces (coordinates 0 and 1), through the same debug entry as the device rounds above (LASSO_DEBUG_CUBIC_HOST=1 routes it to the host rounds)."""
    monkeypatch.setenv("LASSO_DEBUG_CUBIC_HOST", "1")
    if ell == 0:
        pytest.skip("the debug entry needs at least one round")
    cubic_batched_case(host, oracle, k, ell, special, seed=7000 + k * 100 + ell)
