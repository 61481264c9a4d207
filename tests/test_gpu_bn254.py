"""-m gpu: the BN254 build of the HIP path (liblasso_prover_bn254.so over liblasso_hip_bn254.so: the same kernels over ark-bn254's Fr / G1,
csrc/bn254_fr.cuh, fr29.cuh, bn254_fq.cuh, bn254_fe29.cuh over mont32.cuh / mont29.cuh) against the oracle's BN254 instantiation — G = BN254 is the group BASELINE.json's configs[1] names.
Commitment and proof bytes identical to the oracle prover's; at configs[1]'s full size the reference's own acceptance property
prove -> verify (src/e2e_test.rs:54-59) through the oracle verifier, tamper rejection and determinism."""
import ctypes as C

import numpy as np
import pytest

from lasso_amd import _abi
from proverutil import OracleSession

pytestmark = pytest.mark.gpu

CASES = [("lt", 4, 4, 0, 16), ("and", 4, 4, 0, 16), ("range", 3, 8, 40, 16), ("and", 1, 4, 0, 2), ("xor", 3, 4, 0, 11), ("or", 2, 4, 0, 8),
         ("and", 1, 16, 0, 1 << 10), ("and", 4, 16, 0, 1 << 12), ("xor", 8, 8, 0, 1 << 10), ("and", 1, 16, 0, 1 << 14),
         ("spark", 2, 8, 0, 300), ("spark", 4, 16, 0, 1 << 12), ("spark", 16, 4, 0, 64)]   # LASSO_SPARK_UNCONFIRMED over BN254


@pytest.fixture(scope="module")
def host():
    from lasso_amd import HostProver
    hp = HostProver(curve="bn254")            # product library (BN254 pair); raises if the extension or the GPU is missing
    yield hp
    hp.close()


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", CASES)
def test_gpu_bn254_proof_bit_exact_vs_oracle(host, oracle_bn254, kind, c, log_m, log_r, lookups):
    alpha = 2 * c if kind == "lt" else c
    s = 1 << max((lookups - 1).bit_length(), 0)
    idx = host.gen_indices(lookups, 1 << log_m, c)
    if (kind, c) == ("xor", 3):
        idx = np.random.default_rng(7).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = host.gen_random_point(max(s.bit_length() - 1, 0))
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = host.gens(c, s, alpha, log_m)
    dense = host.densify(idx, log_m)
    comm = host.commit(dense, gens)
    proof = host.prove(dense, gens, S, r)
    proof2 = host.prove(dense, gens, S, r)
    accepted = host.verify(gens, S, s, r, proof, comm)      # product-side verifier, BN254 build
    host.free(dense, gens)
    assert proof == proof2
    assert accepted is True
    orc = OracleSession(oracle_bn254, _abi.KINDS[kind], c, log_m, log_r, idx, r)
    try:
        assert comm == orc.commit()
        assert proof == orc.prove()
        assert orc.verify(proof, comm) == 1
    finally:
        orc.close()


def test_gpu_bn254_baseline_config1_full_size(host, oracle_bn254):
    """BASELINE.json configs[1] as written: AND, C = 4, log_M = 16, 2^20 lookups, G = BN254."""
    kind, c, log_m, log_r, log_s = "and", 4, 16, 0, 20
    s = 1 << log_s
    idx = host.gen_indices(s, 1 << log_m, c)
    r = host.gen_random_point(log_s)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = host.gens(c, s, c, log_m)
    dense = host.densify(idx, log_m)
    comm = host.commit(dense, gens)
    import time
    proof = host.prove(dense, gens, S, r)
    t0 = time.perf_counter(); again = host.prove(dense, gens, S, r); dt = time.perf_counter() - t0
    host.free(dense, gens)
    assert proof == again
    print(f"\n[bn254] AND C=4 2^20 lookups: prove {dt * 1e3:.1f} ms ({s / dt:.3e} lookups/s), proof {len(proof)} bytes")
    rr = np.ascontiguousarray(r, dtype=np.uint64)
    o = oracle_bn254
    o.orc_verify_only.argtypes = [C.c_int, C.c_size_t, C.c_size_t, C.c_size_t, C.c_size_t, C.c_void_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    assert o.orc_verify_only(_abi.KINDS[kind], c, 1 << log_m, log_r, s, rr.ctypes.data_as(C.c_void_p), proof, len(proof), comm, len(comm)) == 1, o.orc_last_error()
    bad = bytearray(proof); bad[len(bad) // 2] ^= 0x04
    assert o.orc_verify_only(_abi.KINDS[kind], c, 1 << log_m, log_r, s, rr.ctypes.data_as(C.c_void_p), bytes(bad), len(bad), comm, len(comm)) != 1


def test_gpu_bn254_config1_bit_exact_at_full_size(host, oracle_bn254):
    """BASELINE.json configs[1] as written (AND, C = 4, log_M = 16, 2^20 lookups, G = BN254): commitment and proof BYTES identical to the oracle
    prover's on the harness inputs (the oracle runs on all host cores; bytes independent of the thread count)."""
    from proverutil import oracle_harness_proof
    kind, c, log_m, log_r, log_s = "and", 4, 16, 0, 20
    s = 1 << log_s
    idx = host.gen_indices(s, 1 << log_m, c)
    r = host.gen_random_point(log_s)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = host.gens(c, s, c, log_m)
    dense = host.densify(idx, log_m)
    comm = host.commit(dense, gens)
    proof = host.prove(dense, gens, S, r)
    host.free(dense, gens)
    o_comm, o_proof, tm = oracle_harness_proof(oracle_bn254, _abi.KINDS[kind], c, log_m, log_r, log_s)
    print(f"\n[oracle bn254] AND C=4 2^20: {tm['threads']} threads, commit {tm['commit_s']:.1f}s prove {tm['prove_s']:.1f}s")
    assert comm == o_comm
    assert proof == o_proof


def _rerun_on_bn254(module, extra=(), timeout=900):
    """a test module re-run in a child process with LASSO_TEST_CURVE=bn254 (the switch is read at import time by tests/fieldref.py, so it cannot share this process)"""
    import os
    import subprocess
    import sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LASSO_TEST_CURVE="bn254")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join(root, "tests", module), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", *extra],
                         cwd=root, env=env, capture_output=True, text=True, timeout=timeout)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout


def test_gpu_bn254_kernel_parity_suite():
    """Every entry point of the BN254 library against the BN254 mock: tests/test_gpu_kernels.py re-run in a child process with LASSO_TEST_CURVE=bn254."""
    _rerun_on_bn254("test_gpu_kernels.py")


def test_gpu_bn254_msm_over_caller_points():
    """tests/test_gpu_msm_points.py on the BN254 build (minus its two long cases): the short-Weierstrass build is where "the group laws are complete" (msm_points_kernels.cuh) is
    carried by the Renes-Costello-Batina formulas and the six-lane tree — test_degenerate_inputs (equal points, P and -P in one bucket, buckets that sum to the identity) is the
    test of that sentence, and on the Edwards build the unified addition is complete anyway."""
    _rerun_on_bn254("test_gpu_msm_points.py", ["-k", "not 2p17 and not 2p16"])


def test_gpu_bn254_custom_strategy_kernel_level():
    """Sections 5 and 9 of tests/test_gpu_custom_strategy.py (the tests over its `dev` fixture) on the BN254 build: every degree 1..17 of k_combine_round_custom, the caps exactly
    reached and all inputs at LAZY_BOUND over the wider Fr, whose fr29 magnitude arguments are its own.  (The whole-proof tests of that module take the curve as a parameter.)"""
    _rerun_on_bn254("test_gpu_custom_strategy.py", ["-k", "test_every_degree_one_term_and_several or test_sizes_and_memory_counts or test_repeated_memories_special_coefficients_and_constants "
                                                    "or test_caps_exactly_reached or test_all_inputs_at_the_lazy_bound_and_two_factor_terms_with_coefficient_one "
                                                    "or test_invalid_descriptor_at_the_device_entry_points"])


def test_gpu_bn254_msm_variants():
    """tests/test_gpu_msm_variants.py on the BN254 build: every switched MSM kernel against the BN254 mock."""
    _rerun_on_bn254("test_gpu_msm_variants.py")


def test_gpu_bn254_round_variants():
    """tests/test_gpu_round_variants.py on the BN254 build: every switched cubic-round kernel against the BN254 mock."""
    _rerun_on_bn254("test_gpu_round_variants.py")


def test_gpu_bn254_pass_variants():
    """tests/test_gpu_pass_variants.py on the BN254 build: every running sum of the sumcheck kernels through its fold, against the BN254 mock."""
    _rerun_on_bn254("test_gpu_pass_variants.py")


def test_gpu_bn254_write_contract():
    """tests/test_gpu_write_contract.py on the BN254 build: every child of it (the arena cases of tests/arena_cases.py by group and switch setting) inherits LASSO_TEST_CURVE."""
    _rerun_on_bn254("test_gpu_write_contract.py", timeout=1800)


def test_gpu_bn254_stale_memory():
    """tests/test_gpu_stale_memory.py on the BN254 build: the BN254 proofs above and the verifier and set-up modules under LASSO_POISON=1 (its children inherit LASSO_TEST_CURVE)."""
    _rerun_on_bn254("test_gpu_stale_memory.py", timeout=900)
