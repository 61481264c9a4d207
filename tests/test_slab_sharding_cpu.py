"""CPU: ONE proof sharded over P ranks (slab mode): every polynomial split by low index bits, partial sums all-gathered each round,
partial Hyrax row commitments exchanged and added, replicated transcript.  The ranks run as threads against the oracle's mock of the device ABI
(tests/cpp/slab_threads.cpp); the commitment and the proof must be byte-identical to the single-rank prover's AND to the oracle prover's, for
P = 2, 4, 8 and every strategy.  The torch.distributed (gloo) collective itself is covered by tests/test_multirank_cpu.py."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lasso_amd import _abi
from proverutil import HostProver, OracleSession, build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_slab_lib(curve="curve25519"):
    return C.CDLL(build_mock_prover(curve, harness=["slab_threads.cpp"], extra_flags=["-pthread"]))


@pytest.fixture(scope="module")
def slab():
    return build_slab_lib()


@pytest.fixture(scope="module")
def host():
    hp = HostProver(C.CDLL(build_mock_prover()))
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def slab_bn254():
    return build_slab_lib("bn254")


@pytest.fixture(scope="module")
def host_bn254():
    hp = HostProver(C.CDLL(build_mock_prover("bn254")))
    yield hp
    hp.close()


def slab_prove(lib, world, S, num_memories, idx, r):
    idx = np.ascontiguousarray(idx, dtype=np.uint64); r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
    comm = (C.c_uint8 * (1 << 20))(); proof = (C.c_uint8 * (1 << 22))(); cl = C.c_size_t(); pl = C.c_size_t(); nc = C.c_size_t(); nb = C.c_size_t(); err = C.create_string_buffer(512)
    rc = lib.slab_prove_threads(world, C.byref(S), C.c_size_t(num_memories), idx.ctypes.data_as(C.c_void_p), C.c_size_t(idx.shape[0]), r.ctypes.data_as(C.c_void_p), C.c_size_t(r.shape[0]),
                                comm, C.c_size_t(len(comm)), C.byref(cl), proof, C.c_size_t(len(proof)), C.byref(pl), C.byref(nc), C.byref(nb), err, C.c_size_t(512))
    assert rc == 0, err.value.decode()
    return bytes(comm[: cl.value]), bytes(proof[: pl.value]), nc.value, nb.value


# (kind, C, log_m, log_r, lookups): every strategy; ragged lookups; sizes where late layers are smaller than the world (replicated tops)
CASES = [("and", 1, 4, 0, 64), ("and", 2, 4, 0, 32), ("xor", 3, 4, 0, 50), ("or", 2, 6, 0, 16), ("lt", 2, 6, 0, 32), ("range", 3, 8, 40, 16), ("and", 1, 8, 0, 1 << 9), ("xor", 4, 6, 0, 100),
         ("spark", 2, 4, 0, 64), ("spark", 3, 6, 0, 100)]   # "spark" = LASSO_SPARK_UNCONFIRMED: the strategy BASELINE.json configs[4] names, restated (not in the reference snapshot)


@pytest.mark.parametrize("world", [2, 4, 8])
@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", CASES)
def test_slab_proof_equals_single_rank_and_oracle(slab, host, oracle, world, kind, c, log_m, log_r, lookups):
    _slab_case(slab, host, oracle, world, kind, c, log_m, log_r, lookups)


@pytest.mark.parametrize("world", [2, 8])
@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", [CASES[0], CASES[2], CASES[4], CASES[6]])
def test_slab_proof_bn254(slab_bn254, host_bn254, oracle_bn254, world, kind, c, log_m, log_r, lookups):
    """The same over G = BN254 (partial row commitments of the ranks are added with the complete projective addition; all-zero slabs are the identity (0 : 1 : 0))."""
    _slab_case(slab_bn254, host_bn254, oracle_bn254, world, kind, c, log_m, log_r, lookups)


def _slab_case(slab, host, oracle, world, kind, c, log_m, log_r, lookups):
    s = 1 << (lookups - 1).bit_length()
    nv_m = (c - 1).bit_length() + log_m
    if s < 2 * world or (1 << log_m) < 2 * world or (1 << (nv_m - nv_m // 2)) < world:
        pytest.skip("fewer than 2 elements, or less than one Hyrax column, per rank")
    alpha = 2 * c if kind == "lt" else c
    idx = np.random.default_rng(world * 1000 + lookups + c).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = host.gen_random_point(s.bit_length() - 1)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    comm_p, proof_p, ncoll, nbytes = slab_prove(slab, world, S, alpha, idx, r)
    gens = host.gens(c, s, alpha, log_m); dense = host.densify(idx, log_m)
    comm_1 = host.commit(dense, gens); proof_1 = host.prove(dense, gens, S, r)
    host.free(dense, gens)
    assert comm_p == comm_1 and proof_p == proof_1
    assert ncoll > 0 and nbytes / ncoll < 1 << 20          # many small collectives (per-round sums), never a polynomial
    orc = OracleSession(oracle, _abi.KINDS[kind], c, log_m, log_r, idx, r)
    try:
        assert comm_p == orc.commit() and proof_p == orc.prove() and orc.verify(proof_p, comm_p) == 1
    finally:
        orc.close()


@pytest.mark.parametrize("world,capacity", [(2, False), (4, True)])
def test_slab_threads_over_the_shm_exchange_and_capacity_mode(slab, host, world, capacity):
    """The harness the full-size GPU test uses (slab_prove_threads_ex: lasso_host_set_comm_shm between the ranks of one process, lasso_host_set_capacity, repeated proofs): the same
    bytes as the single-rank prover, every repeat identical."""
    kind, c, log_m, log_r, lookups = "xor", 2, 6, 0, 100
    s = 1 << (lookups - 1).bit_length()
    idx = np.ascontiguousarray(np.random.default_rng(world).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64))
    r = np.ascontiguousarray(host.gen_random_point(s.bit_length() - 1), dtype=np.uint64)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    comm = (C.c_uint8 * (1 << 20))(); proof = (C.c_uint8 * (1 << 22))(); cl = C.c_size_t(); pl = C.c_size_t(); nc = C.c_size_t(); nb = C.c_size_t(); err = C.create_string_buffer(512)
    peak = (C.c_uint64 * world)(); used = (C.c_uint64 * world)(); ms = C.c_double()
    rc = slab.slab_prove_threads_ex(world, C.byref(S), C.c_size_t(c), idx.ctypes.data_as(C.c_void_p), C.c_size_t(lookups), r.ctypes.data_as(C.c_void_p), C.c_size_t(r.shape[0]),
                                    f"/lasso_test_slab_ex_{os.getpid()}_{world}".encode(), 1 if capacity else 0, 3, comm, C.c_size_t(len(comm)), C.byref(cl), proof, C.c_size_t(len(proof)), C.byref(pl),
                                    C.byref(nc), C.byref(nb), peak, used, C.byref(ms), err, C.c_size_t(512))
    assert rc == 0, err.value.decode()
    gens = host.gens(c, s, c, log_m); dense = host.densify(idx, log_m)
    try:
        assert bytes(comm[: cl.value]) == host.commit(dense, gens) and bytes(proof[: pl.value]) == host.prove(dense, gens, S, r)
    finally:
        host.free(dense, gens)
    assert all(u > 0 for u in used)     # the prover's own accounting (the mock does not track device bytes)


_SLAB_SWITCH_SCRIPT = r"""
import ctypes as C, hashlib, sys
sys.path.insert(0, "tests")
import numpy as np
from lasso_amd import _abi
import test_slab_sharding_cpu as T
from proverutil import HostProver, build_mock_prover
lib = T.build_slab_lib()
hp = HostProver(C.CDLL(build_mock_prover()))
for world, (kind, c, log_m, log_r, lookups) in [(2, T.CASES[0]), (4, T.CASES[2]), (8, T.CASES[6]), (2, T.CASES[4])]:
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    alpha = 2 * c if kind == "lt" else c
    s = 1 << (lookups - 1).bit_length()
    idx = np.random.default_rng(world * 1000 + lookups + c).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = hp.gen_random_point(s.bit_length() - 1)
    comm, proof, _, _ = T.slab_prove(lib, world, S, alpha, idx, r)
    print("DIGEST", hashlib.sha256(comm + proof).hexdigest())
"""


@pytest.mark.parametrize("env", [{"LASSO_SLAB_AHEAD": "0"}, {"LASSO_SLAB_HOST_TAIL": "0"}, {"LASSO_SLAB_HOST_TOPS": "0"}, {"LASSO_SLAB_AHEAD": "0", "LASSO_SLAB_HOST_TAIL": "0", "LASSO_SLAB_HOST_TOPS": "0"},
                                 {"LASSO_ROUNDS_AHEAD": "0"}])
def test_slab_schedule_switches_do_not_change_the_bytes(env):
    """Round 6 brought round 5's schedule to slab mode: rounds launched ahead of their challenge with the cross-rank exchange in between (LASSO_SLAB_AHEAD), and the last log2 P
    rounds of every layer on the host from one all-gather of the local heads instead of uploads + a device phase (LASSO_SLAB_HOST_TAIL), and the replicated top layers P .. 2 of
    every tree built and proved on the host from the all-gathered local roots (LASSO_SLAB_HOST_TOPS).  All of it only moves WHERE and WHEN the same
    field arithmetic runs: with either switched off (round 5's schedule) commitment and proof bytes are the default's (each setting in its own process: the switches are read once).
    The defaults themselves are held to the oracle by test_slab_proof_equals_single_rank_and_oracle above."""
    import sys

    def run(extra):
        e = dict(os.environ)
        for k in ("LASSO_SLAB_AHEAD", "LASSO_SLAB_HOST_TAIL", "LASSO_SLAB_HOST_TOPS", "LASSO_ROUNDS_AHEAD"):
            e.pop(k, None)
        e.update(extra); e["PYTHONPATH"] = ROOT + os.pathsep + e.get("PYTHONPATH", "")
        out = subprocess.run([sys.executable, "-c", _SLAB_SWITCH_SCRIPT], env=e, cwd=ROOT, capture_output=True, text=True, timeout=900)
        assert out.returncode == 0, out.stderr[-2000:]
        return [l.split()[1] for l in out.stdout.splitlines() if l.startswith("DIGEST")]
    want = run({})
    assert len(want) == 4
    assert run(env) == want
