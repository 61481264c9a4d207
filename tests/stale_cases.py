"""The host prover over the oracle's mock with LASSO_POISON=1: every lasso_alloc of the mock holds the word 0x00000001 repeated (oracle/mock_hip.cpp, the device library's own
switch and word: lasso_amd/csrc/device_switches.cuh), so a prover that reads a pool buffer it has not written, or counts on a zeroed allocation, produces other bytes than the
oracle.  Not collected by name: tests/test_stale_memory_cpu.py runs it in a child process, the switch being read once per process."""
import ctypes as C
import os

import numpy as np
import pytest

from lasso_amd import _abi
from proverutil import HostProver, OracleSession, build_mock_prover
from test_fuzz_host_cpu import run as fuzz_run
from test_host_prover_cpu import CASES

CURVES = ["curve25519", "bn254"]
POISON_WORD = 0x00000001
FUZZ_COUNT = 8      # of the 40 configurations per seed of tests/test_fuzz_host_cpu.py: the first ones of the same seeds


@pytest.fixture(scope="module")
def hosts():
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = HostProver(C.CDLL(build_mock_prover(curve)))
        return made[curve]
    yield get
    for hp in made.values():
        hp.close()


@pytest.fixture
def oracle_of(oracle, oracle_bn254):
    return {"curve25519": oracle, "bn254": oracle_bn254}.__getitem__


@pytest.mark.parametrize("curve", CURVES)
def test_stale_switch_is_live_in_the_mock(curve):
    assert os.environ.get("LASSO_POISON") == "1", "the child runs without LASSO_POISON=1"
    from lasso_amd import Device
    lib = C.CDLL(build_mock_prover(curve)); _abi.declare(lib)
    d = Device(0, lib=lib)
    try:
        for nbytes in (4096, 6001, 1):
            p = d.alloc(nbytes)
            got = d.download(p, nbytes, dtype=np.uint8)
            d.free(p)
            want = np.zeros(nbytes, dtype=np.uint8); want[::4] = POISON_WORD
            assert np.array_equal(got, want), f"a fresh lasso_alloc of {nbytes} bytes of the {curve} mock does not hold the fill word"
    finally:
        d.close()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", CASES)
def test_stale_cases_give_the_oracles_bytes(hosts, oracle_of, curve, kind, c, log_m, log_r, lookups):
    host, oracle = hosts(curve), oracle_of(curve)
    s = 1 << (lookups - 1).bit_length()
    idx = host.gen_indices(lookups, 1 << log_m, c)
    if kind == "xor" and c == 3:
        idx = np.random.default_rng(3).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64)
    r = host.gen_random_point(max(s.bit_length() - 1, 0))
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens = host.gens(c, s, 2 * c if kind == "lt" else c, log_m)
    dense = host.densify(idx, log_m)
    comm = host.commit(dense, gens)
    proof = host.prove(dense, gens, S, r)
    again = host.prove(dense, gens, S, r)      # the second proof runs on the pool's recycled buffers
    host.free(dense, gens)
    orc = OracleSession(oracle, _abi.KINDS[kind], c, log_m, log_r, idx, r)
    try:
        assert comm == orc.commit()
        assert proof == orc.prove() and again == proof
        assert orc.verify(proof, comm) == 1
    finally:
        orc.close()


@pytest.mark.parametrize("curve,seed", [("curve25519", 2024), ("bn254", 2025)])
def test_stale_fuzz_gives_the_oracles_bytes(hosts, oracle_of, curve, seed):
    fuzz_run(hosts(curve), oracle_of(curve), seed, FUZZ_COUNT)
