"""-m gpu: slab-mode proofs (ONE proof over P ranks, the ranks being P contexts of the one device driven by P threads: tests/cpp/slab_threads.cpp) under the host switches of
slab mode, on both curve builds, and throughput mode (lasso_host_set_throughput_mode) under both settings of LASSO_THROUGHPUT_AHEAD.  The host switches are read once per
process, so every setting is one child process; the expected bytes are the CPU oracle's (OracleSession), computed in this process.  Every comparison is byte equality.

  curve25519   LASSO_SLAB_OPEN=0 (every rank runs the WHOLE opening over the full generator set, its bullet rounds launched ahead of their challenges), the same with
               LASSO_BULLET_AHEAD=0, LASSO_SLAB_HOST_TAIL=0 (a layer's last log2 P rounds on replicated device arrays), LASSO_SLAB_HOST_TOPS=0 (the replicated top layers built
               and proved on the device), all three at 0: AND C=1 and Spark C=4 at 2^10 lookups over 2 and 8 ranks
  BN254        the default switches — the first device run of lasso_bullet_round_slab / lasso_msm_dev_slab inside a proof on that build — and LASSO_SLAB_OPEN=0: AND C=1, LT C=2
               (64 lookups) and Spark C=4 over 2 and 8 ranks, through a harness library built with lasso_amd/build.py's BN254 flags against liblasso_hip_bn254.so
  throughput   AND C=2 (log_m 16) and Spark C=2 (log_m 8) at 2^14 lookups: a host in throughput mode alone, then four such hosts proving at once in four threads, all against
               the digest of a plain host of the same process; once with no setting (Dev::no_ahead(): nothing of such a host is launched ahead of its challenge) and once
               under LASSO_THROUGHPUT_AHEAD=1 (launched ahead all the same).  Every host is set up (generators, densify, commit) before the first proof and freed after the
               last, one at a time, as bench.py's concurrent leg and test_gpu_concurrent_proofs_identical_to_sequential do.  A first form of the child did set-up and free
               inside the four threads, beside the other hosts' proofs: under LASSO_THROUGHPUT_AHEAD=1 two of the four hosts then got "lasso_result_wait failed (-3): a
               result was not delivered by the device" — their gate kernels had given up after 5 s without a post (poly_kernels.cuh k_gate) and their streams ended without a
               result (lasso_hip.hip wait_flag).  Supposed, not shown: allocations, frees and synchronous copies wait for the whole device, a waiting gate included, and hold up
               the other hosts' calls meanwhile.  Set-up beside launched-ahead proofs of other hosts is what that run says not to do; with no setting the same child passed.

Why LASSO_SLAB_OPEN=0 cannot make one rank wait for another inside the opening (DotProductProofLog::prove, lasso_amd/host/prover.hpp): with `shard` false, `ahead` is true for
every rank, so each rank enqueues round k + 1 behind a gate kernel on ITS context's stream and releases it with lasso_bullet_post on ITS context.  What a rank posts is the
challenge it draws from its own transcript after lasso_result_wait has returned ITS round k's L and R — a kernel that precedes the gate in the same stream, so it has ended
before the gate starts polling.  The only collective of the opening is sum_points, which runs under `shard` alone: in the replicated opening nothing between a round's enqueue and
its post involves another rank, and a waiting gate is one wave of one workgroup, which cannot keep another context's kernels off the device.
What DID stall such a proof once, at 8 ranks: without a collective at its end the ranks drift apart, and the thread harness let a rank that had finished free its polynomials,
generators and host while another was still inside its opening; rank 4 then got "a result was not delivered by the device" 5 s later — its gate had given up waiting for the
post (poly_kernels.cuh k_gate), as in throughput mode below.  A free waits for the whole device, which the ranks share here and nowhere else (supposed, not shown: it holds up
the other rank's stream query meanwhile, so its host cannot post).  tests/cpp/slab_threads.cpp now frees nothing before every rank is through with its proofs.

Out of reach on one device: LASSO_SLAB_AHEAD (ranks_share_a_device() switches the slab-local rounds launched ahead off; held over the mock in
tests/test_slab_sharding_cpu.py) and LASSO_SLAB_RCCL (RCCL declines ranks that share a device, tests/test_gpu_kernels.py test_rccl_two_ranks_on_one_device, so the bulk exchange
takes the shared-memory route whatever the switch says; the mock has no RCCL either, so the RCCL route of lasso_host_set_comm_shm stays without a test).

After a child that did not end normally nothing more is started on the GPU by this module.  The harness libraries are built before a child's time limit (240 s) starts.
Measured on an MI355X, seconds per child (its whole life: imports, four or six slab proofs with up to 8 contexts and their generator tables each, or the six hosts of throughput
mode): curve25519 1.5 to 1.6 under each of the five settings, BN254 2.6 and 2.7, throughput mode 1.1 and 2.1; under 20 s for the module, most of it the oracle's proofs in this
process."""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest

from gpuutil import rand_fr
from lasso_amd import _abi
from proverutil import OracleSession

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TIMEOUT = 240
_dead = []          # why nothing more may be started

AND = ("and", 1, 8, 0, 1 << 10)
LT = ("lt", 2, 6, 0, 64)
SPARK = ("spark", 4, 8, 0, 1 << 10)
WORLDS = (2, 8)      # 2 first: the smallest number of contexts side by side
ALL_OFF = {"LASSO_SLAB_OPEN": "0", "LASSO_SLAB_HOST_TAIL": "0", "LASSO_SLAB_HOST_TOPS": "0"}
SETTINGS_25519 = [{"LASSO_SLAB_OPEN": "0"}, {"LASSO_SLAB_OPEN": "0", "LASSO_BULLET_AHEAD": "0"}, {"LASSO_SLAB_HOST_TAIL": "0"}, {"LASSO_SLAB_HOST_TOPS": "0"}, ALL_OFF]
SETTINGS_BN254 = [{}, {"LASSO_SLAB_OPEN": "0"}]
SLAB_SWITCHES = ("LASSO_SLAB_OPEN", "LASSO_SLAB_HOST_TAIL", "LASSO_SLAB_HOST_TOPS", "LASSO_SLAB_RCCL", "LASSO_SLAB_AHEAD", "LASSO_BULLET_AHEAD", "LASSO_THROUGHPUT_AHEAD")


def _env_id(env):
    return "default" if not env else ",".join(f"{k}={v}" for k, v in sorted(env.items()))


def _build_slab_hip(curve="curve25519"):
    """tests/cpp/slab_threads.cpp with the host prover, linked against the device library of `curve` -> the path of the harness library (tests/test_gpu_prover.py
    _build_slab_hip builds the same file for curve25519).  Compiling needs no GPU; the library is loaded in a child process only."""
    from lasso_amd import build
    suffix, flags = build.CURVES[curve]
    out_dir = os.path.join(ROOT, "tests", "_build"); os.makedirs(out_dir, exist_ok=True)
    so = os.path.join(out_dir, f"libslab_threads_hip{suffix}.so")
    srcs = [os.path.join(ROOT, "tests", "cpp", "slab_threads.cpp"), os.path.join(ROOT, "lasso_amd", "host", "prover_capi.cpp")]
    lib_dir = os.path.join(ROOT, "lasso_amd")
    if not os.path.exists(so) or any(os.path.getmtime(x) > os.path.getmtime(so) for x in srcs + [os.path.join(lib_dir, f"liblasso_hip{suffix}.so"), os.path.join(lib_dir, "host", "prover.hpp")]):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-pthread", "-Wno-unknown-pragmas", *flags, "-o", so] + srcs + ["-L" + lib_dir, f"-llasso_hip{suffix}", "-Wl,-rpath," + lib_dir])
    return so


def _child(script, args, env_extra, what):
    """one child process under `env_extra` and no other slab switch -> its standard output; a child that does not end normally is the last one this module starts"""
    if _dead:
        pytest.fail("not started: an earlier child of this module did not end normally (" + _dead[0] + ")")
    env = {k: v for k, v in os.environ.items() if k not in SLAB_SWITCHES}
    env.update(env_extra)
    t0 = time.perf_counter()
    try:
        res = subprocess.run([sys.executable, "-c", script, ROOT] + args, capture_output=True, text=True, timeout=TIMEOUT, env=env, cwd=ROOT)
    except subprocess.TimeoutExpired:
        _dead.append(f"time limit of {TIMEOUT} s: {what}")
        raise
    print(f"\n[slab switches] {what}: {time.perf_counter() - t0:.1f} s")
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
        _dead.append(f"exit status {res.returncode}: {what}")
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return res.stdout


# ---- slab proofs: the child proves every job through slab_prove_threads of the harness library and leaves commitment and proof as files

_SLAB_CHILD = """
import ctypes as C, json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1])
from lasso_amd import _abi
lib = C.CDLL(sys.argv[2])
job_dir = sys.argv[3]
jobs = json.load(open(os.path.join(job_dir, "jobs.json")))
for j in jobs:      # in the order given; the first failure ends the child
    idx = np.load(os.path.join(job_dir, j["case"] + ".idx.npy")); r = np.load(os.path.join(job_dir, j["case"] + ".r.npy"))
    S = _abi.Strategy(_abi.KINDS[j["kind"]], j["c"], j["log_m"], j["log_r"])
    comm = (C.c_uint8 * (1 << 22))(); proof = (C.c_uint8 * (1 << 22))(); cl = C.c_size_t(); pl = C.c_size_t(); nc = C.c_size_t(); nb = C.c_size_t(); err = C.create_string_buffer(512)
    rc = lib.slab_prove_threads(j["world"], C.byref(S), C.c_size_t(j["alpha"]), idx.ctypes.data_as(C.c_void_p), C.c_size_t(idx.shape[0]), r.ctypes.data_as(C.c_void_p), C.c_size_t(r.shape[0]),
                                comm, C.c_size_t(len(comm)), C.byref(cl), proof, C.c_size_t(len(proof)), C.byref(pl), C.byref(nc), C.byref(nb), err, C.c_size_t(512))
    if rc != 0:
        print("FAILED", j["name"], rc, err.value.decode(), flush=True)
        sys.exit(1)
    with open(os.path.join(job_dir, j["name"] + ".comm"), "wb") as f:
        f.write(bytes(comm[: cl.value]))
    with open(os.path.join(job_dir, j["name"] + ".proof"), "wb") as f:
        f.write(bytes(proof[: pl.value]))
    print("PROVED", j["name"], nc.value, flush=True)
print("DONE", len(jobs))
"""
_WANT = {}      # (curve, case) -> (indices, r, the oracle's commitment, the oracle's proof)


def _instance(orc, curve, case):
    if (curve, case) not in _WANT:
        kind, c, log_m, log_r, lookups = case
        rng = np.random.default_rng([lookups, c, log_m])
        idx = np.ascontiguousarray(rng.integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64))
        r = np.ascontiguousarray(rand_fr(rng, (lookups - 1).bit_length(), edge=False))      # any value below 2^252 is a field element in memory form on both curves
        o = OracleSession(orc, _abi.KINDS[kind], c, log_m, log_r, idx, r)
        try:
            comm, proof = o.commit(), o.prove()
            assert o.verify(proof, comm) == 1
        finally:
            o.close()
        _WANT[curve, case] = (idx, r, comm, proof)
    return _WANT[curve, case]


def _slab_proofs(orc, curve, cases, env, tmp_path):
    so = _build_slab_hip(curve)      # before the child's time limit starts
    jobs = []
    for world in WORLDS:
        for case in cases:
            kind, c, log_m, log_r, lookups = case
            idx, r, _, _ = _instance(orc, curve, case)
            name = f"{kind}_c{c}"
            np.save(tmp_path / f"{name}.idx.npy", idx); np.save(tmp_path / f"{name}.r.npy", r)
            jobs.append({"name": f"{name}_w{world}", "case": name, "world": world, "kind": kind, "c": c, "log_m": log_m, "log_r": log_r, "alpha": 2 * c if kind == "lt" else c})
    (tmp_path / "jobs.json").write_text(json.dumps(jobs))
    out = _child(_SLAB_CHILD, [so, str(tmp_path)], env, f"{curve} {_env_id(env)}")
    assert out.splitlines()[-1:] == [f"DONE {len(jobs)}"], out[-1000:]
    bad = []
    for j, (world, case) in zip(jobs, [(w, cs) for w in WORLDS for cs in cases]):
        _, _, comm, proof = _instance(orc, curve, case)
        if (tmp_path / (j["name"] + ".comm")).read_bytes() != comm:
            bad.append(f"{j['name']}: the commitment differs from the oracle's")
        if (tmp_path / (j["name"] + ".proof")).read_bytes() != proof:
            bad.append(f"{j['name']}: the proof differs from the oracle's")
    assert not bad, f"{curve} under {_env_id(env)}: " + "; ".join(bad)


@pytest.mark.parametrize("env", SETTINGS_25519, ids=[_env_id(e) for e in SETTINGS_25519])
def test_slab_proofs_under_the_host_switches(oracle_25519, env, tmp_path):
    _slab_proofs(oracle_25519, "curve25519", (AND, SPARK), env, tmp_path)


@pytest.mark.parametrize("env", SETTINGS_BN254, ids=[_env_id(e) for e in SETTINGS_BN254])
def test_slab_proofs_on_the_bn254_build(oracle_bn254, env, tmp_path):
    _slab_proofs(oracle_bn254, "bn254", (AND, LT, SPARK), env, tmp_path)


@pytest.fixture(scope="module")
def oracle_25519():
    """the curve25519 oracle whatever LASSO_TEST_CURVE says: this module names its curves itself"""
    from conftest import _build_oracle, _load_oracle
    return _load_oracle(_build_oracle())


# ---- throughput mode

_THROUGHPUT_CHILD = """
import hashlib, json, sys, threading
sys.path.insert(0, sys.argv[1])
from lasso_amd import HostProver, _abi
instances = json.loads(sys.argv[2])
out = {}
for kind, c, log_m, log_s in instances:
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)

    def set_up(throughput):      # one at a time, before anything proves: allocations and synchronous copies wait for the whole device
        hp = HostProver()
        if throughput:
            hp.set_throughput_mode(True)
        idx = hp.gen_indices(1 << log_s, 1 << log_m, c); r = hp.gen_random_point(log_s)
        gens = hp.gens(c, 1 << log_s, c, log_m); dense = hp.densify(idx, log_m)
        return hp, gens, dense, r, hp.commit(dense, gens)

    def digest(w):
        hp, gens, dense, r, comm = w
        return hashlib.sha256(comm + hp.prove(dense, gens, S, r)).hexdigest()
    plain, alone = set_up(False), set_up(True)
    four = [set_up(True) for _ in range(4)]
    want, one = digest(plain), digest(alone)
    got, errors = [None] * 4, []
    bar = threading.Barrier(4)

    def run(t):
        try:
            bar.wait(timeout=60)
            got[t] = digest(four[t])
        except Exception as e:      # a failed proof must not leave the others waiting at the barrier
            errors.append(repr(e)); bar.abort()
    ths = [threading.Thread(target=run, args=(t,)) for t in range(4)]
    for th in ths:
        th.start()
    for th in ths:
        th.join()
    for hp, gens, dense, r, comm in [plain, alone] + four:      # nothing is freed while a proof runs
        hp.free(dense, gens); hp.close()
    out[kind] = {"plain": want, "alone": one, "four": got, "errors": errors}
    if errors:
        break
print(json.dumps(out))
"""


@pytest.mark.parametrize("env", [{}, {"LASSO_THROUGHPUT_AHEAD": "1"}], ids=["default", "LASSO_THROUGHPUT_AHEAD=1"])
def test_throughput_mode_does_not_change_the_bytes(env):
    """a host in throughput mode, alone and as one of four proving at once, gives the commitment and proof of a plain host: with no setting nothing of it is launched ahead of
    its challenge (Dev::no_ahead()), under LASSO_THROUGHPUT_AHEAD=1 it launches ahead all the same, the gates and waiting tails of four proofs side by side on the device.
    The hosts are set up one after the other and freed after the last proof, as bench.py's concurrent leg does (the module's docstring says why)."""
    from test_gpu_prover import _SWITCH_INSTANCES
    instances = [list(_SWITCH_INSTANCES[k]) for k in ("and", "spark")]
    out = json.loads(_child(_THROUGHPUT_CHILD, [json.dumps(instances)], env, f"throughput mode, {_env_id(env)}").strip().split("\n")[-1])
    assert all(res["errors"] == [] for res in out.values()), {kind: res["errors"] for kind, res in out.items()}
    assert set(out) == {"and", "spark"}
    for kind, res in out.items():
        assert res["errors"] == [], (kind, res["errors"])
        assert res["alone"] == res["plain"], f"{kind}: a host in throughput mode proves other bytes than a plain host"
        assert res["four"] == [res["plain"]] * 4, f"{kind}: four hosts proving at once: {res['four']} against {res['plain']}"
