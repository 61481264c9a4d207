"""-m gpu: lasso_tables_mle / lasso_tables_mle_dev (include/lasso_hip_mle.h) on the real library, and the verifier's device route for caller-defined subtables.
All comparisons are exact (integers mod p).  Reference: Python big integers up to log_m = 12, the oracle's mock (lasso_eq_evals + lasso_multi_dot) above.
Runs on the build LASSO_TEST_CURVE selects; the last test re-runs the module on the BN254 build.

  kernel      log_m in mleutil.LOG_MS (tests/test_mle_cpu.py holds that list against the launch plan's boundaries), 1 .. 32 tables, both table forms
  tables      unit tables (the result is chi_i: bit order and the hi / lo split), all zero, all 0xFFFFFFFF, all p - 1, lazily reduced entries, random
  points      random, Boolean (the result is T[index]), a coordinate p - 1, lazily reduced coordinates
  folds       shapes at which every lane passes both fold periods at least twice, on maximal entries
  strips      LASSO_MLE_STRIP: a 2^10-entry table in three strips and a ragged one
  _dev        same results, tables untouched, under LASSO_SCRATCH_GUARD=1 in a child process, lasso_sync = 0
  arguments   every broken rule is LASSO_ERR_INVALID with a message, nothing launched, context usable
  verifier    custom proofs at 2^10 lookups, log_m = 8 and 16, u32 and Fr tables: device route = host route = the oracle's verifier, mle_stats proves the route"""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mleutil as M
from fieldref import CURVE, L as FR_P
from gpuutil import LAZY_BOUND, canon, full_fr, lift, load_mock, words

pytestmark = pytest.mark.gpu
ROOT = M.ROOT
ONE = (1 << 256) % FR_P


@pytest.fixture(scope="module")
def dev():
    from lasso_amd import Device
    d = Device(0, curve=CURVE)
    yield d
    d.close()


@pytest.fixture(scope="module")
def mock():
    from lasso_amd import Device
    d = Device(0, lib=load_mock())
    yield d
    d.close()


def rand_point(rng, log_m):
    return full_fr(rng, log_m)


def rand_u32(rng, n):
    t = rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32)
    t[:3] = [0, 1, 0xFFFFFFFF][:min(3, n)]
    return t


def rand_fr_table(rng, n):
    if n > 1 << 12:      # large tables: words below 2^252 (canonical on both curves) straight from numpy
        t = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
        t[:, 3] &= np.uint64(2**60 - 1)
    else:
        t = full_fr(rng, n)
    edge = words([0, ONE, FR_P - 1, 1])
    t[:min(4, n)] = edge[:min(4, n)]
    return t


def reference(mock, tables, point, field):
    """the memory words of sum_i T_k[i] chi_i for every table"""
    log_m = np.asarray(point).reshape(-1, 4).shape[0]
    if log_m <= 12:
        chi = M.chi_int(point, FR_P)
        return words([M.mle_int(t, chi, FR_P, field) for t in tables])
    n = 1 << log_m
    d_chi = mock.alloc(32 * n); mock.eq_evals(canon(point), d_chi)
    ptrs = []
    try:
        for t in tables:
            if field:
                ptrs.append(mock.upload(t if (np.asarray(t)[:, 3] < np.uint64(2**60)).all() else canon(t)))
            else:
                src = mock.upload(np.ascontiguousarray(t, dtype=np.uint32)); dst = mock.alloc(32 * n)
                mock.fr_from_u32(src, n, dst); mock.free(src); ptrs.append(dst)
        return canon(mock.multi_dot(ptrs, d_chi, n))
    finally:
        for p in ptrs + [d_chi]:
            mock.free(p)


def check(dev, mock, tables, point, field, want=None):
    got = dev.tables_mle(tables, point)
    want = reference(mock, tables, point, field) if want is None else want
    assert np.array_equal(got, want), "lasso_tables_mle differs from the reference"
    assert all(v < FR_P for v in M.word_ints(got)), "a result is not fully reduced"
    return got


# ---- kernel against reference

@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
@pytest.mark.parametrize("log_m", M.LOG_MS)
def test_against_reference(dev, mock, log_m, field):
    rng = np.random.default_rng(100 * log_m + field)
    n = 1 << log_m
    k = 3 if log_m <= 13 else 2 if log_m <= 17 else 1
    tables = [rand_fr_table(rng, n) if field else rand_u32(rng, n) for _ in range(k)]
    check(dev, mock, tables, rand_point(rng, log_m), field)


@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
@pytest.mark.parametrize("num_tables", [1, 2, 3, 31, 32])
def test_table_counts(dev, mock, num_tables, field):
    rng = np.random.default_rng(7 * num_tables + field)
    log_m = 8
    tables = [rand_fr_table(rng, 1 << log_m) if field else rand_u32(rng, 1 << log_m) for _ in range(num_tables)]
    got = check(dev, mock, tables, rand_point(rng, log_m), field)
    assert len({tuple(r) for r in got.tolist()}) == num_tables            # no two tables share a slot


# ---- table patterns

@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
@pytest.mark.parametrize("log_m", [1, 2, 3, 5, 9, 12])
def test_unit_tables_give_chi(dev, log_m, field):
    """T = e_i: the result is chi_i — pins the bit order (point[0] <-> the top bit) and the hi / lo split"""
    rng = np.random.default_rng(log_m)
    m, lo = 1 << log_m, 1 << (log_m - (log_m + 1) // 2)
    point = rand_point(rng, log_m)
    chi = M.chi_int(point, FR_P)
    idx = sorted({0, 1, lo - 1, lo % m, m - 1})
    tables = []
    for i in idx:
        t = np.zeros((m, 4), dtype=np.uint64) if field else np.zeros(m, dtype=np.uint32)
        if field:
            t[i] = words([ONE])[0]
        else:
            t[i] = 1
        tables.append(t)
    got = dev.tables_mle(tables, point)
    assert M.word_ints(got) == [chi[i] * M.R % FR_P for i in idx]


@pytest.mark.parametrize("log_m", [9] + M.FOLD_LOG_MS)
def test_constant_and_lazily_reduced_tables(dev, mock, log_m):
    """all zero, all 0xFFFFFFFF, all p - 1 and its largest representative, random lazily reduced entries.  At mleutil.FOLD_LOG_MS every lane walks 64 rows of
    these maximal entries: four carry passes of the u32 sum, twenty-one of the Fr sum"""
    rng = np.random.default_rng(40 + log_m)
    n = 1 << log_m
    point = rand_point(rng, log_m)
    u = [np.zeros(n, dtype=np.uint32), np.full(n, 0xFFFFFFFF, dtype=np.uint32), rand_u32(rng, n)]
    got = check(dev, mock, u, point, False)
    assert not got[0].any()
    assert M.word_ints(got[1:2]) == [0xFFFFFFFF * M.R % FR_P]                              # sum chi = 1: a constant table evaluates to the constant
    pm1 = np.tile(words([FR_P - 1]), (n, 1))
    rnd = rand_fr_table(rng, n)
    f = [np.zeros((n, 4), dtype=np.uint64), pm1, lift(pm1), rnd, lift(rnd), lift(rnd, rng=rng)]
    assert max(M.word_ints(f[2][:1])) >= LAZY_BOUND - FR_P
    got = check(dev, mock, f, point, True)
    assert not got[0].any() and np.array_equal(got[1], got[2]) and np.array_equal(got[3], got[4]) and np.array_equal(got[3], got[5])
    assert M.word_ints(got[1:2]) == [FR_P - 1]                                              # memory word p - 1 = the field element (p - 1) / R, times sum chi = 1


# ---- points

@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
@pytest.mark.parametrize("log_m", [2, 9, 13])
def test_boolean_points_read_the_table(dev, log_m, field):
    rng = np.random.default_rng(60 + log_m)
    n = 1 << log_m
    tables = [rand_fr_table(rng, n) if field else rand_u32(rng, n) for _ in range(2)]
    for index in sorted({0, n - 1, 0b1011001110001 & (n - 1), 1, n >> 1, (n >> 1) - 1}):
        point = words([ONE if (index >> (log_m - 1 - j)) & 1 else 0 for j in range(log_m)])
        got = dev.tables_mle(tables, point)
        want = [t[index] for t in tables] if field else [words([int(t[index]) * M.R % FR_P])[0] for t in tables]
        assert np.array_equal(got, np.array(want, dtype=np.uint64)), index


@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
def test_edge_and_lazily_reduced_coordinates(dev, mock, field):
    rng = np.random.default_rng(70 + field)
    log_m = 9
    tables = [rand_fr_table(rng, 1 << log_m) if field else rand_u32(rng, 1 << log_m) for _ in range(2)]
    point = rand_point(rng, log_m)
    point[0] = words([(FR_P - 1) * M.R % FR_P])[0]         # the field element p - 1 in the row factor ...
    point[log_m - 1] = words([FR_P - 1])[0]                # ... and the memory word p - 1 in the column factor
    point[3] = words([0])[0]; point[6] = words([ONE])[0]
    got = check(dev, mock, tables, point, field)
    assert np.array_equal(dev.tables_mle(tables, lift(point)), got)                  # every coordinate's largest representative below 2^254 + 2^130
    assert np.array_equal(dev.tables_mle(tables, lift(point, rng=rng)), got)


# ---- strips

@pytest.mark.parametrize("field", [False, True], ids=["u32", "fr"])
def test_strips_with_a_ragged_last_one(dev, mock, field, monkeypatch):
    rng = np.random.default_rng(80 + field)
    log_m = 10
    tables = [rand_fr_table(rng, 1 << log_m) if field else rand_u32(rng, 1 << log_m) for _ in range(3)]
    point = rand_point(rng, log_m)
    whole = check(dev, mock, tables, point, field)
    for strip in (M.STRIP_TEST_LEN, 32, 1 << 10, 1 << 12, 1000):     # three strips and a ragged one; whole rows; exactly the table; longer than the table; a 24-entry tail
        monkeypatch.setenv("LASSO_MLE_STRIP", str(strip))
        assert np.array_equal(dev.tables_mle(tables, point), whole), strip
    monkeypatch.delenv("LASSO_MLE_STRIP")
    assert np.array_equal(dev.tables_mle(tables, point), whole)


# ---- the _dev form, under the scratch guard, in a child process (LASSO_SCRATCH_GUARD is read once per process)

_DEV_CHILD = r"""
import json, os, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from fieldref import CURVE
from gpuutil import full_fr
from lasso_amd import Device
d = Device(0, curve=CURVE)
out = []
for log_m, field, k in ((10, False, 3), (10, True, 3), (16, False, 2), (16, True, 2), (1, True, 1), (5, False, 32)):
    rng = np.random.default_rng(log_m + field)
    n = 1 << log_m
    tables = [full_fr(rng, n) if field else rng.integers(0, 2**32, size=n, dtype=np.uint64).astype(np.uint32) for _ in range(k)]
    point = full_fr(rng, log_m)
    host = d.tables_mle(tables, point)
    os.environ["LASSO_MLE_STRIP"] = "300"
    strips = d.tables_mle(tables, point)
    del os.environ["LASSO_MLE_STRIP"]
    ptrs = [d.upload(t) for t in tables]
    res = d.tables_mle_dev(ptrs, point, field)
    d.sync()                                                        # LASSO_SCRATCH_GUARD: raises when a launch wrote behind the scratch it asked for
    same = all(np.array_equal(d.download(p, t.shape, t.dtype), t) for p, t in zip(ptrs, tables))
    for p in ptrs:
        d.free(p)
    out.append({"log_m": log_m, "field": field, "equal": bool(np.array_equal(res, host) and np.array_equal(strips, host)), "tables_unchanged": bool(same), "sync": d.lib.lasso_sync(d.ctx)})
print(json.dumps(out))
d.close()
"""


def test_dev_form_equals_host_form_and_leaves_the_tables_alone():
    env = dict(os.environ, LASSO_SCRATCH_GUARD="1")
    env.pop("LASSO_MLE_STRIP", None)
    res = subprocess.run([sys.executable, "-c", _DEV_CHILD, ROOT], env=env, cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    rows = json.loads(res.stdout.strip().split("\n")[-1])
    assert len(rows) == 6
    for r in rows:
        assert r["equal"] and r["tables_unchanged"] and r["sync"] == 0, r


def test_scratch_is_counted_and_bounded(dev):
    """the host form's scratch comes from the context's pool (lasso_mem_stats) and stays under the header's bound at a size whose tables exceed it"""
    live, peak = C.c_uint64(), C.c_uint64()
    rng = np.random.default_rng(5)
    log_m = 22                                                       # 32 tables x 16 MiB = 512 MiB of u32 tables
    one = rng.integers(0, 2**32, size=1 << log_m, dtype=np.uint64).astype(np.uint32)
    tables = [one] * 32
    point = rand_point(rng, log_m)
    assert dev.lib.lasso_mem_stats(dev.ctx, C.byref(live), C.byref(peak), 1) == 0
    before = live.value
    got = dev.tables_mle(tables, point)
    assert dev.lib.lasso_mem_stats(dev.ctx, C.byref(live), C.byref(peak), 0) == 0
    assert before < live.value or live.value >= 64 << 20, "no scratch was accounted to the context"
    assert peak.value - before <= (69 << 20) + (64 << 10), (peak.value, before)
    assert all(np.array_equal(got[0], g) for g in got[1:])
    assert np.array_equal(dev.tables_mle([one], point), got[:1])


# ---- invalid arguments

def test_invalid_arguments_are_refused_before_any_launch(dev):
    from lasso_amd import _abi
    _abi.declare_mle(dev.lib)
    rng = np.random.default_rng(9)
    t = rand_u32(rng, 16); f = rand_fr_table(rng, 16); point = rand_point(rng, 4)
    good = dev.tables_mle([t], point)
    pt = (C.c_void_p * 33)(*([t.ctypes.data] * 33)); pf = (C.c_void_p * 33)(*([f.ctypes.data] * 33))
    pp = point.ctypes.data_as(C.c_void_p)
    launches = lambda: sum(dev.prof_get(k)[0] for k in range(_abi.K_COUNT))
    dev.prof_reset(); dev.prof_enable((1 << _abi.K_COUNT) - 1)
    try:
        for fn in (dev.lib.lasso_tables_mle, dev.lib.lasso_tables_mle_dev):
            for tu, tf, k, log_m in ((pt, pf, 1, 4), (None, None, 1, 4), (pt, None, 0, 4), (pt, None, 33, 4), (None, pf, 33, 4), (pt, None, 1, 0), (pt, None, 1, 31), (None, pf, 1, 31)):
                out = np.zeros((33, 4), dtype=np.uint64)
                assert fn(dev.ctx, tu, tf, k, log_m, pp, out.ctypes.data_as(C.c_void_p)) == -1           # LASSO_ERR_INVALID
                assert dev.lib.lasso_last_error(dev.ctx).decode().startswith("invalid argument")
                assert not out.any()
            hole = (C.c_void_p * 2)(t.ctypes.data, None)
            assert fn(dev.ctx, hole, None, 2, 4, pp, np.zeros((2, 4), dtype=np.uint64).ctypes.data_as(C.c_void_p)) == -1
            assert fn(dev.ctx, pt, None, 1, 4, None, np.zeros((1, 4), dtype=np.uint64).ctypes.data_as(C.c_void_p)) == -1
            assert fn(dev.ctx, pt, None, 1, 4, pp, None) == -1
        assert launches() == 0, "a refused call launched something"
        assert np.array_equal(dev.tables_mle([t], point), good) and launches() > 0                        # the context is usable, and the counter does count
    finally:
        dev.prof_enable(0)


# ---- the verifier

# log_m = 8 and 16, integer and field-element tables; built-in strategies as descriptors, so that the oracle's verifier can judge the same bytes
VERIFY_SPECS = [{"make": "builtin", "args": ["lt", 2, 8, 0]}, {"make": "builtin", "args": ["spark", 2, 8, 0]}, {"make": "builtin", "args": ["and", 1, 16, 0]},
                {"make": "builtin", "args": ["spark", 1, 16, 0]}]


def test_verifier_device_route_host_route_and_oracle_agree():
    import conftest
    from lasso_amd import _abi
    from proverutil import OracleSession
    lookups = 1 << 10
    import types
    devs = M.verify_in_child("", CURVE, VERIFY_SPECS, lookups, {"LASSO_MLE_DEVICE_MIN": "0"}, timeout=600, few=True)
    hosts = M.verify_in_child("", CURVE, VERIFY_SPECS, lookups, {"LASSO_MLE_DEVICE_MIN": "0", "LASSO_VERIFY_DEVICE_MLE": "0"}, timeout=600, few=True)
    oracle = conftest._load_oracle(conftest._build_oracle_bn254() if CURVE == "bn254" else conftest._build_oracle())
    for spec, dev, host in zip(VERIFY_SPECS, devs, hosts):
        assert dev["available"] and dev["proof"] == host["proof"] and dev["comm"] == host["comm"]
        for a, b in zip(dev["results"], host["results"]):
            assert a["name"] == b["name"] and a["verdict"] == b["verdict"], (spec, a, b)
            assert b["device_tables"] == 0 and a["device_tables"] in (0, dev["distinct"])
        assert dev["results"][0] == {"name": "honest", "verdict": True, "device_tables": dev["distinct"]}                    # mle_stats: the device route ran ...
        assert dev["results"][-1] == {"name": "one table entry changed", "verdict": False, "device_tables": dev["distinct"]}  # ... and it is what rejects a changed table
        assert all(r["verdict"] is not True for r in dev["results"][1:])
        kind, c, log_m, log_r = spec["args"]
        cs = types.SimpleNamespace(c=c, log_m=log_m, num_memories=2 * c if kind == "lt" else c)          # what child_indices and tampered read of a strategy
        r = np.array(dev["r"], dtype=np.uint64)
        o = OracleSession(oracle, _abi.KINDS[kind], c, log_m, log_r, M.child_indices(cs, lookups), r)
        try:
            proof, comm = bytes.fromhex(dev["proof"]), bytes.fromhex(dev["comm"])
            assert proof == o.prove() and comm == o.commit(), "the descriptor's proof is not the oracle's proof of the built-in"
            variants = [("honest", proof, comm)] + M.tampered(proof, comm, cs, few=True)
            verdicts = {x["name"]: x["verdict"] for x in dev["results"]}
            assert len(variants) >= 4 and all(name in verdicts for name, _, _ in variants)
            for name, p, cm in variants:
                assert (o.verify(p, cm) == 1) == (verdicts[name] is True), (spec, name)
        finally:
            o.close()


def test_gpu_bn254_mle():
    """this module again on the BN254 build, in a child process (tests/fieldref.py reads LASSO_TEST_CURVE at import)"""
    if CURVE == "bn254":
        return
    env = dict(os.environ, LASSO_TEST_CURVE="bn254")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", "not test_gpu_bn254_mle"],
                         cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout
