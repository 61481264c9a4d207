"""-m gpu: every row of tests/roundvariants.py TABLE on the device, against the oracle's mock, byte for byte.

The runtime switches that select a cubic-round kernel are read once per process, so tests/test_gpu_kernels.py only ever runs the defaults (and LASSO_EQ_INLINE_BIG=1 in a child of
its own), and the proof-level switch test (tests/test_gpu_prover.py::test_gpu_ab_switches_do_not_change_the_bytes) proves one instance whose launches need not reach the kernel a
setting is about: with the layer's eq table built inside round 0, no proof starts a layer with the plain table-reading round LASSO_LB_NT=1 changes.  Here each switch setting gets
ONE child process that runs the setting's rows at the shapes tests/test_round_reach_cpu.py has shown to reach the instantiation: k_cubic_eqw_small<BIND, NT>, k_cubic_eqw_fused
with three sums, two wide and two narrow (LASSO_CUBIC_WIDE=0), launched ahead with the wait behind k_gate or inside the kernel on both sides of LASSO_AHEAD_INKERNEL_WGS,
k_cubic_eqw_lb over EqNone (pipelined, plain under LASSO_LB_PIPELINE=0, non-temporal under LASSO_LB_NT=1), EqInline, EqInlineMem and EqGlobal (LASSO_EQ_INLINE_BIG=1), behind
k_eq_small2 / k_eq_small2_mem and k_eq_outer, block sums direct or through the second stage (LASSO_DIRECT_NX, LASSO_TAGGED_RESULTS=0), grids at their cap and at an x-extent that
is no power of two (LASSO_CUBIC_NX), both pointer tables.

The expected bytes come from the mock Device, once per module: they do not depend on the setting, which is the point.  Arrays a round has bound are compared as residues (the
device keeps lazily reduced representatives).  Runs on the build LASSO_TEST_CURVE selects (tests/test_gpu_bn254.py re-runs the module on the BN254 build)."""
import os
import subprocess
import sys
import time

import numpy as np
import pytest

import roundvariants as V
from gpuutil import load_mock

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def expected():
    """{row id: {name: array}} from the oracle's mock; rows of the same call and shape share one run"""
    from lasso_amd import Device
    mock = Device(0, lib=load_mock())
    by_key, out = {}, {}
    for row in V.TABLE:
        key = V.reference_key(row)
        if key not in by_key:
            by_key[key] = V.reference(mock, row)
        out[row.id] = by_key[key]
    yield out
    mock.close()


def run_child(index, timeout):
    """the rows of ENVS[index] on the device, in a fresh process with that environment -> {row id: {name: bytes}}"""
    env = {k: v for k, v in os.environ.items() if k not in V.SWITCHES}
    env.update(V.ENVS[index])
    t0 = time.perf_counter()
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "roundvariants.py"), str(index)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the child of {V.env_id(V.ENVS[index])} did not finish in {timeout} s\n{err[-2000:]}")
    print(f"\n[round variants] {V.env_id(V.ENVS[index])}: {len(V.rows_of(V.ENVS[index]))} rows, child {time.perf_counter() - t0:.1f} s")
    assert res.returncode == 0, f"the child of {V.env_id(V.ENVS[index])} ended with {res.returncode}\n{res.stdout[-300:]}\n{res.stderr[-3000:]}"
    got = {}
    for ln in res.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "ROW":
            got.setdefault(f[1], {})[f[2]] = bytes.fromhex(f[3])
    assert f"DONE {len(V.rows_of(V.ENVS[index]))}" in res.stdout.splitlines()[-1:], res.stdout[-500:] + res.stderr[-2000:]
    return got


def first_difference(name, g, w, ncirc):
    """where `name` first differs, in the row's own terms"""
    idx = int(np.flatnonzero(np.any((g != w).reshape(-1, 4), axis=1))[0])
    if name in V.LAZY:
        per = w.shape[1]
        return f"circuit {idx // per}, index {idx % per}"
    if name == "sums":
        per = w.shape[0] // ncirc
        return f"circuit {idx // per}, sum {idx % per}"
    return f"index {idx}"


@pytest.mark.parametrize("index", range(len(V.ENVS)), ids=[V.env_id(e) for e in V.ENVS])
def test_every_row_of_the_setting_gives_the_mocks_bytes(expected, index):
    got = run_child(index, timeout=120)
    rows = V.rows_of(V.ENVS[index])
    assert set(got) == {r.id for r in rows}
    bad = []
    for r in rows:
        want = expected[r.id]
        assert set(got[r.id]) == set(want), r.id
        out = V.comparable({name: np.frombuffer(raw, dtype=V.DTYPES[name]).reshape(want[name].shape) for name, raw in got[r.id].items()})
        for name, w in want.items():
            if not np.array_equal(out[name], w):
                what = f"{out[name].tolist()} against {w.tolist()}" if name == "rc" else f"first at {first_difference(name, out[name], w, r.shape.ncirc)}"
                bad.append(f"{r.id} ({r.entry} {tuple(r.shape)}, expected plan {r.expect}): `{name}` differs from the mock's, {what}")
    assert not bad, "\n".join(bad)
