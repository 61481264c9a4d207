"""-m gpu: every row of tests/msmvariants.py TABLE on the device, against the oracle's mock, byte for byte.

The runtime switches that select an MSM kernel are read once per process, so tests/test_gpu_kernels.py only ever runs the defaults, and the proof-level switch test
(tests/test_gpu_prover.py::test_gpu_ab_switches_do_not_change_the_bytes) proves shapes that never reach most of the switched kernels.  Here each switch setting gets ONE child
process that runs the setting's rows at the shapes tests/test_msm_reach_cpu.py has shown to reach the kernel: k_msm_rows_full<8> (LASSO_MSM_FULL8=1: signed-byte recoding, LDS
batches of 128 columns, chunked rows, ragged last batch), k_msm_rows8w with rpw > 1 (LASSO_MSM_ROWS8W_WAVES), k_msm_rows8 at >= 1024 rows (LASSO_MSM_ROWS8W=0), the bucket
kernel in place of each of them, k_msm_direct / k_bullet_msm over both multiple tables at every chunking LASSO_MSM_DIRECT_WGS gives, the 12-bit-window kernels in one group and
several, wire bytes by hipMemcpy (more than 2^16 rows) and row sums left on the device; and slab mode (lasso_bullet_round_slab, lasso_msm_dev_slab: world > 1), every rank of
each shape, under the default switches, both multiple tables and the chunkings LASSO_MSM_DIRECT_WGS gives (tests/test_gpu_kernels.py holds the ranks' results, put together
again, to the single-rank calls).

The expected bytes come from the mock Device, once per module: they do not depend on the setting, which is the point.  Runs on the build LASSO_TEST_CURVE selects
(tests/test_gpu_bn254.py re-runs the module on the BN254 build)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import msmvariants as V
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
    yield mock.lib, out
    mock.close()


def run_child(index, timeout):
    """the rows of ENVS[index] on the device, in a fresh process with that environment -> {row id: {name: bytes}}"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("LASSO_MSM_")}
    env.update(V.ENVS[index])
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "msmvariants.py"), str(index)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the child of {V.env_id(V.ENVS[index])} did not finish in {timeout} s\n{err[-2000:]}")
    assert res.returncode == 0, f"the child of {V.env_id(V.ENVS[index])} ended with {res.returncode}\n{res.stderr[-3000:]}"
    got = {}
    for ln in res.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "ROW":
            got.setdefault(f[1], {})[f[2]] = bytes.fromhex(f[3])
    assert f"DONE {len(V.rows_of(V.ENVS[index]))}" in res.stdout.splitlines()[-1:], res.stdout[-500:] + res.stderr[-2000:]
    return got


@pytest.mark.parametrize("index", range(len(V.ENVS)), ids=[V.env_id(e) for e in V.ENVS])
def test_every_row_of_the_setting_gives_the_mocks_bytes(expected, index):
    mock_lib, want = expected
    got = run_child(index, timeout=240)
    rows = V.rows_of(V.ENVS[index])
    assert set(got) == {r.id for r in rows}
    bad = []
    for r in rows:
        out = V.as_wire(mock_lib, {name: np.frombuffer(raw, dtype=V.dtype_of(name)) for name, raw in got[r.id].items()})
        assert set(out) == set(want[r.id]), r.id
        for name, w in want[r.id].items():
            g = out[name].reshape(w.shape)
            if not np.array_equal(g, w):
                where = np.flatnonzero(np.any((g != w).reshape(w.shape[0], -1), axis=1))
                bad.append(f"{r.id} ({r.entry} {tuple(r.shape)}, expected plan {r.expect}): `{name}` differs from the mock's in {len(where)} of {w.shape[0]} rows, first at {where[:8].tolist()}")
    assert not bad, "\n".join(bad)
