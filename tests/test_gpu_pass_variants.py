"""-m gpu: every row of tests/passvariants.py TABLE on the device, against the oracle's mock, byte for byte.

The kernels that sum field products keep lazily reduced running sums and fold them at a fixed period, counted in passes of a thread's grid-stride loop: a carry pass after every
3rd product, fr29_mul(acc, one_s) every 128 or 64 additions, every LT_FOLD_EVERY() = 32 indices.  At the shapes of tests/test_gpu_kernels.py a thread makes one pass (the cubic
rows of tests/roundvariants.py: 2 to 8), so the fold and the accumulation behind it never ran in the compiled device code.  Here each switch setting gets ONE child process that
runs the setting's rows at the shapes tests/test_pass_reach_cpu.py has shown to reach the fold: under LASSO_CUBIC_NX=3 and LASSO_REDUCE_NX=3 three workgroups share a launch, so
arrays of 2^13 .. 2^19 elements give a thread 5 to 171 passes; under the default switches the second stage sums 512 and 1024 partials per row and the mat-vec's row chunks reach
their carries and k_matvec_reduce's fold.  Every row runs on uniform elements and on the data that maximises what a running sum holds between two folds.

The expected bytes come from the mock Device, once per module: they do not depend on the setting.  The mock is exact canonical arithmetic: the criterion is equality, and it
is given the canonical representatives of the residues the device gets as lazily reduced ones (passvariants.run_row says why).  Arrays a round has bound are compared as
residues (the device keeps lazily reduced representatives); arrays above 4 KiB by their SHA-256.  Runs on the build LASSO_TEST_CURVE selects
(tests/test_gpu_bn254.py re-runs the module on the BN254 build)."""
import os
import subprocess
import sys
import time

import pytest

import passvariants as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def expected():
    """{row id: {name: text}} from the oracle's mock; rows of the same call, shape and data share one run"""
    from lasso_amd import Device
    t0 = time.perf_counter()
    mocks, by_key, out = {}, {}, {}
    for row in V.TABLE:
        key = V.reference_key(row)
        if key not in by_key:
            lib = V.mock_for(row)
            if id(lib) not in mocks:
                mocks[id(lib)] = Device(0, lib=lib)
            by_key[key] = V.printable(V.run_row(mocks[id(lib)], row, reduced=True))
        out[row.id] = by_key[key]
    print(f"\n[pass variants] the mock's {len(by_key)} runs: {time.perf_counter() - t0:.1f} s")
    yield out
    for m in mocks.values():
        m.close()


def run_child(index, timeout):
    """the rows of ENVS[index] on the device, in a fresh process with that environment -> {row id: {name: text}}"""
    env = {k: v for k, v in os.environ.items() if k not in V.SWITCHES}
    env.update(V.ENVS[index])
    t0 = time.perf_counter()
    try:
        res = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "passvariants.py"), str(index)], cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        err = e.stderr.decode(errors="replace") if isinstance(e.stderr, bytes) else (e.stderr or "")
        pytest.fail(f"the child of {V.env_id(V.ENVS[index])} did not finish in {timeout} s\n{err[-2000:]}")
    print(f"\n[pass variants] {V.env_id(V.ENVS[index])}: {len(V.rows_of(V.ENVS[index]))} rows, child {time.perf_counter() - t0:.1f} s")
    assert res.returncode == 0, f"the child of {V.env_id(V.ENVS[index])} ended with {res.returncode}\n{res.stdout[-300:]}\n{res.stderr[-3000:]}"
    got = {}
    for ln in res.stdout.splitlines():
        f = ln.split(" ")
        if f[0] == "ROW":
            got.setdefault(f[1], {})[f[2]] = f[3]
    assert f"DONE {len(V.rows_of(V.ENVS[index]))}" in res.stdout.splitlines()[-1:], res.stdout[-500:] + res.stderr[-2000:]
    return got


def first_difference(g, w):
    """where two outputs printed as hex first differ, in field elements; a digest says only that they do"""
    if g.startswith("sha256:") or len(g) != len(w):
        return "the arrays' digests differ"
    return f"first at element {next(i for i in range(0, len(w), 64) if g[i:i + 64] != w[i:i + 64]) // 64}"


@pytest.mark.parametrize("index", range(len(V.ENVS)), ids=[V.env_id(e) for e in V.ENVS])
def test_every_row_of_the_setting_gives_the_mocks_bytes(expected, index):
    got = run_child(index, timeout=180)
    rows = V.rows_of(V.ENVS[index])
    assert set(got) == {r.id for r in rows}
    bad = []
    for r in rows:
        want = expected[r.id]
        assert set(got[r.id]) == set(want), r.id
        for name, w in want.items():
            if got[r.id][name] != w:
                bad.append(f"{r.id} ({r.kernel}, period {r.period}, claim `{r.claim}`): `{name}` differs from the mock's, {first_difference(got[r.id][name], w)}")
    assert not bad, "\n".join(bad)
