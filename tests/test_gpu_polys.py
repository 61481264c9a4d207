"""-m gpu: several caller vectors under one commitment, opened at r in one proof (include/lasso_prover_polys.h) on the product libraries of both curves.  All
comparisons are exact; every child runs under LASSO_POISON=1 and LASSO_SCRATCH_GUARD=1.

  shapes      (nv, k) = (1, 2) one row of two columns per vector, (2, 3) one row per vector and one identity row, (3, 2), (5, 5), (9, 3) an odd joint variable count
              (left 5, right 6), (12, 2) 32 rows per vector (tests/polysutil.py SHAPES_CHILD): mixed forms, device-resident vectors (lasso_alloc; as DeviceVector and
              as a bare (pointer, form) pair) beside host vectors in one call; commitment and opening bytes equal the wrapped-mock prover library's, evals equal Python
              integers and polys_evaluate, the opening verifies; poly_stats' 64-bit counters grow by s per 64-bit vector: the 8-byte device entries ran
  end to end  2^10 lookups at log_m = 16, (x, y, v_first, v_second) under one commitment, the result vectors never leaving the device: AND C=1 with LT C=2 over the same
              operands; XOR C=8 (64-bit results of full width) with Spark C=2 (field form)
After a child that did not end normally nothing more is started on the GPU by this module."""
import json
import os
import subprocess
import sys

import pytest

import polysutil as S
import polyutil as P

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
CURVES = S.CURVES
_dead = []


def _child(script, args, env_extra, timeout):
    if _dead:
        pytest.fail("not started: an earlier child of this module did not end normally (" + _dead[0] + ")")
    env = dict(os.environ)
    for k in ("LASSO_POISON", "LASSO_SCRATCH_GUARD", "LASSO_LEAFLESS_MIN", "LASSO_CAPACITY_COMPACT"):
        env.pop(k, None)
    env.update(env_extra)
    try:
        res = subprocess.run([sys.executable, "-c", script, ROOT] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        _dead.append("time limit: " + " ".join(args))
        raise
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
        _dead.append(f"exit status {res.returncode}: " + " ".join(args))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])


GUARDED = {"LASSO_POISON": "1", "LASSO_SCRATCH_GUARD": "1"}


@pytest.mark.parametrize("curve", CURVES)
def test_shapes_against_the_mock_and_python_integers(curve):
    P.build_mock_prover_poly(curve)          # compiled before the child's time limit starts
    out = _child(S.SHAPES_CHILD, [curve, json.dumps(S.GPU_SHAPES)], GUARDED, timeout=240)
    assert out["failures"] == []
    assert out["done"] == [list(x) for x in S.GPU_SHAPES]


E2E_CASES = [[["and", 1], ["lt", 2], 16, 1000, 8], [["xor", 8], ["spark", 2], 16, 1000, 64]]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("case", E2E_CASES, ids=["and_lt", "xor_spark"])
def test_end_to_end_on_the_product_library(case, curve):
    P.build_mock_prover_poly(curve)
    out = _child(S.E2E_CHILD, [curve, json.dumps(case)], GUARDED, timeout=300)
    assert out["done"] is True
    assert out["stats"]["vectors_committed"] >= 8 and out["stats"]["vectors_opened"] >= 8
