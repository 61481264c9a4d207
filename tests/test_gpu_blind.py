"""-m gpu: hiding commitments (include/lasso_prover_blind.h) on the product libraries of both curves.  All comparisons are exact; every child runs under LASSO_POISON=1
and LASSO_SCRATCH_GUARD=1 (tests/blindutil.py GPU_CHILD).

  bytes       num_vars = 1 (one row), 5 (4 rows of 8) and 11 (32 rows of 64: the smallest that takes the multi-row MSM kernels) x field form, 64-bit form below 2^32,
              64-bit form with bit 63 set x host and device residence: commitment, returned blinds, opening, Zr and C_Zr equal the mock build's on the same tape (which
              tests/test_blind_cpu.py holds to the oracle's); a merge of 3 vectors of 2^5 values, mixed forms and residence, likewise
  verdicts    the product verifier accepts the committed form and, under a non-zero blind_Zr, refuses the plain one; a flipped bit in C_Zr, in the proof, in a row and one
              changed blind are each rejected
  routes      field-form rows are blinded on the device (lasso_hyrax_commit_rows_dev twice, lasso_points_reduce_compress), 64-bit rows through the decode route with
              the 8-byte entries counted by poly_stats; a second child under LASSO_WIRE_DEVICE_MIN=1 reaches the device decoder at 32 rows and below
After a child that did not end normally nothing more is started on the GPU by this module."""
import json
import os
import subprocess
import sys

import pytest

import blindutil as B
import polyutil as P

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
_dead = []
GUARDED = {"LASSO_POISON": "1", "LASSO_SCRATCH_GUARD": "1"}
ROWS = sum(1 << (nv // 2) for nv in B.GPU_NUM_VARS)          # rows of one pass over the shapes


def _child(args, env_extra, timeout):
    if _dead:
        pytest.fail("not started: an earlier child of this module did not end normally (" + _dead[0] + ")")
    env = dict(os.environ)
    for k in ("LASSO_POISON", "LASSO_SCRATCH_GUARD", "LASSO_WIRE_DEVICE_MIN", "LASSO_VERIFY_DEVICE_POINTS"):
        env.pop(k, None)
    env.update(env_extra)
    try:
        res = subprocess.run([sys.executable, "-c", B.GPU_CHILD, ROOT] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        _dead.append("time limit: " + " ".join(args))
        raise
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
        _dead.append(f"exit status {res.returncode}: " + " ".join(args))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])


@pytest.mark.parametrize("curve", B.CURVES)
@pytest.mark.parametrize("decoder", ["default", "device"])
def test_bytes_verdicts_and_routes(curve, decoder):
    B.build(curve, "poly")          # compiled before the child's time limit starts
    env = dict(GUARDED, **({"LASSO_WIRE_DEVICE_MIN": "1"} if decoder == "device" else {}))
    out = _child([curve], env, timeout=240)
    assert out["failures"] == []
    assert out["cases"] == len(B.GPU_NUM_VARS) * len(B.FORMS) * 2 + 1
    # field form: host and device residence, all on the device; the two 64-bit forms: both residences through the decode route
    assert out["routes"]["rows_device"] == 2 * ROWS and out["routes"]["rows_host"] == 4 * ROWS
    # the decode route's decoder: the host's below the default threshold (376 points), the device's from one point on
    assert out["routes"]["wire"] == (4 * ROWS if decoder == "device" else 0)
