"""-m gpu: the three entries of include/lasso_hip_poly.h on the real libraries of both curves, and the chain commit(values) -> open at r -> the Lasso proof's claim end to
end on the product libraries.  All comparisons are exact.

  matvec      lasso_matvec_left_u64_dev against Python integers and, byte for byte, lasso_matvec_left_dev of the lifted array (tests/polyutil.py MATVEC_CHILD, under
              LASSO_POISON=1 and LASSO_SCRATCH_GUARD=1): odd and even r_size, the half-filled last lane pair, one and several row chunks, 33 rows per chunk (two carry
              passes); all 0, all 2^64 - 1, random 64-bit, random 8-bit; d_out is followed by a pattern that must survive; lasso_u64_or in the same child
  commit      lasso_hyrax_commit_compressed_u64 against lasso_hyrax_commit_compressed of the lifted array and the oracle's MSM rows (COMMIT_CHILD): rows 1 / 3 / 32 / 33,
              columns 1 / 2 / 255 / 512, bounds of 1 .. 64 bits on both sides of the 2^32 boundary, all-zero rows, all-equal scalars, every scalar 2^64 - 1
  end to end  2^10 lookups: AND C=1 (4-byte route), XOR C=8 at log_m 16 (8-byte route), LT C=2, Spark C=2 (field form); the vector never leaves the device; commitment and
              opening bytes equal the wrapped-mock prover library's; capacity mode once
After a child that did not end normally nothing more is started on the GPU by this module."""
import ctypes as C
import json
import os
import subprocess
import sys

import pytest

import polyutil as P

pytestmark = pytest.mark.gpu
ROOT = P.ROOT
CURVES = P.CURVES
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
@pytest.mark.parametrize("group", ["small", "large"])
def test_matvec_left_u64_against_python_integers_and_the_lifted_array(group, curve):
    out = _child(P.MATVEC_CHILD, [curve, group], GUARDED, timeout=240)
    print(group, curve, out["cases"], "cases")
    assert out["failures"] == []
    assert out["cases"] == (7 * 4 + 3 * len(P.OR_NS) if group == "small" else 2 * 4)


@pytest.mark.parametrize("curve", CURVES)
def test_commit_u64_against_the_lifted_array_and_the_oracle(curve):
    out = _child(P.COMMIT_CHILD, [curve], GUARDED, timeout=300)
    print(curve, out["cases"], "cases")
    assert out["failures"] == []
    assert out["cases"] == len(P.COMMIT_ROWS) * len(P.COMMIT_COLS) * (len(P.COMMIT_WIDTHS) + 6)
    assert out["routes"] == ["narrow", "wide"]


# argv: root, curve, capacity ("1" / "0"), JSON list of [kind, c, log_m, log_r, expect_u64].  The end-to-end story of tests/polyutil.py end_to_end on the product library,
# with the wrapped-mock prover library of the same curve loaded beside it for the byte comparison.
E2E_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd.prover import HostProver
import polyutil as P
curve, capacity, cases = sys.argv[2], sys.argv[3] == "1", json.loads(sys.argv[4])
hp = HostProver(curve=curve)
if capacity:
    hp.set_capacity(True)
mock = HostProver(C.CDLL(P.build_mock_prover_poly(curve)), curve=curve)
assert hp.poly_stats()["available"] is True
done = []
for kind, c, log_m, log_r, expect_u64 in cases:
    P.end_to_end(hp, curve, kind, c, log_m, log_r, lookups=1000, expect_u64=expect_u64, mock=mock)
    done.append(kind)
print(json.dumps({"done": done, "stats": hp.poly_stats()}))
mock.close(); hp.close()
"""

E2E_CASES = [["and", 1, 16, 0, True], ["xor", 8, 16, 0, True], ["lt", 2, 8, 0, True], ["spark", 2, 8, 0, False]]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("case", E2E_CASES, ids=[c[0] for c in E2E_CASES])
def test_end_to_end_on_the_product_library(case, curve):
    P.build_mock_prover_poly(curve)          # compiled before the child's time limit starts
    out = _child(E2E_CHILD, [curve, "0", json.dumps([case])], GUARDED, timeout=300)
    assert out["done"] == [case[0]]
    if case[4]:
        assert out["stats"]["u64_commit_elements"] >= 1024 and out["stats"]["u64_open_elements"] >= 2048


def test_end_to_end_in_capacity_mode():
    P.build_mock_prover_poly("curve25519")
    out = _child(E2E_CHILD, ["curve25519", "1", json.dumps([E2E_CASES[0], E2E_CASES[2]])], {"LASSO_LEAFLESS_MIN": "64"}, timeout=300)
    assert out["done"] == ["and", "lt"]
