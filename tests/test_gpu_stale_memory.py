"""-m gpu: proofs, verifier and set-up paths of the suite once more under LASSO_POISON=1 (lasso_amd/csrc/device_switches.cuh): every allocation the device library makes —
scratch, sort and big-result buffers, generator tables, term lists, mapped result buffers, everything the prover takes from lasso_alloc — starts as the word 0x00000001 repeated,
and the first request a public call makes of the scratch, the sort buffer or the big-result buffer fills its requested range with the word in stream order.  Nothing is asserted
here: the selected tests keep their own assertions (bytes equal to the oracle's, to the default configuration's, to the host's arithmetic), and a kernel or a prover step that
reads what its own call did not store fails them.  tests/test_gpu_write_contract.py does the same at kernel level.

One child pytest per group, smallest shapes only, each with its own time limit; a child that does not finish in it, or is ended by a signal, is the last one started (the
groups after it fail at once), and nothing is retried.  Runs on the build LASSO_TEST_CURVE selects: tests/test_gpu_bn254.py re-runs the module on the BN254 build, where the
groups are the BN254 proofs and the verifier and set-up modules (the slab, soak and switch tests of tests/test_gpu_prover.py exist for the curve25519 build only; slab proofs on the BN254 build are in tests/test_gpu_slab_switches.py).

  proofs     tests/test_gpu_prover.py: test_gpu_proof_bit_exact_vs_oracle (all CASES), test_gpu_cubic_batched_scripted_eq_points, test_gpu_soak_alternating_shapes_on_one_prover
             (240 proofs of four shapes on one prover: the pool and the scratch as another shape left them)
  slab       test_gpu_slab_proof_bit_exact over 2 and 4 ranks; tests/test_gpu_custom_strategy.py test_custom_as_builtin_in_capacity_mode (2^12 lookups)
  switches   test_gpu_ab_switches_do_not_change_the_bytes: each setting's own process inherits the fill
  setup      tests/test_gpu_wire_points.py, test_gpu_mle.py, test_gpu_gens_device.py, test_gpu_msm_points.py, test_gpu_operands.py, test_gpu_custom_strategy.py without their
             BN254 re-runs, the 2^16 and 2^17 cases, the large custom shapes and the 2^16 end-to-end strategies

Measured on an MI355X, seconds per child (tests that passed): curve25519 build — proofs 11 (39), slab 12 (14), switches 24 (48), setup 39 (266; the torch-tensor test of
tests/test_gpu_operands.py skips where torch sees no device, as it does in its own module); 86 s for the module.  BN254 build — proofs 5 (13), setup 26 (239); 31 s.  Every
limit is the write-contract module's 300 s; the longest child stays below a seventh of it.  No test failed under the fill on either build."""
import os
import re
import subprocess
import sys
import time

import pytest

import passvariants as PV
import roundvariants as RV
from fieldref import CURVE

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_T = lambda *names: [os.path.join(ROOT, "tests", n) for n in names]      # noqa: E731

_SETUP = (_T("test_gpu_wire_points.py", "test_gpu_mle.py", "test_gpu_gens_device.py", "test_gpu_msm_points.py", "test_gpu_operands.py", "test_gpu_custom_strategy.py"),
          "not test_gpu_bn254_mle and not test_gpu_bn254_operands and not 2p17 and not 2p16 and not large_shapes and not capacity_mode and not 16-lte and not 16-field")
# group -> (files, -k expression, time limit in seconds)
GROUPS = {
    "proofs": (_T("test_gpu_prover.py"), "test_gpu_proof_bit_exact_vs_oracle or test_gpu_cubic_batched_scripted_eq_points or test_gpu_soak_alternating_shapes_on_one_prover", 300),
    "slab": (_T("test_gpu_prover.py", "test_gpu_custom_strategy.py"), "(test_gpu_slab_proof_bit_exact and (-2] or -4])) or test_custom_as_builtin_in_capacity_mode", 300),
    "switches": (_T("test_gpu_prover.py"), "test_gpu_ab_switches_do_not_change_the_bytes", 300),
    "setup": _SETUP + (300,),
} if CURVE != "bn254" else {
    "proofs": (_T("test_gpu_bn254.py"), "test_gpu_bn254_proof_bit_exact_vs_oracle", 300),
    "setup": (_SETUP[0], _SETUP[1] + " and not test_custom_as_builtin and not test_new_strategies and not test_linear_custom and not test_generators_and_proof and not test_whole_path "
              "and not test_device_resident and not test_torch_tensors", 300),
}
_STOPPED = []      # why no further child is started


def run_child(group):
    """the group's tests on the device, in a fresh process under LASSO_POISON=1 -> the number of tests that passed"""
    files, select, timeout = GROUPS[group]
    env = {k: v for k, v in os.environ.items() if k not in RV.SWITCHES + PV.SWITCHES and not k.startswith("LASSO_MSM_") and k not in ("LASSO_ARENA_OVER", "LASSO_SCRATCH_GUARD")}
    env["LASSO_POISON"] = "1"
    if _STOPPED:
        pytest.fail(f"not started: {_STOPPED[0]}")
    t0 = time.perf_counter()
    try:
        res = subprocess.run([sys.executable, "-m", "pytest", *files, "-m", "gpu", "-k", select, "-x", "-q", "-p", "no:cacheprovider"],
                             cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        _STOPPED.append(f"the child `{group}` did not finish in {timeout} s")
        pytest.fail(f"the child `{group}` did not finish in {timeout} s\n{out[-3000:]}")
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    print(f"\n[stale memory] `{group}`: {last}, child {time.perf_counter() - t0:.1f} s")
    if res.returncode < 0 or res.returncode in (134, 139):
        _STOPPED.append(f"the child `{group}` was ended by a signal ({res.returncode})")
    assert res.returncode == 0, f"the child `{group}` ended with {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-2000:]}"
    assert "failed" not in last and "error" not in last, last
    m = re.search(r"(\d+) passed", last)
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_gives_the_same_bytes_on_filled_memory(group):
    assert run_child(group) > 0, f"no test of group {group} ran"
