"""-m gpu: tests/arena_cases.py on the device — the suite's kernel-level calls once more with every caller buffer inside one patterned allocation (tests/arenautil.py), at
interior pointers no more aligned than the element type needs, and after each case all memory outside the calls' documented write sets (tests/writecontract.py) must be
unchanged.  One child pytest per group of cases and per switch setting (the switches are read once per process), each with its own time limit; a failing child ends its test and
nothing is retried.  Runs on the build LASSO_TEST_CURVE selects (tests/test_gpu_bn254.py re-runs the module on the BN254 build).

Every child runs with LASSO_SCRATCH_GUARD=1: the library puts 64 KiB of guard pattern directly behind the requested size of every request of its scratch, sort and big-result
buffers, and the lasso_sync that ends each case (tests/arena_cases.py arena_case) fails the case that damaged one.  A child that does not finish in its time limit, or is ended
by a signal, is the last one started: the tests after it fail at once.

Every child also runs with LASSO_POISON=1: each allocation of the library starts as the word 0x00000001 repeated, and the first request a public call makes of the scratch, sort
or big-result buffer fills its requested range with the word in stream order (in front of the guard).  A case whose kernels read a partial, a bucket sum or a table entry that
the call did not store then computes with the word instead of with zeros or with what the identical call before it left there, and fails its own parity assertion; nothing else
is asserted for it.  The last two sensitivity cases read fresh lasso_alloc memory back and require the word everywhere, the second after the scratch has grown beyond its floor
with live data and been trimmed, twice.

Measured on an MI355X with both switches on: 873 cases in 22 children, 130 s for the module on the curve25519 build and 124 s on the BN254 build (131 s before the fill was
added: the memsets do not show); the longest child is the curve group (88 cases, 40 s: the commitments' reference runs on the mock), then the round group (120 cases, 14 s) and
LASSO_REDUCE_NX=3 (77 rows, 12 s); every other child takes 2 to 9 s.  Cases per group: sensitivity 13, kernels 211 + 88 + 120, field edges 66 + 77, operands 65, MSM over caller
points 22, wire points 8, candidates 8, table rows 75 / 5 / 8 / 4 / 77 / 8 / 7 / 1 / 1 / 9 in the order of SETTINGS.  No stray write, no damaged guard and no
stale read was found on either build."""
import os
import re
import subprocess
import sys
import time

import pytest

from arenautil import SETTINGS      # by index: the child reads LASSO_ARENA_SETTING and checks its own environment against the same table
import passvariants as PV
import roundvariants as RV

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

_STOPPED = []      # why no further child is started: one did not finish in its time limit or was ended by a signal, and nothing more is run on a device in that state

_KA = "bind or eq_evals or combine or lt_ or multi_dot or gp_build or fingerprint or matvec or materialize or read_runs or densify"
_KB = "hyrax or msm or slab or inner_products or bullet"
_KC = "cubic or linear or layer"
# group -> the child's -k expression; the *_rest groups make the split complete whatever a test is called
GROUPS = {
    "sensitivity": "test_sens_",
    "kernels_streaming": f"test_k_ and ({_KA})",
    "kernels_curve": f"test_k_ and ({_KB}) and not ({_KA})",
    "kernels_rounds": f"test_k_ and ({_KC}) and not ({_KA}) and not ({_KB})",
    "kernels_rest": f"test_k_ and not ({_KA}) and not ({_KB}) and not ({_KC})",
    "field_edges_lazy": "test_fe_lazy",
    "field_edges_edge": "test_fe_edge",
    "field_edges_rest": "test_fe_ and not test_fe_lazy and not test_fe_edge",
    "operands": "test_op_",
    "msm_points": "test_mp_",
    "wire_points": "test_wp_",
    "gens_device": "test_gd_",
}
MAY_BE_EMPTY = ("kernels_rest", "field_edges_rest")


def run_child(select, setting, timeout):
    """tests/arena_cases.py -k `select` on the device, in a fresh process under SETTINGS[setting] -> the number of cases that passed"""
    env = {k: v for k, v in os.environ.items() if k not in RV.SWITCHES + PV.SWITCHES and not k.startswith("LASSO_MSM_") and k not in ("LASSO_ARENA_OVER", "LASSO_POISON")}
    env.update(SETTINGS[setting])
    env["LASSO_ARENA_SETTING"] = str(setting)
    env["LASSO_SCRATCH_GUARD"] = "1"      # the library's own buffers: a guard behind every request's size, reported by the lasso_sync that ends each case
    env["LASSO_POISON"] = "1"             # ... and in front of every call's own data the fill word, not zeros or an earlier call's bytes: a stale read fails the case's parity
    if _STOPPED:
        pytest.fail(f"not started: {_STOPPED[0]}")
    t0 = time.perf_counter()
    try:
        res = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "arena_cases.py"), "-m", "gpu", "-k", select, "-x", "-q", "-p", "no:cacheprovider"],
                             cwd=ROOT, env=env, capture_output=True, text=True, timeout=timeout)
    except subprocess.TimeoutExpired as e:
        out = e.stdout.decode(errors="replace") if isinstance(e.stdout, bytes) else (e.stdout or "")
        _STOPPED.append(f"the child `{select}` under {SETTINGS[setting]} did not finish in {timeout} s")
        pytest.fail(f"the child `{select}` under {SETTINGS[setting]} did not finish in {timeout} s\n{out[-3000:]}")
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    print(f"\n[write contract] `{select}` under {SETTINGS[setting] or 'the defaults'}: {last}, child {time.perf_counter() - t0:.1f} s")
    if res.returncode < 0 or res.returncode in (134, 139):
        _STOPPED.append(f"the child `{select}` under {SETTINGS[setting]} was ended by a signal ({res.returncode})")
    if res.returncode == 5:      # nothing selected
        return 0
    assert res.returncode == 0, f"the child `{select}` under {SETTINGS[setting]} ended with {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-2000:]}"
    assert "failed" not in last and "error" not in last, last
    m = re.search(r"(\d+) passed", last)
    return int(m.group(1)) if m else 0


@pytest.mark.parametrize("group", list(GROUPS))
def test_group_writes_only_what_its_calls_may_write(group):
    passed = run_child(GROUPS[group], 0, timeout=300)
    assert passed > 0 or group in MAY_BE_EMPTY, f"no case of group {group} ran"


@pytest.mark.parametrize("setting", range(len(SETTINGS)), ids=["default" if not s else ",".join(f"{k}={v}" for k, v in sorted(s.items())) for s in SETTINGS])
def test_table_rows_of_the_setting_write_only_what_their_calls_may_write(setting):
    assert run_child("test_tab_", setting, timeout=300) > 0
