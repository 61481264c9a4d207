"""CPU: LASSO_POISON=1 (lasso_amd/csrc/device_switches.cuh) over the oracle's mock — the host prover on allocations that start as the word 0x00000001 repeated instead of as
whatever malloc hands out (mostly zeros in a young process), and the pure part of the device library's fill.

  prover   tests/stale_cases.py in a child process (the switch is read once per process): the CASES of tests/test_host_prover_cpu.py and the first 8 configurations of each
           fuzz seed, on both curve builds, give the oracle's commitment and proof bytes, twice in a row on one prover; a fresh lasso_alloc of the mock holds the word
  slab     in the same child: tests/test_slab_sharding_cpu.py's proofs over 2 ranks, and its threads harness with the shared-memory exchange and capacity mode
  plan     tests/cpp/test_launch_plan_host.cpp (poison_range beside the guard's functions, the host fill, the word), plain and under -fsanitize=undefined

The device library's side of the switch needs the device: tests/test_gpu_write_contract.py (kernel level) and tests/test_gpu_stale_memory.py (proofs)."""
import os
import re
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SELECT = "test_stale_ or test_slab_threads_over_the_shm_exchange_and_capacity_mode or (test_slab_proof_equals_single_rank_and_oracle and -2])"


def test_host_prover_and_slab_mode_on_filled_allocations():
    env = dict(os.environ, LASSO_POISON="1")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.join(ROOT, "tests", "stale_cases.py"), os.path.join(ROOT, "tests", "test_slab_sharding_cpu.py"), "-m", "not gpu",
                          "-k", SELECT, "-x", "-q", "-p", "no:cacheprovider"], cwd=ROOT, env=env, capture_output=True, text=True, timeout=900)
    last = res.stdout.strip().splitlines()[-1] if res.stdout.strip() else ""
    print(f"\n[stale memory over the mock] {last}")
    assert res.returncode == 0, f"the child ended with {res.returncode}\n{res.stdout[-6000:]}\n{res.stderr[-2000:]}"
    m = re.search(r"(\d+) passed", last)
    from test_host_prover_cpu import CASES
    from test_slab_sharding_cpu import CASES as SLAB_CASES
    want = 2 + 2 * len(CASES) + 2 + 2 + len(SLAB_CASES)      # liveness, CASES and fuzz on both builds, the threads harness twice, every slab case over 2 ranks
    assert m and int(m.group(1)) == want and "failed" not in last and "skipped" not in last, (last, want)


@pytest.mark.parametrize("sanitize", [False, True], ids=["plain", "ubsan"])
def test_launch_plan_host_program(sanitize):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_launch_plan_host_stale" + ("_ubsan" if sanitize else "_plain"))
    flags = ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if sanitize else []
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_launch_plan_host.cpp")])
    env = {k: v for k, v in os.environ.items() if k not in ("LASSO_POISON", "LASSO_SCRATCH_GUARD")}      # the program asserts both defaults
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300, env=env)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
