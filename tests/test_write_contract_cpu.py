"""CPU: the write contract (tests/writecontract.py) covers exactly the exported symbols, and the arena harness (tests/arenautil.py, tests/arena_cases.py) holds over the
oracle's mock, whose device memory is host memory: every re-collected case passes with nothing written outside its calls' write sets, and every planted write and shrunk
contract of the sensitivity cases is reported with the right owner.

The mock is a serial CPU statement of every call, so the cases are limited to parameters of at most MAX_PARAM (2^11): larger shapes run on the device only
(tests/test_gpu_write_contract.py).  Measured: 359 cases (128 above the limit deselected) in 17 to 42 s, depending on the host's cores."""
import os
import time

import pytest

import writecontract
from test_abi_exports import header_functions

HERE = os.path.dirname(os.path.abspath(__file__))
MAX_PARAM = 1 << 11
EXTRA_HEADERS = ("lasso_hip_wire.h", "lasso_hip_gens.h", "lasso_hip_msm.h", "lasso_hip_operands.h")


def exported_symbols():
    """what tests/test_abi_exports.py lists — the device library's header and the host prover's — plus the device library's four smaller headers"""
    names = set(header_functions("lasso_hip.h")) | {n for n in header_functions("lasso_prover.h") if n.startswith("lasso_host_")}
    for h in EXTRA_HEADERS:
        names |= {n for n in header_functions(h) if n.startswith("lasso_") and not n.startswith("lasso_host_")}
    return names


def test_contract_covers_exactly_the_exported_symbols():
    have, want = set(writecontract.CONTRACT), exported_symbols()
    assert not want - have, f"no write contract for {sorted(want - have)}"
    assert not have - want, f"contract entries for names no header exports: {sorted(have - want)}"
    assert all(callable(f) for f in writecontract.CONTRACT.values())


class _Limit:
    """cases with an integer parameter above MAX_PARAM are left to the device"""

    def __init__(self):
        self.kept = self.dropped = 0

    def pytest_collection_modifyitems(self, config, items):
        keep, drop = [], []
        for it in items:
            params = getattr(getattr(it, "callspec", None), "params", {})
            big = any(isinstance(v, int) and v > MAX_PARAM for v in params.values())
            row = params.get("row")
            if row is not None:
                vals = list(getattr(row, "shape", ())) + list(getattr(row, "args", {}).values())
                big = big or any(isinstance(v, int) and v > MAX_PARAM for v in vals)
            (drop if big else keep).append(it)
        config.hook.pytest_deselected(items=drop)
        items[:] = keep
        self.kept, self.dropped = len(keep), len(drop)


def test_arena_cases_hold_over_the_mock(monkeypatch):
    monkeypatch.setenv("LASSO_ARENA_OVER", "mock")
    monkeypatch.setenv("LASSO_ARENA_SETTING", "0")
    limit = _Limit()
    t0 = time.perf_counter()
    rc = pytest.main([os.path.join(HERE, "arena_cases.py"), "-q", "-x", "-p", "no:cacheprovider", "--no-header", "-W", "ignore::pytest.PytestAssertRewriteWarning"], plugins=[limit])
    print(f"\n[write contract over the mock] {limit.kept} cases ({limit.dropped} above {MAX_PARAM} left to the device): {time.perf_counter() - t0:.1f} s")
    assert rc == 0, f"tests/arena_cases.py over the mock ended with {rc} (its report is above)"
    assert limit.kept >= 300
