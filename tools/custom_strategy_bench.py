#!/usr/bin/env python3
"""Measure what a caller-defined strategy (include/lasso_hip.h lasso_strategy_custom) costs next to the built-in it can be compared with, on the GPU.

  kernel level   lasso_sumcheck_combine_round at n = 2^22: Spark (g = prod_m E_m) as a one-term descriptor against the built-in LASSO_SPARK_UNCONFIRMED kernel at
                 C = 4, 8, 16 — the same number of field products per index and point, so the expectation is parity; and, for information, LT written out flat
                 (sum_i i products per point) against the built-in Horner kernel (C per point) at C = 8, 16.  Device events around each call (lasso_prof_*),
                 the two variants alternated in one process, `--reps` repetitions each; the built-in's own spread is reported beside the difference.
  end to end     prove time of AND-as-descriptor (C = 1, M = 2^16, 2^24 lookups: the headline shape) against built-in AND, and of Spark-as-descriptor (C = 4, 2^20)
                 against built-in Spark, alternating, host clock around a call that ends in the result hand-off; the proofs' bytes are compared.

Writes one JSON file (default profiles/custom_combine_round.json).  Needs the built libraries and a GPU; nothing here falls back to a CPU."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from lasso_amd import CustomStrategy, Device, HostProver, _abi, fr_words  # noqa: E402
from lasso_amd.custom import FR_MODULUS  # noqa: E402

P = FR_MODULUS["curve25519"]


def rand_fr(rng, n):
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(2**60 - 1)      # < 2^252 < p: a valid memory word
    return a


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "all_ms": ms}


def timed_round(dev, call):
    """device time of one lasso_sumcheck_combine_round-style call: the events the library brackets the family's launches with"""
    dev.prof_reset(); dev.prof_enable(1 << _abi.K_COMBINE)
    out = call()
    n, ms, _ = dev.prof_get(_abi.K_COMBINE)
    dev.prof_enable(0)
    assert n >= 1
    return ms, out


def kernel_level(reps, log_n):
    dev = Device(0)
    rng = np.random.default_rng(1)
    n = 1 << log_n
    polys = [dev.upload(rand_fr(rng, n)) for _ in range(32)]
    eq = dev.upload(rand_fr(rng, n))
    tables = [np.zeros(4, dtype=np.uint32)]
    rows = []

    def desc(alpha, terms):
        return CustomStrategy(alpha, 2, tables, terms, num_memories=alpha, memory_subtable=[0] * alpha, memory_dimension=list(range(alpha)))
    try:
        for c in (4, 8, 16):
            S = _abi.Strategy(_abi.KINDS["spark"], c, 16, 0)
            cs = desc(c, [(1, list(range(c)))])
            a = lambda: dev.sumcheck_combine_round(S, polys[:c], eq, n, c + 1)
            b = lambda: dev.sumcheck_combine_round(cs, polys[:c], eq, n, c + 1)
            a(); b()                                    # warm: code objects, scratch, the term list's upload
            ta, tb = [], []
            for _ in range(reps):
                ms, oa = timed_round(dev, a); ta.append(ms)
                ms, ob = timed_round(dev, b); tb.append(ms)
                assert np.array_equal(oa, ob), "the descriptor's round differs from the built-in's"
            alg = 32.0 * n * (c + 1)
            rows.append({"shape": f"spark C={c} n=2^{log_n}", "products_per_index_and_point": {"builtin": c, "custom": c}, "algorithmic_bytes": alg,
                         "builtin": summary(ta), "custom": summary(tb), "custom_over_builtin_median": statistics.median(tb) / statistics.median(ta),
                         "builtin_frac_of_8TBps": alg / (statistics.median(ta) * 1e-3) / 8e12, "custom_frac_of_8TBps": alg / (statistics.median(tb) * 1e-3) / 8e12})
        for c in (8, 16):                               # for information: LT flat against the Horner kernel
            S = _abi.Strategy(_abi.KINDS["lt"], c, 4, 0)
            cs = desc(2 * c, [(1, [2 * j + 1 for j in range(i)] + [2 * i]) for i in range(c)])
            scaled = [dev.alloc(n * 32) for _ in range(2 * c)]
            dev.lt_prescale(S, scaled, n, src=polys[:2 * c])
            a = lambda: dev.sumcheck_combine_round_lt_scaled(S, scaled, eq, n, c + 1)
            b = lambda: dev.sumcheck_combine_round(cs, polys[:2 * c], eq, n, c + 1)
            a(); b()
            ta, tb = [], []
            for _ in range(reps):
                ms, oa = timed_round(dev, a); ta.append(ms)
                ms, ob = timed_round(dev, b); tb.append(ms)
                assert np.array_equal(oa, ob), "LT written out flat differs from the built-in's round"
            for p in scaled:
                dev.free(p)
            alg = 32.0 * n * (2 * c + 1)
            rows.append({"shape": f"lt C={c} n=2^{log_n} (flat term list, for information)", "products_per_index_and_point": {"builtin": c, "custom": c * (c - 1) // 2 + 1},
                         "algorithmic_bytes": alg, "builtin": summary(ta), "custom": summary(tb), "custom_over_builtin_median": statistics.median(tb) / statistics.median(ta)})
    finally:
        for p in polys + [eq]:
            dev.free(p)
        dev.close()
    return rows


def eq_evals_int(point):
    out = [1]
    for r in point:
        out = [v for x in out for v in (x * (1 - r) % P, x * r % P)]
    return out


def and_descriptor(c, log_m):
    bits = log_m // 2
    idx = np.arange(1 << log_m, dtype=np.uint64)
    mask = np.uint64((1 << bits) - 1)
    return CustomStrategy(c, log_m, [((idx >> np.uint64(bits)) & mask) & (idx & mask)], [(1 << (i * bits), [i]) for i in range(c)])


def spark_descriptor(hp, c, log_m):
    rinv = pow(1 << 256, -1, P)
    tau = [(int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192) * rinv % P for w in hp.gen_random_point(c * log_m)]
    tables = [fr_words(eq_evals_int(tau[i * log_m:(i + 1) * log_m])) for i in range(c)]
    return CustomStrategy(c, log_m, tables, [(1, list(range(c)))], num_memories=c, memory_subtable=list(range(c)), memory_dimension=list(range(c)))


def end_to_end(reps):
    hp = HostProver()
    rows = []
    try:
        for kind, c, log_m, log_s in (("and", 1, 16, 24), ("spark", 4, 16, 20)):
            s = 1 << log_s
            idx = hp.gen_indices(s, 1 << log_m, c)
            r = hp.gen_random_point(log_s)
            S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
            cs = and_descriptor(c, log_m) if kind == "and" else spark_descriptor(hp, c, log_m)
            gens = hp.gens(c, s, c, log_m); hp.gens_prepare(gens)
            dense = hp.densify(idx, log_m)
            p0 = hp.prove(dense, gens, S, r); p1 = hp.prove(dense, gens, cs, r)      # warm both
            assert p0 == p1, "the descriptor's proof differs from the built-in's"
            ta, tb = [], []
            for _ in range(reps):
                t = time.perf_counter(); hp.prove(dense, gens, S, r); ta.append((time.perf_counter() - t) * 1e3)
                t = time.perf_counter(); hp.prove(dense, gens, cs, r); tb.append((time.perf_counter() - t) * 1e3)
            hp.free(dense, gens)
            rows.append({"shape": f"{kind} C={c} M=2^{log_m} lookups=2^{log_s}", "proof_bytes_equal": True, "builtin": summary(ta), "custom": summary(tb),
                         "custom_over_builtin_median": statistics.median(tb) / statistics.median(ta)})
    finally:
        hp.close()
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "custom_combine_round.json"))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--log-n", type=int, default=22)
    ap.add_argument("--skip-end-to-end", action="store_true")
    a = ap.parse_args()
    res = {"what": "tools/custom_strategy_bench.py", "reps": a.reps, "timing": "kernel level: HIP events around the launches of the combine family (lasso_prof_get); end to end: host clock around lasso_host_prove",
           "note": "built-in and descriptor variants alternate in one process; the built-in kernels are those of this build (their source is unchanged by the descriptor's addition)",
           "kernel_level": kernel_level(a.reps, a.log_n)}
    if not a.skip_end_to_end:
        res["end_to_end"] = end_to_end(a.reps)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    print(json.dumps({k: [(r["shape"], round(r["custom_over_builtin_median"], 3)) for r in v] for k, v in res.items() if isinstance(v, list)}))


if __name__ == "__main__":
    main()
