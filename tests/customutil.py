"""Helpers of the caller-defined-strategy tests: the built-in strategies re-expressed as descriptors (lasso_amd.CustomStrategy), two strategies the reference does
not ship, a big-integer evaluation of a term list, and the CPU build of the host prover against the wrapped mock (tests/cpp/mock_custom_wrap.cpp)."""
import os

import numpy as np

from lasso_amd import CustomStrategy, _abi, fr_words
from lasso_amd.custom import FR_MODULUS
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def build_mock_prover_custom(curve="curve25519"):
    """the host prover over the mock with the two strategy-taking entry points wrapped (tests/cpp/mock_custom_wrap.cpp): custom strategies can be PROVED on the CPU"""
    return build_mock_prover(curve, ext=("custom",))


# ---- the built-in strategies as descriptors (materialize_subtables of and.rs / or.rs / xor.rs / lt.rs / range_check.rs, restated)

def _split(log_m):
    bits = log_m // 2
    idx = np.arange(1 << log_m, dtype=np.uint64)
    mask = np.uint64((1 << bits) - 1)
    return (idx >> np.uint64(bits)) & mask, idx & mask


def builtin_as_custom(kind, c, log_m, log_r=0, curve="curve25519", host=None):
    """the descriptor equivalent to _abi.Strategy(KINDS[kind], c, log_m, log_r).  "spark" needs `host` (a HostProver over the same curve): its tables are
    EqPolynomial(tau_i).evals() for the tau the strategy fixes, restated here as field-element tables (spark_tables)."""
    l, r = _split(log_m)
    if kind in ("and", "or", "xor"):
        t = {"and": l & r, "or": l | r, "xor": l ^ r}[kind]
        inc = log_m // 2
        return CustomStrategy(c, log_m, [t], [(1 << (i * inc), [i]) for i in range(c)], curve=curve)
    if kind == "lt":
        lt, eq = (l < r).astype(np.uint64), (l == r).astype(np.uint64)
        terms = [(1, [2 * j + 1 for j in range(i)] + [2 * i]) for i in range(c)]          # lt.rs:62-71 written out flat: LT_i prod_{j<i} EQ_j
        return CustomStrategy(c, log_m, [lt, eq], terms, curve=curve)
    if kind == "range":
        m = 1 << log_m
        idx = np.arange(m, dtype=np.uint64)
        cutoff = 1 << (log_r % log_m)
        tables = [idx, np.where(idx < cutoff, idx, 0), np.zeros(m, dtype=np.uint64)]
        sub = [2 if i * log_m > log_r else (1 if (i + 1) * log_m > log_r else 0) for i in range(c)]     # range_check.rs:62-69
        return CustomStrategy(c, log_m, tables, [(1 << (i * log_m), [i]) for i in range(c)], num_memories=c, memory_subtable=sub, memory_dimension=list(range(c)), curve=curve)
    if kind == "spark":
        tables = spark_tables(c, log_m, curve, host)
        return CustomStrategy(c, log_m, tables, [(1, list(range(c)))], num_memories=c, memory_subtable=list(range(c)), memory_dimension=list(range(c)), curve=curve)
    raise ValueError(kind)


def eq_evals_int(point, p):
    """EqPolynomial(point).evals() on Python ints (eq_poly.rs:22-38: point[0] <-> the top bit)"""
    out = [1]
    for r in point:
        out = [v for x in out for v in (x * (1 - r) % p, x * r % p)]
    return out


def spark_tables(c, log_m, curve, host):
    """Spark's subtables as field-element tables: tau = C * log2(M) draws of F::rand from a fresh test_rng — the stream host.gen_random_point draws from"""
    p = FR_MODULUS[curve]
    pt = host.gen_random_point(c * log_m)
    rinv = pow(1 << 256, -1, p)
    tau = [(int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192) * rinv % p for w in pt]
    return [fr_words(eq_evals_int(tau[i * log_m:(i + 1) * log_m], p), curve) for i in range(c)]


# ---- two strategies the reference does not ship

def lte_strategy(c, log_m, curve="curve25519"):
    """LTE over operand chunks: x <= y  =  LT(x, y) + EQ(x, y)  =  sum_i LT_i prod_{j<i} EQ_j  +  prod_j EQ_j — mixed term lengths (1 .. C), with the all-EQ term
    entered as 2 * prod EQ - prod EQ so that a coefficient of -1 (p - 1) is on the path.  Subtables LT, EQ as lt.rs's; memories 2i = LT_i, 2i + 1 = EQ_i."""
    l, r = _split(log_m)
    terms = [(1, [2 * j + 1 for j in range(i)] + [2 * i]) for i in range(c)]
    all_eq = [2 * j + 1 for j in range(c)]
    terms += [(2, all_eq), (-1, all_eq)]
    return CustomStrategy(c, log_m, [(l < r).astype(np.uint64), (l == r).astype(np.uint64)], terms, curve=curve)


def field_square_strategy(c, log_m, seed, curve="curve25519"):
    """field-element tables, a squared memory and a constant term: g = 7 + 3 * E_0^2 * E_1 - E_{C-1} + 5 * E_0 (C >= 2), one random table per dimension"""
    p = FR_MODULUS[curve]
    rng = np.random.default_rng(seed)
    vals = [[int.from_bytes(rng.bytes(40), "little") % p for _ in range(1 << log_m)] for _ in range(c)]
    tables = [fr_words(v, curve) for v in vals]
    terms = [(7, []), (3, [0, 0, 1]), (-1, [c - 1]), (5, [0])]
    cs = CustomStrategy(c, log_m, tables, terms, num_memories=c, memory_subtable=list(range(c)), memory_dimension=list(range(c)), curve=curve)
    cs.table_values = vals
    return cs


def g_int(terms, vals, p):
    """g(vals) on Python ints for a term list [(coeff, [memory, ...]), ...]"""
    total = 0
    for cf, mems in terms:
        t = cf % p
        for m in mems:
            t = t * vals[m] % p
        total += t
    return total % p
