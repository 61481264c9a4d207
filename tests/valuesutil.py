"""Helpers of the lookup-value tests (tests/test_lookup_values_cpu.py, tests/test_gpu_lookup_values.py): the CPU build of the host prover against the mock with
lasso_lookup_values added (tests/cpp/mock_values_wrap.cpp), every strategy kind as (strategy, its descriptor restatement), Python big-integer values, the shapes the GPU
tests run (here so that the CPU test can hold them against the launch plan without importing a GPU module)."""
import os

import numpy as np

import customutil as U
import mleutil as M
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]
R = 1 << 256
U64_TEXT = "the 64-bit form is offered over integer tables for LT"      # the start of VALUES_MSG_U64 (lasso_amd/csrc/values_combine.cuh)


def build_mock_prover_values(curve="curve25519"):
    """build_mock_prover_mle's library with lasso_lookup_values on top (tests/cpp/mock_values_wrap.cpp: a literal loop), so lasso_host_lookup_values takes its
    device route on the CPU; include/lasso_hip_poly.h stays absent"""
    return build_mock_prover(curve, ext=("custom", "mle", "values"))


# ---- every strategy kind: (name, what the C ABI takes, the same strategy as a descriptor whose tables and term list Python can read)

def builtin(kind, c, log_m, log_r=0):
    return _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)


def all_kinds(curve, host, c=2, log_m=4):
    """one strategy of every kind at (c, log_m): the five built-in integer kinds, Spark, and four caller-defined ones — [(name, strategy, descriptor)]"""
    out = []
    for kind, log_r in (("and", 0), ("or", 0), ("xor", 0), ("lt", 0), ("range", log_m + 1), ("spark", 0)):
        out.append((kind, builtin(kind, c, log_m, log_r), U.builtin_as_custom(kind, c, log_m, log_r, curve, host=host)))
    for name, cs in (("lte", U.lte_strategy(c, log_m, curve)), ("field_square", U.field_square_strategy(c, log_m, 5, curve)),
                     ("xor_as_custom", U.builtin_as_custom("xor", c, log_m, 0, curve)), ("lt_as_custom", U.builtin_as_custom("lt", c, log_m, 0, curve))):
        out.append((name, cs, cs))
    return out


def u64_offered(kind, c, log_m):
    """the rule of include/lasso_hip_values.h, restated: LT always; the linear kinds when sum_i 2^(i * inc) * max_table_value < 2^64"""
    if kind == "lt":
        return True
    if kind not in ("and", "or", "xor", "range"):
        return False
    inc = log_m if kind == "range" else log_m // 2
    mx = (1 << log_m) - 1 if kind == "range" else (1 << (log_m // 2)) - 1
    return sum(mx << (i * inc) for i in range(c)) < 1 << 64


# ---- Python integers

def table_ints(desc):
    """the descriptor's tables as lists of Python ints (field tables: the values behind the memory words, whatever representative they hold)"""
    p = FR_MODULUS[desc.curve]
    if not desc.field:
        return [[int(v) for v in t] for t in desc.tables]
    rinv = pow(R, -1, p)
    return [[w * rinv % p for w in M.word_ints(t)] for t in desc.tables]


def values_int(desc, idx, s=None, tables=None):
    """v[k] = g(T[sub(i)][idx[k][dim(i)]]) as Python ints mod p, k < s (default next_pow2(rows)); rows behind idx read address 0"""
    p = FR_MODULUS[desc.curve]
    tables = tables or table_ints(desc)
    n = idx.shape[0]
    s = s if s is not None else 1 << max((n - 1).bit_length(), 0)
    maps = [desc.memory_map(i) for i in range(desc.num_memories)]
    out = []
    for k in range(s):
        row = idx[k] if k < n else [0] * desc.c
        out.append(U.g_int(desc.terms, [tables[sub][int(row[dim])] for sub, dim in maps], p))
    return out


def words_to_ints(words, curve):
    """(n, 4) memory words -> the integers behind them; asserts every word is canonical (below p)"""
    p = FR_MODULUS[curve]
    ws = M.word_ints(words)
    assert all(w < p for w in ws), "a memory word is not fully reduced"
    rinv = pow(R, -1, p)
    return [w * rinv % p for w in ws]


def mle_int(values, r_words, curve):
    """sum_k eq(r, k) values[k] on Python ints"""
    p = FR_MODULUS[curve]
    chi = M.chi_int(r_words, p) if len(r_words) else [1]
    return sum(v * c for v, c in zip(values, chi)) % p


def claim_int(words, curve):
    return words_to_ints(np.asarray(words).reshape(1, 4), curve)[0]


def walker_claim(proof):
    """the byte walk the custom-strategy tests carry privately (surge.rs:92-104 in wire order): the canonical integer of claimed_evaluation"""
    pos = 8 + 32 * int.from_bytes(proof[:8], "little")
    rounds = int.from_bytes(proof[pos:pos + 8], "little"); pos += 8
    for _ in range(rounds):
        pos += 8 + 32 * int.from_bytes(proof[pos:pos + 8], "little")
    return int.from_bytes(proof[pos:pos + 32], "little"), pos


def random_indices(c, log_m, n, seed, corners=True):
    """n x c addresses; with `corners`, every dimension sees address 0 and address M - 1 at the first, the last and a middle lookup (first: all 0, last: all M - 1, middle:
    alternating; from five lookups on also the second: all M - 1 and the last but one: all 0)"""
    idx = np.random.default_rng(seed).integers(0, 1 << log_m, size=(n, c), dtype=np.uint64)
    if corners:
        top = (1 << log_m) - 1
        idx[0, :] = 0
        if n >= 2:
            idx[n - 1, :] = top
        if n >= 3:
            idx[n // 2, ::2] = 0; idx[n // 2, 1::2] = top
        if n >= 5:
            idx[1, :] = top; idx[n - 2, :] = 0
    return np.ascontiguousarray(idx)


# ---- the identity, over any host (mock or product library)

def check_identity(hp, curve, name, st, desc, idx, log_m):
    """lookup_values == _ref == Python; MLE(values)(r) == the proof's claim; the proof is what it was before the call.  One lookup (s = 1) has no proof — the prover's
    product trees need two leaves and say so — so there the vector and its evaluation in no variables are held to the CPU statement and Python alone."""
    from lasso_amd.device import LassoError
    n, c = idx.shape
    s = 1 << max((n - 1).bit_length(), 0)
    r = hp.gen_random_point(s.bit_length() - 1)
    gens = hp.gens(c, s, desc.num_memories, log_m)
    dense = hp.densify(idx, log_m)
    try:
        before = None
        if s >= 2:
            before = hp.prove(dense, gens, st, r)
        else:
            try:
                hp.prove(dense, gens, st, r)
                raise AssertionError("a proof of one lookup exists now: hold it to the identity too")
            except LassoError:
                pass
        base = hp.values_stats()["device_lookups"]
        vals = hp.lookup_values(dense, st)
        assert hp.values_stats()["device_lookups"] == base + s, name
        assert np.array_equal(vals, hp.lookup_values_ref(st, idx)), name
        ints = words_to_ints(vals, curve)
        assert ints == values_int(desc, idx), name
        got = hp.values_evaluate(vals, r)
        assert claim_int(got, curve) == mle_int(ints, r, curve), name
        if before is not None:
            after = hp.prove(dense, gens, st, r)
            assert after == before, name
            claim = hp.claimed_evaluation(after)
            assert claim_int(claim, curve) == walker_claim(after)[0], name
            assert np.array_equal(got, claim), name
        if u64_offered(name, c, log_m):
            assert [int(v) for v in hp.lookup_values(dense, st, form="u64")] == ints, name
    finally:
        hp.free(dense, gens)


# argv: root, library ("" = the product library of `curve`), curve, lookups.  Capacity mode with a compact representation (the caller sets LASSO_LEAFLESS_MIN): the identity
# for an integer linear kind, LT, Spark and a caller-defined strategy over field tables; prints one JSON line.
CAPACITY_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd.prover import HostProver
import valuesutil as V
lib, curve, lookups = sys.argv[2], sys.argv[3], int(sys.argv[4])
hp = HostProver(C.CDLL(lib) if lib else None, curve=curve)
hp.set_capacity(True)
c, log_m = 2, 4
idx = V.random_indices(c, log_m, lookups, seed=3)
probe = hp.densify(idx, log_m)
compact = hp.dense_info(probe)["compact"]
hp.free(probe)
done = []
for name, st, desc in V.all_kinds(curve, hp, c=c, log_m=log_m):
    if name in ("and", "lt", "spark", "field_square"):
        V.check_identity(hp, curve, name, st, desc, idx, log_m)
        done.append(name)
print(json.dumps({"compact": compact, "kinds": done}))
hp.close()
"""


# ---- what tests/test_gpu_lookup_values.py runs
GPU_NS = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 1025]
GPU_NX = 3                      # LASSO_VALUES_NX in the GPU test's child
GPU_N_PASSES = 3075             # odd; under GPU_NX workgroups both kernels walk at least three passes per lane (derived in test_lookup_values_cpu.py)
GPU_CS = [1, 2, 4, 8]
GPU_LOG_MS = [2, 4, 8, 16]
GPU_KINDS = ["and", "or", "xor", "lt", "range", "spark", "xor_as_custom", "lte", "field_lazy", "big_u32"]
PATTERN = 0xA5
TAIL = 64 << 10                 # pattern-filled bytes behind the s elements of d_out
LAZY_BOUND = 2**254 + 2**130


def gpu_strategy(kind, c, log_m, curve, host, seed=1):
    """(what the C ABI takes, the descriptor Python reads) for one of GPU_KINDS, or None where the kind has no such shape"""
    p = FR_MODULUS[curve]
    if kind in ("and", "or", "xor", "lt", "spark"):
        return builtin(kind, c, log_m), U.builtin_as_custom(kind, c, log_m, 0, curve, host=host)
    if kind == "range":
        log_r = c * log_m - (log_m // 2 if c > 1 else 0)          # the top chunk is a remainder chunk
        return builtin(kind, c, log_m, log_r), U.builtin_as_custom(kind, c, log_m, log_r, curve)
    if kind == "xor_as_custom":
        cs = U.builtin_as_custom("xor", c, log_m, 0, curve)
        return cs, cs
    if kind == "lte":
        cs = U.lte_strategy(c, log_m, curve)
        return cs, cs
    rng = np.random.default_rng(seed + 100 * c + log_m)
    m = 1 << log_m
    if kind == "big_u32":       # u32 tables whose entries reach 2^32 - 1, a product, a square and a negative coefficient
        tables = [rng.integers(0, 2**32, size=m, dtype=np.uint64) for _ in range(c)]
        for t in tables:
            t[0] = 2**32 - 1; t[m - 1] = 2**32 - 1; t[m // 2] = 0
        terms = [(1, [0]), (3, [0, c - 1]), (-1, [c - 1, c - 1, 0]), (5, [])] + [(2, [i]) for i in range(1, c)]
        cs = U.CustomStrategy(c, log_m, tables, terms, num_memories=c, memory_subtable=list(range(c)), memory_dimension=list(range(c)), curve=curve)
        return cs, cs
    if kind == "field_lazy":    # field tables holding lazily reduced representatives: the largest multiple of p that keeps the word below 2^254 + 2^130 is added
        if c < 2:
            return None
        cs = U.field_square_strategy(c, log_m, seed, curve)
        for t in cs.tables:
            ws = M.word_ints(t)
            lazy = [w + (LAZY_BOUND - 1 - w) // p * p for w in ws]
            lazy[1 % m] = ws[1 % m]                                  # one canonical word stays
            t[:] = M.int_words(lazy)
        return cs, cs
    raise ValueError(kind)


def gpu_shapes(kind):
    """[(c, log_m, ns)]: every n at one shape, every (C, log_m) of the lists at n = 3 and 257; C = 16 for LT and Spark.  Kinds whose 2^16-entry FIELD tables are built on
    Python integers (Spark's eq tables, field_lazy's random ones: seconds per table set) meet log_m = 16 at C = 2 only — the kernel's table reads do not depend on C"""
    main = (4, 8)
    out = [(main[0], main[1], GPU_NS + [GPU_N_PASSES])]
    cs = GPU_CS + ([16] if kind in ("lt", "spark") else [])
    for c in cs:
        for log_m in GPU_LOG_MS:
            if (c, log_m) != main and not (kind in ("spark", "field_lazy") and log_m == 16 and c != 2):
                out.append((c, log_m, [3, 257]))
    return out


def shape_valid(kind, c, log_m):
    """(C - 1) * inc < 64 for the weighted sums (RangeCheck: inc = log_m): the library refuses the others"""
    if kind in ("and", "or", "xor"):
        return (c - 1) * (log_m // 2) < 64
    if kind == "range":
        return (c - 1) * log_m < 64
    return True


# argv: root, curve, kind.  The kernel against Python integers at every shape of gpu_shapes, both forms where offered, d_out followed by a pattern; prints one JSON line.
# The caller sets LASSO_VALUES_NX, LASSO_POISON and LASSO_SCRATCH_GUARD (read once per process).
KERNEL_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import Device, _abi
from lasso_amd.custom import strategy_ptr
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver
import valuesutil as V
curve, kind = sys.argv[2], sys.argv[3]
dev = Device(0, curve=curve)
host = HostProver(curve=curve) if kind == "spark" else None
cases, failures, refusals = 0, [], []
for c, log_m, ns in V.gpu_shapes(kind):
    made = V.gpu_strategy(kind, c, log_m, curve, host)
    if made is None:
        continue
    st, desc = made
    tables = V.table_ints(desc)
    d_tabs = [dev.upload(t) for t in desc.tables]
    try:
        if not V.shape_valid(kind, c, log_m):
            d_dim = [dev.upload(np.zeros(4, dtype=np.uint32)) for _ in range(c)]; d_out = dev.alloc(256)
            try:
                dev.lookup_values(strategy_ptr(st), d_dim, d_tabs, desc.field, 3, _abi.VALUES_FR, d_out)
                failures.append(f"{kind} c={c} log_m={log_m}: a shape with (C - 1) * inc >= 64 was accepted")
            except LassoError as e:
                refusals.append(str(e))
            for q in d_dim + [d_out]:
                dev.free(q)
            continue
        forms = [("field", _abi.VALUES_FR, 32)] + ([("u64", _abi.VALUES_U64, 8)] if V.u64_offered(kind, c, log_m) else [])
        for n in ns:
            idx = V.random_indices(c, log_m, n, seed=n + c)
            want = V.values_int(desc, idx, s=n, tables=tables)
            d_dim = [dev.upload(np.ascontiguousarray(idx[:, j].astype(np.uint32))) for j in range(c)]
            for name, form, elem in forms:
                buf = np.full(n * elem + V.TAIL, V.PATTERN, dtype=np.uint8)
                d_out = dev.upload(buf)
                dev.lookup_values(strategy_ptr(st), d_dim, d_tabs, desc.field, n, form, d_out)
                dev.sync()
                got = dev.download(d_out, buf.shape, dtype=np.uint8)
                dev.free(d_out)
                cases += 1
                tag = f"{kind} c={c} log_m={log_m} n={n} {name}"
                if not (got[n * elem:] == V.PATTERN).all():
                    failures.append(tag + ": bytes behind the n elements were written")
                if name == "u64":
                    vals = [int(x) for x in got[:n * 8].view(np.uint64)]
                else:
                    ws = V.M.word_ints(got[:n * 32].view(np.uint64).reshape(n, 4))
                    p = V.FR_MODULUS[curve]
                    if any(w >= p for w in ws):
                        failures.append(tag + ": an element is not canonical")
                    rinv = pow(V.R, -1, p)
                    vals = [w * rinv % p for w in ws]
                if vals != want:
                    bad = [k for k in range(n) if vals[k] != want[k]]
                    failures.append(tag + f": {len(bad)} wrong values, first at {bad[0]}")
            if not V.u64_offered(kind, c, log_m) and n == ns[0]:
                d_out = dev.alloc(8 * n + 16)
                try:
                    dev.lookup_values(strategy_ptr(st), d_dim, d_tabs, desc.field, n, _abi.VALUES_U64, d_out)
                    failures.append(f"{kind} c={c} log_m={log_m}: the 64-bit form was not refused")
                except LassoError as e:
                    refusals.append(str(e))
                dev.free(d_out)
            for q in d_dim:
                dev.free(q)
    finally:
        for q in d_tabs:
            dev.free(q)
dev.sync()          # LASSO_SCRATCH_GUARD: verified here; raises if a guard is damaged
print(json.dumps({"cases": cases, "failures": failures[:20], "refusals": sorted(set(refusals))}))
if host: host.close()
dev.close()
"""
