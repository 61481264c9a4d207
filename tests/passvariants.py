"""The launches that make every lazily reduced running sum of the sumcheck kernels reach its fold (lasso_amd/csrc/poly_kernels.cuh, k_inner_lr of lasso_hip.hip), as ONE table of
calls: switch setting, entry point, shape, data set, the kernel instantiation the row is there for, that kernel's fold period P (counted in passes of a thread's grid-stride
loop), the items a workgroup takes per pass, and the claim the row makes:

  fold+      some thread makes more than P passes and its count is no multiple of P: it folds, and accumulates again on the folded sum;
  carry      (P = 3) threads whose pass counts leave remainder 0 and a non-zero remainder both exist, each with at least 4 passes;
  stage2 k   the second stage (reduce_partials_row) sums nx > 256 partials per row: k passes of ITS loop.

Two users:

  tests/test_pass_reach_cpu.py     holds every row to its claim with the grid tests/cpp/pass_plan_dump.cpp prints for it (round_nx, cubic_plan, reduce_nx and matvec_plan of
                                   launch_plan.cuh over the real switch table, one child process per setting), the periods to the source text, and the union of the rows to every
                                   kernel that keeps such a sum — without a GPU;
  tests/test_gpu_pass_variants.py  runs every row on the device, one child process per setting, against the oracle's mock, byte for byte.

Largest number of passes a thread makes in the GPU suite, without these rows -> with them: k_cubic_round_lb, k_cubic_eqw_lb<3>, k_cubic_eqw_fused<3> and <2, narrow> 8 -> 171;
the linear rounds 1 -> 171 (k_dot_eqw_lb, k_dot_eqw_fused<false>), 1 -> 6 (the u32 forms, the round launched ahead); k_combine_round_linear 1 -> 86; the LT, Spark, bits and
caller-defined rounds 1 -> 86 (T = 1, 2), 65 (T = 3), 108 (T = 5); k_combine_claim<A>, k_combine_claim_custom, k_inner_lr 1 -> 171; k_multi_dot 1 -> 6; k_matvec_left 2 -> 7;
k_matvec_reduce 256 (two whole periods, nothing behind the last fold) -> 200 as well; the second stage 1 -> 4.

LASSO_CUBIC_NX=3 and LASSO_REDUCE_NX=3 (device_switches.cuh) bring the folds within reach of arrays of 2^13 .. 2^19 elements: 3 workgroups share the blocks of a launch, so a
thread makes a third of the launch's passes.  3 is no multiple of 8: cubic_grid takes its plain branch.

Every row runs on two data sets: `uniform` (uniform field elements) and `extreme`, which maximises what a running sum holds between two folds: every element of every array is
the largest representative below LAZY_BOUND of p - 1, (p - 1) / 2 or the word whose low eight 29-bit limbs are all ones, cycled (every entry here accepts lazily reduced
arrays).  The u32 entries take the largest integers they accept: 2^32 - 1 for the linear rounds; bits for the LT round, in the patterns `ones` and `alternating` of
test_lt_first_round_from_bits.  lasso_sumcheck_combine_round_lt_scaled is called on the arrays as they are (no lasso_lt_prescale in front): it is a polynomial in its inputs like
the others, and the extreme representatives reach it unchanged.

Out of scope: the 128-folds of k_bullet_step (its 129th pass comes at nk = 2^22) and of the inner-product workgroup of k_bullet_msm (nk >= 2^16: 65,538 generators with their
multiple tables — no few-second test).  Their arithmetic is acc_add's (add, carry pass, a product with one_s every 128 terms), which tests/cpp/test_fr29_host.cpp runs through
whole fold periods on the CPU under UBSan.

Run as a program (`python tests/passvariants.py <index into ENVS>`) it is the child process: it runs the setting's rows on the device and prints every output as hex (arrays
above 4 KiB: the SHA-256 of their bytes).  The curve is fieldref.CURVE (LASSO_TEST_CURVE), as for tests/gpuutil.py."""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np

from roundvariants import ROOT, SWITCHES as ROUND_SWITCHES, _vp, _wait, env_id

SWITCHES = ROUND_SWITCHES + ("LASSO_REDUCE_NX",)

# row: args is the entry's shape as a dict (n, k / c / kind / strategy name ...); purpose: what the row is the only one of its setting to reach
Row = namedtuple("Row", "id env entry args data kernel period per_pass claim purpose")

CN3 = {"LASSO_CUBIC_NX": "3"}
CN3_NARROW = {"LASSO_CUBIC_NX": "3", "LASSO_CUBIC_WIDE": "0"}
RN3 = {"LASSO_REDUCE_NX": "3"}
DEFAULT = {}

# DISPATCH_LT / DISPATCH_CUSTOM of lasso_hip.hip, restated (tests/test_pass_reach_cpu.py reads the macros and holds these to them): (bound on memories or degree, D, lanes T)
LT_DISPATCH = [(2, 2, 1), (4, 3, 1), (8, 5, 1), (16, 9, 2), (32, 17, 3)]
CUSTOM_DISPATCH = {False: [(2, 2, 1), (3, 3, 1), (5, 5, 1), (9, 9, 2), (17, 17, 3)], True: [(2, 2, 1), (3, 3, 1), (5, 5, 2), (7, 7, 2), (11, 11, 3), (17, 17, 5)]}
CLAIM_DISPATCH = [2, 4, 8, 16, 32]      # DISPATCH_A: k_combine_claim<A>


def lt_instance(alpha):
    a, d, t = next(x for x in LT_DISPATCH if alpha <= x[0])
    return a, d, t


def custom_instance(degree, multi):
    _, d, t = next(x for x in CUSTOM_DISPATCH[multi] if degree <= x[0])
    return d, t


# ---- caller-defined strategies over 4 memories (tests/customutil.py descriptors): one single-term list per lanes-per-index value, one multi-term list per value; -1, -2: p - 1, p - 2
CUSTOM_ALPHA = 4
CUSTOM_TERMS = {
    "single_t1": [(5, [0, 1, 2])],                                                                  # sumcheck degree 4: <5, 1, false>
    "single_t2": [(7, [0, 1, 2, 3, 0, 1, 2])],                                                      # 8: <9, 2, false>
    "single_t3": [(1, [0, 1, 2, 3] * 3)],                                                           # 13: <17, 3, false>; coefficient 1: no coefficient product
    "multi_t1": [(3, [0, 1]), (-1, [2]), (1, [3]), (9, [])],                                        # 3: <3, 1, true>; two single-factor terms in a row: a fold mark
    "multi_t2": [(2, [0, 1, 2, 3]), (1, [1, 1]), (5, [2])],                                         # 5: <5, 2, true>
    "multi_t3": [(3, [0, 1, 2, 3, 0, 1, 2, 3]), (1, [0, 3, 2]), (11, [1]), (4, [2])],               # 9: <11, 3, true>; a fold mark
    "multi_t5": [(1, [0, 1, 2, 3] * 3), (6, [3, 3, 1]), (-2, [0, 1])],                              # 13: <17, 5, true>
}


def custom_degree(name):
    """the sumcheck degree of a term list: g's degree + 1 (custom_strategy_degree + 1)"""
    return max(len(m) for _, m in CUSTOM_TERMS[name]) + 1


def sets_fold_mark(name):
    """pack_custom_terms' walk over the bound on |v| / p, restated: True where a term of the list gets flag 4 (the round kernel folds v behind it)"""
    terms = CUSTOM_TERMS[name]
    q = max(max(len(m) for _, m in terms), 1)
    budget, marked = 0, False
    for cf, mems in terms:
        ln = len(mems)
        unit = cf == 1 and ln == q and ln >= 2
        mag = 1 if ln == 0 else 19 if ln == 1 else (12 if unit else 4) if ln == 2 else 3 if ln == 3 else 2
        if budget + mag > 23:
            marked, budget = True, 2
        budget += mag
    return marked


# ---- the table

def _tag(env):
    return "default" if not env else "+".join(k.replace("LASSO_", "").lower() + "=" + v for k, v in sorted(env.items()))


U32_LINEAR = ("linear_eqw_round_u32", "linear_eqw_round_fused_from_u32")


def data_sets(entry):
    return ("uniform", "ones", "alternating") if entry == "combine_round_lt_u32" else ("uniform", "extreme")


def _rows(env, specs):
    out = []
    for entry, args, kernel, period, per_pass, claim, purpose in specs:
        name = "_".join(str(v) for v in args.values())
        for data in data_sets(entry):
            out.append(Row(f"{_tag(env)}:{entry}_{name}:{data}", env, entry, args, data, kernel, period, per_pass, claim, f"{purpose}, {data} data"))
    return out


def _linear_rows():
    specs = []
    for alpha in (1, 3):
        w = f"alpha = {alpha}"
        # 16 blocks of indices over 3 workgroups: 6, 5 and 5 passes
        specs += [("linear_eqw_round", {"n": 1 << 13, "alpha": alpha}, "k_dot_eqw_lb", 3, 256, "carry", f"k_dot_eqw_lb, {w}"),
                  ("linear_eqw_round_u32", {"n": 1 << 13, "alpha": alpha}, "k_dot_eqw_lb_u32", 3, 256, "carry", f"k_dot_eqw_lb_u32, {w}"),
                  ("linear_eqw_round_fused", {"n": 1 << 14, "alpha": alpha}, "k_dot_eqw_fused<false>", 3, 256, "carry", f"k_dot_eqw_fused<false> in place, {w}"),
                  ("linear_eqw_round_fused_from", {"n": 1 << 14, "alpha": alpha}, "k_dot_eqw_fused<false>", 3, 256, "carry", f"k_dot_eqw_fused<false> from other arrays, {w}"),
                  ("linear_eqw_round_fused_from_u32", {"n": 1 << 14, "alpha": alpha}, "k_dot_eqw_fused_from_u32", 3, 256, "carry", f"k_dot_eqw_fused_from_u32, {w}"),
                  ("linear_eqw_round_fused_ahead", {"n": 1 << 14, "alpha": alpha}, "k_dot_eqw_fused<true>", 3, 256, "carry", f"k_dot_eqw_fused<true> launched ahead, {w}")]
    # 512 blocks over 3 workgroups: 171, 171 and 170 passes — 57 carries in a row
    specs += [("linear_eqw_round", {"n": 1 << 18, "alpha": 1}, "k_dot_eqw_lb", 3, 256, "carry", "k_dot_eqw_lb, 171 passes"),
              ("linear_eqw_round_fused", {"n": 1 << 19, "alpha": 1}, "k_dot_eqw_fused<false>", 3, 256, "carry", "k_dot_eqw_fused<false>, 171 passes")]
    return specs


def _lt_n(t):
    """the smallest power of two n at which the longest of 3 workgroups makes more than 64 passes over n / 2 indices, 256 / t of them per pass: the 32-fold runs twice"""
    n = 4
    while -(-(-(-(n // 2) // (256 // t))) // 3) <= 64:
        n *= 2
    return n


def _lt_rows():
    specs = []
    for c in (1, 2, 4, 8, 16):
        a, d, t = lt_instance(2 * c)
        k = f"k_combine_round_lt<{a}, {d}, {t}>"
        specs.append(("combine_round", {"kind": "lt", "c": c, "n": _lt_n(t)}, k, 32, 256 // t, "fold+", f"{k} behind k_lt_prescale's copies"))
        specs.append(("combine_round_lt_scaled", {"kind": "lt", "c": c, "n": _lt_n(t)}, k, 32, 256 // t, "fold+", f"{k} on the caller's scaled arrays"))
    for c in (3, 8, 16):
        a, d, t = lt_instance(2 * c)
        k = f"k_combine_round_lt<{a}, {d}, {t}, PROD>"
        specs.append(("combine_round", {"kind": "spark", "c": c, "n": _lt_n(t)}, k, 32, 256 // t, "fold+", k))
    for c in (4, 8, 16):
        a, d, t = lt_instance(2 * c)
        k = f"k_combine_round_lt_u32<{a}, {d}, {t}>"
        specs.append(("combine_round_lt_u32", {"kind": "lt", "c": c, "n": _lt_n(t)}, k, 32, 256 // t, "fold+", k))
    return specs


def _custom_rows():
    specs = []
    for name in CUSTOM_TERMS:
        multi = len(CUSTOM_TERMS[name]) > 1
        d, t = custom_instance(custom_degree(name), multi)
        k = f"k_combine_round_custom<{d}, {t}, {'true' if multi else 'false'}>"
        specs.append(("combine_round", {"kind": "custom", "strategy": name, "n": _lt_n(t)}, k, 32, 256 // t, "fold+", k))
        specs.append(("combine_claim", {"kind": "custom", "strategy": name, "n": 1 << 17}, "k_combine_claim_custom", 128, 256, "fold+", f"k_combine_claim_custom over `{name}`"))
    return specs


TABLE = (
    # the 128-period folds of the three-sum cubic kernels: 2^17 index pairs or quadruples = 512 blocks over 3 workgroups, 171, 171 and 170 passes; the carries of the two-sum
    # forms at 6, 5 and 5 passes; the linear rounds
    _rows(CN3, [
        ("cubic_round", {"n": 1 << 18, "k": 1}, "k_cubic_round_lb", 128, 256, "fold+", "k_cubic_round_lb"),
        ("eqw_round", {"n": 1 << 18, "k": 1}, "k_cubic_eqw_lb<3>", 128, 256, "fold+", "k_cubic_eqw_lb<3>"),
        ("eqw_round_fused", {"n": 1 << 19, "k": 1}, "k_cubic_eqw_fused<3>", 128, 256, "fold+", "k_cubic_eqw_fused<3>"),
        ("eqw2_begin", {"n": 1 << 13, "k": 1}, "k_cubic_eqw_lb<2>", 3, 256, "carry", "k_cubic_eqw_lb<2>"),
        ("eqw2_begin_r", {"n": 1 << 14, "k": 1}, "k_cubic_eqw_fused<2, wide>", 3, 256, "carry", "k_cubic_eqw_fused<2, wide>")] + _linear_rows())
    # single-width accumulators in the two-sum fused round: CUBIC_ACCUMULATE2's fold
    + _rows(CN3_NARROW, [
        ("eqw2_begin_r", {"n": 1 << 19, "k": 2}, "k_cubic_eqw_fused<2, narrow>", 128, 256, "fold+", "k_cubic_eqw_fused<2, narrow>")])
    # the reduction launches outside the round grids, 3 workgroups each
    + _rows(RN3, [
        # 256 blocks: 86, 85 and 85 passes over a period of 64
        ("combine_round", {"kind": "and", "c": 2, "n": 1 << 17}, "k_combine_round_linear", 64, 256, "fold+", "k_combine_round_linear, AND's weights"),
        ("combine_round", {"kind": "range", "c": 3, "n": 1 << 17}, "k_combine_round_linear", 64, 256, "fold+", "k_combine_round_linear, the range check's weights")]
        + _lt_rows() + [
        # 512 blocks: 171, 171, 170 passes
        ("combine_claim", {"kind": "and", "c": 1, "n": 1 << 17}, "k_combine_claim<2>", 128, 256, "fold+", "k_combine_claim<2>, a weighted sum"),
        ("combine_claim", {"kind": "lt", "c": 16, "n": 1 << 17}, "k_combine_claim<32>", 128, 256, "fold+", "k_combine_claim<32>, LT's Horner walk"),
        ("combine_claim", {"kind": "range", "c": 4, "n": 1 << 17}, "k_combine_claim<4>", 128, 256, "fold+", "k_combine_claim<4>, the range check's weights")]
        + _custom_rows() + [
        ("inner_products_lr", {"nk": 1 << 18}, "k_inner_lr", 128, 256, "fold+", "k_inner_lr"),
        # 15 whole blocks and one of 17 elements: 6, 5 and 5 passes
        ("multi_dot", {"k": 2, "n": 3 * 256 * 5 + 17}, "k_multi_dot", 3, 256, "carry", "k_multi_dot, a partly filled last block")])
    # the second stage over more than 256 partials per row, at the launches' own caps; the row chunks of the mat-vec
    + _rows(DEFAULT, [
        ("combine_round", {"kind": "and", "c": 1, "n": 1 << 18}, "reduce_partials_row", 256, 256, "stage2 2", "the second stage over 512 partials of 3 values"),
        ("combine_round", {"kind": "and", "c": 1, "n": 1 << 19}, "reduce_partials_row", 256, 256, "stage2 4", "the second stage over 1024 partials of 3 values"),
        ("combine_claim", {"kind": "and", "c": 1, "n": 1 << 18}, "reduce_partials_row", 256, 256, "stage2 4", "the second stage over 1024 partials of one value"),
        # 2561 blocks over 512 workgroups: 6 passes for the first, 5 for the others
        ("multi_dot", {"k": 1, "n": 5 * (1 << 17) + 7}, "k_multi_dot", 3, 256, "carry", "k_multi_dot at its own cap, and its second stage over 512 partials"),
        # 16 column blocks, 64 chunks of 7 rows, the last of 6
        ("matvec_left", {"l": 447, "r": 4096}, "k_matvec_left", 3, 1, "carry", "k_matvec_left, the result to the host"),
        ("matvec_left_dev", {"l": 447, "r": 4096}, "k_matvec_left", 3, 1, "carry", "k_matvec_left, the result on the device"),
        # 4 column blocks, 200 chunks of 2 rows: k_matvec_reduce adds 200 partials per column
        ("matvec_left", {"l": 400, "r": 1024}, "k_matvec_reduce", 128, 1, "fold+", "k_matvec_reduce, the result to the host"),
        ("matvec_left_dev", {"l": 400, "r": 1024}, "k_matvec_reduce", 128, 1, "fold+", "k_matvec_reduce, the result on the device")])
)
ENVS = []
for _r in TABLE:
    if _r.env not in ENVS:
        ENVS.append(_r.env)
assert len({r.id for r in TABLE}) == len(TABLE)

# every kernel and instantiation that keeps a lazily reduced running sum: each must have a `fold+` or `carry` row (the lanes-per-index kernels once per T)
REQUIRED_KERNELS = (
    # the carry after every 3rd product
    "k_dot_eqw_lb", "k_dot_eqw_lb_u32", "k_dot_eqw_fused<false>", "k_dot_eqw_fused<true>", "k_dot_eqw_fused_from_u32", "k_multi_dot", "k_matvec_left", "k_cubic_eqw_lb<2>",
    "k_cubic_eqw_fused<2, wide>",
    # fr29_mul(acc, one_s) every 128 additions
    "k_cubic_round_lb", "k_cubic_eqw_lb<3>", "k_cubic_eqw_fused<3>", "k_cubic_eqw_fused<2, narrow>", "k_combine_claim<2>", "k_combine_claim<4>", "k_combine_claim<32>",
    "k_combine_claim_custom", "k_matvec_reduce", "k_inner_lr",
    # every 64
    "k_combine_round_linear",
    # every LT_FOLD_EVERY() indices
    "k_combine_round_lt<2, 2, 1>", "k_combine_round_lt<4, 3, 1>", "k_combine_round_lt<8, 5, 1>", "k_combine_round_lt<16, 9, 2>", "k_combine_round_lt<32, 17, 3>", "k_combine_round_lt<8, 5, 1, PROD>", "k_combine_round_lt<16, 9, 2, PROD>",
    "k_combine_round_lt<32, 17, 3, PROD>", "k_combine_round_lt_u32<8, 5, 1>", "k_combine_round_lt_u32<16, 9, 2>", "k_combine_round_lt_u32<32, 17, 3>",
    "k_combine_round_custom<5, 1, false>", "k_combine_round_custom<9, 2, false>", "k_combine_round_custom<17, 3, false>", "k_combine_round_custom<3, 1, true>",
    "k_combine_round_custom<5, 2, true>", "k_combine_round_custom<11, 3, true>", "k_combine_round_custom<17, 5, true>")


def rows_of(env):
    return [r for r in TABLE if r.env == env]


# ---- the grid of a row's launch (CPU)

_PLAN_EXE = {}


def plan_program(curve):
    """tests/cpp/pass_plan_dump.cpp built for `curve` into tests/_build/"""
    if curve not in _PLAN_EXE:
        out_dir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(out_dir, exist_ok=True)
        exe = os.path.join(out_dir, "pass_plan_dump" + ("_bn254" if curve == "bn254" else ""))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", *(["-DLASSO_BN254"] if curve == "bn254" else []), "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", "pass_plan_dump.cpp")])
        _PLAN_EXE[curve] = exe
    return _PLAN_EXE[curve]


# the caps the reduction launches pass to reduce_nx (lasso_hip.hip; tests/test_pass_reach_cpu.py reads them there)
REDUCE_CAPS = {"combine_round": 1024, "combine_round_lt_scaled": 1024, "combine_round_lt_u32": 1024, "combine_claim": 1024, "multi_dot": 512, "inner_products_lr": 256}
CUBIC_ENTRIES = ("eqw_round", "eqw_round_fused", "eqw2_begin", "eqw2_begin_r")


def launch_of(row):
    """the line of pass_plan_dump's input that asks for the row's grid"""
    a = row.args
    if row.entry in CUBIC_ENTRIES:
        return f"{row.entry} {a['n']} {a['k']} 0"
    if row.entry == "cubic_round":
        return f"round {a['n'] // 2} {a['k']} 0"
    if row.entry.startswith("linear_"):
        return f"round {a['n'] // (4 if 'fused' in row.entry else 2)} {a['alpha']} 0"
    if row.entry in ("matvec_left", "matvec_left_dev"):
        return f"matvec {a['l']} {a['r']} 0"
    items = a["nk"] // 2 if row.entry == "inner_products_lr" else a["n"] if row.entry in ("combine_claim", "multi_dot") else a["n"] // 2
    return f"reduce {items} {REDUCE_CAPS[row.entry]} 0"


def plans(env, rows, curve):
    """one run of the plan program under `env` (a fresh process: the switches are read once) -> {row id: what it printed}"""
    lines = [f"{r.id.replace(' ', '')} {launch_of(r)}" for r in rows]
    e = {k: v for k, v in os.environ.items() if not k.startswith("LASSO_")}
    e.update(env)
    res = subprocess.run([plan_program(curve)], input="\n".join(lines) + "\n", env=e, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    out = {}
    for ln in res.stdout.splitlines():
        p = json.loads(ln)
        out[p["id"]] = p
    assert set(out) == {r.id for r in rows}
    return out


def passes_of(row, plan):
    """passes of its loop the first thread of every workgroup along x makes (of every column thread, for the mat-vec kernels): workgroup x of nx takes
    ceil((blocks - x) / nx) of the launch's blocks of `per_pass` items"""
    if plan["kind"] == "matvec":
        l, rpc, chunks = row.args["l"], plan["rows_per_chunk"], plan["nchunks"]
        return [chunks] if row.kernel == "k_matvec_reduce" else [min(rpc, l - c * rpc) for c in range(chunks)]
    blocks = -(-plan["items"] // row.per_pass)
    return [max(-(-(blocks - x) // plan["nx"]), 0) for x in range(plan["nx"])]


def claim_failure(row, plan):
    """None where the row's claim holds for the planned grid, else why not"""
    ps = passes_of(row, plan)
    if row.claim == "fold+":
        if not any(p > row.period and p % row.period for p in ps):
            return f"no thread makes more than {row.period} passes with accumulation behind the last fold (passes per workgroup: {sorted(set(ps))})"
    elif row.claim == "carry":
        if row.period != 3 or not (any(p >= 4 and p % 3 == 0 for p in ps) and any(p >= 4 and p % 3 for p in ps)):
            return f"remainders 0 and non-zero of the 3-product carry do not both occur at 4 or more passes (passes per workgroup: {sorted(set(ps))})"
    else:
        k = int(row.claim.split()[1])
        if not (row.claim.startswith("stage2 ") and plan["nx"] > 256 and -(-plan["nx"] // 256) == k):
            return f"the second stage sums {plan['nx']} partials per row, not {k} passes of 256"
    return None


# ---- inputs (a function of the row alone: the mock and the device get the same)

_POOL = {}


def _pool(data):
    """5 * 2^17 + 2^13 + 5 field elements per data set, made once per process; an array of a row is a window into it"""
    if data not in _POOL:
        from fieldref import L as FR_P, limbs
        from gpuutil import EDGE, lift, words
        m = 5 * (1 << 17) + (1 << 13) + 5
        if data == "uniform":      # gpuutil.full_fr's rejection sampling over 254 bits, on whole arrays
            rng = np.random.default_rng(20240)
            pw = [np.uint64(w) for w in limbs(FR_P)]
            got = []
            while sum(len(g) for g in got) < m:
                a = rng.integers(0, 2**64, size=(2 * m, 4), dtype=np.uint64)
                a[:, 3] &= np.uint64(2**62 - 1)
                below, equal = np.zeros(len(a), dtype=bool), np.ones(len(a), dtype=bool)
                for k in (3, 2, 1, 0):
                    below |= equal & (a[:, k] < pw[k])
                    equal &= a[:, k] == pw[k]
                got.append(a[below])
            _POOL[data] = np.concatenate(got)[:m]
        else:
            low = 2**232 - 1               # gpuutil._edge_words: limbs 0..7 all 2^29 - 1, limb 8 as large as p allows
            edge = low + ((FR_P - 1 - low) >> 232 << 232)
            assert edge in EDGE
            three = lift(words([FR_P - 1, (FR_P - 1) // 2, edge]))      # the largest representative of each below LAZY_BOUND
            _POOL[data] = np.tile(three, (m // 3 + 1, 1))[:m]
    return _POOL[data]


def field_arrays(row, count, n, salt=0, reduced=False):
    """`count` arrays of n field elements of the row's data set: windows at different offsets (different phases of the extreme cycle).  reduced: the canonical representatives
    of the same residues (what the mock is given)"""
    pool = _pool("uniform" if row.data == "uniform" else "extreme")
    if reduced and row.data != "uniform":
        if "reduced" not in _POOL:
            _POOL["reduced"] = canonical(pool)
        pool = _POOL["reduced"]
    assert n + 97 * (count + salt) <= len(pool)
    return [pool[97 * (j + salt): 97 * (j + salt) + n] for j in range(count)]


def scalars(count, salt):
    from gpuutil import rand_fr
    return rand_fr(np.random.default_rng([77, salt]), count, edge=False)


def u32_arrays(row, count, n):
    if row.entry in U32_LINEAR:
        if row.data == "extreme":
            return [np.full(n, 2**32 - 1, dtype=np.uint32) for _ in range(count)]
        rng = np.random.default_rng([n, count, 32])
        return [rng.integers(0, 2**32, size=n, dtype=np.uint32) for _ in range(count)]
    if row.data == "uniform":
        rng = np.random.default_rng([n, count, 1])
        return [rng.integers(0, 2, size=n, dtype=np.uint32) for _ in range(count)]
    if row.data == "ones":         # lines 0 -> 1 everywhere
        return [np.concatenate([np.zeros(n // 2, dtype=np.uint32), np.ones(n // 2, dtype=np.uint32)]) for _ in range(count)]
    return [np.concatenate([np.full(n // 2, (m + 1) & 1, dtype=np.uint32), np.full(n // 2, m & 1, dtype=np.uint32)]) for m in range(count)]


def strategy_of(row):
    from fieldref import CURVE
    from lasso_amd import CustomStrategy, _abi
    a = row.args
    if a["kind"] == "custom":
        from lasso_amd.custom import FR_MODULUS
        p = FR_MODULUS[CURVE]
        terms = [(cf % p, mems) for cf, mems in CUSTOM_TERMS[a["strategy"]]]
        cs = CustomStrategy(CUSTOM_ALPHA, 2, [np.zeros(4, dtype=np.uint32)], terms, num_memories=CUSTOM_ALPHA, memory_subtable=[0] * CUSTOM_ALPHA,
                            memory_dimension=list(range(CUSTOM_ALPHA)), curve=CURVE)
        return cs, CUSTOM_ALPHA, cs.degree
    log_m, log_r = {"and": (16, 0), "range": (8 if a["c"] == 3 else 16, 40), "lt": (4, 0), "spark": (4, 0)}[a["kind"]]
    alpha = 2 * a["c"] if a["kind"] == "lt" else a["c"]
    return _abi.Strategy(_abi.KINDS[a["kind"]], a["c"], log_m, log_r), alpha, a["c"] + 1 if a["kind"] in ("lt", "spark") else 2


# ---- runs

LAZY = ("bound", "A", "B")      # arrays a round has bound: the device keeps lazily reduced representatives, compared as residues


def run_row(d, row, reduced=False):
    """the row's call on Device `d` -> {name: (.., 4) uint64 array}.  reduced: every field array replaced by the canonical representatives of the same residues — how the mock
    gets the `extreme` rows: its field type adds without reducing a sum above 2^256, so a line through two maximal representatives (4 p on curve25519) stepped to the evaluation
    point 5 wraps there (seen against big-integer arithmetic); on canonical inputs it is exact, and the expected bytes are a function of the residues alone"""
    a, lib, ctx = row.args, d.lib, d.ctx
    held = []

    def arrays(count, n, salt=0):
        return field_arrays(row, count, n, salt, reduced)

    def up(arrays):
        ps = [d.upload(x) for x in arrays]
        held.extend(ps)
        return ps

    def fresh(count, m):
        ps = [d.alloc(32 * m) for _ in range(count)]
        held.extend(ps)
        return ps
    try:
        if row.entry in ("cubic_round",) + CUBIC_ENTRIES:
            n, k = a["n"], a["k"]
            X = arrays(2 * k + 1, n)
            pa, pb = up(X[:k]), up(X[k:2 * k])
            bound = lambda: {"A": np.stack([d.download(p, (n // 2, 4)) for p in pa]), "B": np.stack([d.download(p, (n // 2, 4)) for p in pb])}
            r1 = scalars(1, n)[0]
            if row.entry == "cubic_round":
                return {"sums": d.sumcheck_cubic_round(pa, pb, up([X[2 * k]])[0], n)}
            if row.entry == "eqw_round":
                return {"sums": d.sumcheck_cubic_eqw_round(pa, pb, up([X[2 * k][:n // 2]])[0], n)}
            if row.entry == "eqw_round_fused":
                return {"sums": d.sumcheck_cubic_eqw_round_fused(pa, pb, up([X[2 * k][:n // 4]])[0], n, r1), **bound()}
            if row.entry == "eqw2_begin":
                return {"sums": d.sumcheck_cubic_eqw2(pa, pb, up([X[2 * k][:n // 2]])[0], n)}
            return {"sums": d.sumcheck_cubic_eqw2(pa, pb, up([X[2 * k][:n // 4]])[0], n, r1), **bound()}
        if row.entry.startswith("linear_"):
            n, alpha = a["n"], a["alpha"]
            pe = up([arrays(1, n // 2, salt=40)[0]])[0]
            r1 = scalars(1, n + alpha)[0]
            down = lambda ps: np.stack([d.download(p, (n // 2, 4)) for p in ps])
            if row.entry in U32_LINEAR:
                pu = up(u32_arrays(row, alpha, n))
                if row.entry == "linear_eqw_round_u32":
                    return {"sums": d.sumcheck_linear_eqw_round_u32(pu, pe, n)}
                pd = fresh(alpha, n // 2)
                return {"sums": d.sumcheck_linear_eqw_round_fused_from_u32(pu, pd, pe, n, r1), "bound": down(pd)}
            pp = up(arrays(alpha, n))
            if row.entry == "linear_eqw_round":
                return {"sums": d.sumcheck_linear_eqw_round(pp, pe, n)}
            if row.entry == "linear_eqw_round_fused":
                return {"sums": d.sumcheck_linear_eqw_round_fused(pp, pe, n, r1), "bound": down(pp)}
            if row.entry == "linear_eqw_round_fused_from":
                pd = fresh(alpha, n // 2)
                sums, src = d.sumcheck_linear_eqw_round_fused_from(pp, pd, pe, n, r1), arrays(alpha, n)
                assert all(np.array_equal(d.download(p, (n, 4)), x) for p, x in zip(pp, src)), "the round wrote to its source arrays"
                return {"sums": sums, "bound": down(pd)}
            assert row.entry == "linear_eqw_round_fused_ahead"
            # the prover's schedule: the round enqueued without its challenge, the challenge posted, the result collected
            d._chk(lib.lasso_sumcheck_linear_eqw_round_fused_ahead(ctx, d._ptrs(pp), alpha, C.c_void_p(pe), n))
            d._chk(lib.lasso_challenge_post(ctx, _vp(r1)))
            return {"sums": _wait(d, 3 * alpha).reshape(alpha, 3, 4)[:, :2].copy(), "bound": down(pp)}
        if row.entry in ("combine_round", "combine_round_lt_scaled", "combine_round_lt_u32", "combine_claim"):
            n = a["n"]
            S, alpha, degree = strategy_of(row)
            pe = up([arrays(1, n, salt=40)[0]])[0]
            if row.entry == "combine_round_lt_u32":
                return {"evals": d.sumcheck_combine_round_lt_u32(S, up(u32_arrays(row, alpha, n)), pe, n, degree)}
            pp = up(arrays(alpha, n))
            if row.entry == "combine_claim":
                return {"claim": d.combine_claim(S, pp, pe, n)}
            if row.entry == "combine_round_lt_scaled":
                return {"evals": d.sumcheck_combine_round_lt_scaled(S, pp, pe, n, degree)}
            return {"evals": d.sumcheck_combine_round(S, pp, pe, n, degree)}
        if row.entry == "inner_products_lr":
            pa, pb = up(arrays(2, a["nk"]))
            return {"lr": d.inner_products_lr(pa, pb, a["nk"])}
        if row.entry == "multi_dot":
            X = arrays(a["k"] + 1, a["n"])
            return {"dots": d.multi_dot(up(X[:-1]), up(X[-1:])[0], a["n"])}
        assert row.entry in ("matvec_left", "matvec_left_dev")
        l, r = a["l"], a["r"]
        pool = arrays(1, len(_pool("uniform")) - 97)[0]
        Z = np.concatenate([pool] * (l * r // len(pool) + 1))[:l * r]      # l r elements: the pool over and over (its length is no multiple of r)
        Lv = arrays(1, l, salt=7)[0]
        pz = up([Z])[0]
        if row.entry == "matvec_left":
            return {"LZ": d.matvec_left(pz, Lv, l, r)}
        pl, po = up([Lv])[0], fresh(1, r)[0]
        d.matvec_left_dev(pz, pl, l, r, po)
        return {"LZ": d.download(po, (r, 4))}
    finally:
        for p in held:
            d.free(p)


def canonical(arr):
    """the canonical representative of every element, on whole arrays: p subtracted from the elements at or above it until none is"""
    from fieldref import L as FR_P, limbs
    a = np.ascontiguousarray(arr, dtype=np.uint64).reshape(-1, 4).copy()
    pw = [np.uint64(w) for w in limbs(FR_P)]
    while True:
        below, equal = np.zeros(len(a), dtype=bool), np.ones(len(a), dtype=bool)
        for k in (3, 2, 1, 0):
            below |= equal & (a[:, k] < pw[k])
            equal &= a[:, k] == pw[k]
        ge = ~below
        if not ge.any():
            return a.reshape(np.shape(arr))
        x = a[ge]
        borrow = np.zeros(len(x), dtype=bool)
        for k in range(4):
            nb = (x[:, k] < pw[k]) | ((x[:, k] == pw[k]) & borrow)
            x[:, k] = x[:, k] - pw[k] - borrow.astype(np.uint64)
            borrow = nb
        a[ge] = x


def printable(out):
    """{name: text}: the bytes of every output as hex — residues for the arrays a round has bound, and the SHA-256 of the bytes for arrays above 4 KiB"""
    res = {}
    for name, arr in out.items():
        raw = np.ascontiguousarray(canonical(arr) if name in LAZY else arr, dtype=np.uint64).tobytes()
        res[name] = raw.hex() if len(raw) <= 4096 else "sha256:" + hashlib.sha256(raw).hexdigest()
    return res


def mock_for(row):
    """the library that serves as the row's reference: the oracle's mock; for a caller-defined strategy the mock behind tests/cpp/mock_custom_wrap.cpp"""
    from fieldref import CURVE
    if row.args.get("kind") == "custom":
        import customutil
        from lasso_amd import _abi
        if "custom" not in _MOCKS:
            lib = C.CDLL(customutil.build_mock_prover_custom(CURVE))
            _abi.declare(lib)
            _MOCKS["custom"] = lib
        return _MOCKS["custom"]
    if "mock" not in _MOCKS:
        from gpuutil import load_mock
        _MOCKS["mock"] = load_mock()
    return _MOCKS["mock"]


_MOCKS = {}


def reference_key(row):
    """rows that must give the same bytes: the same call on the same inputs, whatever the switches"""
    return (row.entry, tuple(row.args.items()), row.data)


def child_main(index):
    """run the rows of ENVS[index] on the device (the environment is the parent's business) and print `ROW <id> <name> <hex>` per output"""
    sys.path.insert(0, ROOT)
    from fieldref import CURVE
    from lasso_amd import Device
    d = Device(0, curve=CURVE)
    for row in rows_of(ENVS[index]):
        for name, text in printable(run_row(d, row)).items():
            print("ROW", row.id.replace(" ", ""), name, text, flush=True)
    d.close()
    print("DONE", len(rows_of(ENVS[index])))


if __name__ == "__main__":
    child_main(int(sys.argv[1]))
