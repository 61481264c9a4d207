"""The eq-weighted cubic-round kernels a switch or a shape selects (lasso_amd/csrc/launch_plan.cuh cubic_plan, launched by cubic_eqw_launch_t of lasso_hip.hip), as ONE table of
calls: switch setting, entry point, shape, and the plan the call must be given.  Three users:

  tests/test_round_reach_cpu.py    holds every row to the plan tests/cpp/cubic_plan_dump.cpp prints for it (the real plan function over the real switch table, one child process per
                                   setting), and the union of the rows to every kernel instantiation and loop shape listed there — without a GPU;
  tests/test_gpu_round_variants.py runs every row on the device, one child process per setting, against the oracle's mock;
  tests/test_gpu_kernels.py        imports the shape lists of its six cubic-round tests from here, where the forms their comments name are checked facts.

Run as a program (`python tests/roundvariants.py <index into ENVS>`) it is that child process: it runs the setting's rows on the device and prints every output as hex.
The curve is fieldref.CURVE (LASSO_TEST_CURVE), as for tests/gpuutil.py."""
import ctypes as C
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the shape lists of tests/test_gpu_kernels.py (default switches); tests/test_round_reach_cpu.py holds each to the form the comment beside it names

# test_sumcheck_cubic_eqw_round: (n, circuits).  n <= 128: the latency-shaped kernel (k_cubic_eqw_small), above it the evaluation-only round (k_cubic_eqw_lb<3>)
CUBIC_EQW_ROUND_SHAPES = [(2, 1), (4, 2), (16, 33), (128, 5), (256, 2), (1 << 9, 2), (1 << 13, 8), (1 << 16, 3)]
# test_sumcheck_cubic_eqw_round_fused: a challenge is bound first, n / 4 indices per circuit.  n <= 256: the latency-shaped kernel, above it k_cubic_eqw_fused<3>
CUBIC_EQW_ROUND_FUSED_SHAPES = [(4, 1), (8, 2), (32, 33), (256, 5), (512, 2), (1 << 10, 2), (1 << 14, 8), (1 << 17, 3)]
# test_sumcheck_cubic_eqw2: both of the above in the two-sum form (n = 2 without the bind only)
CUBIC_EQW2_SHAPES = [(2, 1), (4, 1), (8, 2), (32, 33), (256, 5), (512, 2), (1 << 10, 2), (1 << 14, 8), (1 << 17, 3)]
# test_cubic_round_launched_ahead: rounds of n and n / 2 launched ahead (k_cubic_eqw_fused<2, .., AHEAD>), one of n / 4 abandoned; n / 8 <= 64: the refusal
CUBIC_ROUND_AHEAD_SHAPES = [(512, 2), (1 << 12, 2), (1 << 12, 8), (1 << 16, 2), (1 << 18, 3), (1 << 20, 2), (1 << 13, 16)]
# test_sumcheck_cubic_round0_with_inline_eq_table: (n, circuits, scaled).  Tables of up to 2^14 entries are built in LDS (EqInline); above 2^14 entries: factor tables in memory,
# their product by k_eq_outer in front of the round, or inside it under LASSO_EQ_INLINE_BIG=1 (EqGlobal)
CUBIC_ROUND0_EQ_SHAPES = [(256, 2, False), (512, 3, True), (1 << 12, 2, False), (1 << 14, 2, True), (1 << 15, 5, False), (1 << 15, 16, True),
                          (1 << 16, 2, True), (1 << 18, 3, False), (1 << 20, 1, True), (1 << 17, 9, False)]
# test_layer_enqueued_ahead_of_its_point: (n2, circuits, m_stop2, mode).  Tables of up to 2^9 entries: the resident tail serves the layer (no cubic_plan); above: round 0 behind
# the point gate (EqInlineMem up to 2^14 entries, factor tables by k_eq_small2_mem above)
LAYER_AHEAD_SHAPES = [(1 << 12, 2, 1, "post"), (1 << 15, 3, 1, "post"), (1 << 17, 2, 1, "post"), (1 << 18, 9, 1, "post"), (512, 2, 4, "post"), (1024, 2, 1, "post"),
                      (64, 9, 2, "post"), (1 << 13, 2, 1, "cancel"), (1 << 17, 2, 1, "cancel"), (512, 2, 8, "cancel")]

# ---- the table

Row = namedtuple("Row", "id env entry shape expect")
# shape: length of every array, circuits, the context's profiling mask during the call.  The eq point of the two *_eq entries has log2(n / 2) coordinates.
Shape = namedtuple("Shape", "n ncirc prof")
ENTRIES = ("eqw_round", "eqw_round_fused", "eqw2_begin", "eqw2_begin_r", "eqw2_begin_ahead", "eqw2_begin_eq", "eqw2_begin_eq_ahead")
PROF_CUBIC = 1 << 1      # include/lasso_hip.h: bit LASSO_K_CUBIC of lasso_prof_enable's mask
REFUSAL_AHEAD = "a round launched ahead of its challenge: two-sum streaming rounds only (more than 64 index quadruples per circuit)"


def ell_of(shape):
    return (shape.n // 2).bit_length() - 1


def _rows(env, entries):
    tag = "default" if not env else "+".join(k.replace("LASSO_", "").lower() + "=" + v for k, v in sorted(env.items()))
    return [Row(f"{tag}:{entry}_{n}x{k}" + ("_prof" if prof else ""), env, entry, Shape(n, k, prof), expect) for entry, (n, k, *p), expect in entries for prof in [p[0] if p else 0]]


def _small(bind, items, table):
    return {"form": "SMALL", "bind": bind, "items": items, "ptr_table": table}


def _fused(nt, items, nx, direct, wide, table="8", **more):
    return {"form": "FUSED", "NT": nt, "items": items, "nx": nx, "direct": direct, "wide": wide, "gate": False, "inkernel": False, "ptr_table": table, **more}


def _ahead(items, nx, direct, wide, wait, table="8"):
    """a two-sum fused round launched ahead; wait: where it waits for its challenge, "gate" (k_gate in front) or "inkernel" """
    return {"form": "FUSED", "NT": 2, "items": items, "nx": nx, "direct": direct, "wide": wide, "gate": wait == "gate", "inkernel": wait == "inkernel", "ptr_table": table}


def _lb(nt_sums, items, nx, direct, eq, table="8", pipe=1, nt=False, gate=False, eq_outer=False, **more):
    return {"form": "LB", "NT": nt_sums, "items": items, "nx": nx, "direct": direct, "ptr_table": table, "lb.eq": eq, "lb.pipe": pipe, "lb.nt": nt, "lb.gate": gate,
            "lb.eq_outer": eq_outer, **{"lb." + k: v for k, v in more.items()}}


def _outer(items, nx, g_hi, g_lo, gated, table="8", direct=False, pipe=1):
    """round 0 of a table above 2^14 entries under the default switches: factor tables by k_eq_small2 (gated: k_eq_small2_mem), their product by k_eq_outer, the round reads d_E"""
    return _lb(2, items, nx, direct, "TABLE", table, pipe=pipe, gate=gated, eq_outer=True, factors=True, factors_gated=gated, g_hi=g_hi, g_lo=g_lo)


def _factors(items, nx, g_hi, g_lo, gated, table="8"):
    """the same under LASSO_EQ_INLINE_BIG=1: the product inside the round (EqGlobal)"""
    return _lb(2, items, nx, False, "FACTORS", table, gate=gated, eq_outer=False, factors=True, factors_gated=gated, g_hi=g_hi, g_lo=g_lo)


TABLE = (
    _rows({}, [
        # k_cubic_eqw_small<BIND, NT, TM>: every instantiation once, 64 indices per circuit (the last size it serves) and one, both pointer tables
        ("eqw_round", (128, 2), _small(False, 64, "8")), ("eqw_round", (2, 9), _small(False, 1, "full")),
        ("eqw2_begin", (128, 33), _small(False, 64, "full")), ("eqw2_begin", (16, 2), _small(False, 8, "8")),
        ("eqw_round_fused", (256, 8), _small(True, 64, "8")), ("eqw_round_fused", (4, 9), _small(True, 1, "full")),
        ("eqw2_begin_r", (256, 9), _small(True, 64, "full")), ("eqw2_begin_r", (4, 1), _small(True, 1, "8")),
        # k_cubic_eqw_fused, the challenge an argument: three sums; two sums over double-width accumulators.  128 indices: one workgroup, half of it idle; 16 workgroups per circuit:
        # the last grid whose block sums go out direct; 32: the in-launch second stage
        ("eqw_round_fused", (512, 2), _fused(3, 128, 1, False, False)), ("eqw_round_fused", (1 << 12, 9), _fused(3, 1024, 4, True, False, "full")),
        ("eqw2_begin_r", (512, 1), _fused(2, 128, 1, False, True)), ("eqw2_begin_r", (1 << 11, 33), _fused(2, 512, 2, True, True, "full")),
        ("eqw2_begin_r", (1 << 14, 2), _fused(2, 4096, 16, True, True)), ("eqw2_begin_r", (1 << 15, 2), _fused(2, 8192, 32, False, True)),
        # ... launched ahead: 16 x 2 = 32 workgroups wait inside the round's kernel (LASSO_AHEAD_INKERNEL_WGS' default), 1 x 33 and 32 x 2 behind k_gate; profiling the family moves
        # the wait into the gate whatever the size; 64 quadruples per circuit: refused
        ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, True, True, "inkernel")), ("eqw2_begin_ahead", (1 << 10, 33), _ahead(256, 1, False, True, "gate", "full")),
        ("eqw2_begin_ahead", (1 << 15, 2), _ahead(8192, 32, False, True, "gate")),
        ("eqw2_begin_ahead", (1 << 14, 2, PROF_CUBIC), _ahead(4096, 16, True, True, "gate")),
        ("eqw2_begin_ahead", (256, 2), {"form": "REFUSED", "refusal": REFUSAL_AHEAD}),
        # k_cubic_eqw_lb: three sums; two sums from the table in memory (EqNone), a grid at its cap of 64 with two passes per workgroup; the table built in LDS from the point in the
        # arguments (EqInline) at 7, 11 and 14 coordinates; from the gated point (EqInlineMem); above 2^14 entries k_eq_small2 / k_eq_small2_mem and k_eq_outer in front (15
        # coordinates: factor tables of 2^8 and 2^7 entries; 16: both 2^8)
        ("eqw_round", (512, 2), _lb(3, 256, 1, False, "TABLE", pipe=0)), ("eqw_round", (1 << 13, 9), _lb(3, 4096, 16, True, "TABLE", "full", pipe=0)),
        ("eqw2_begin", (1 << 13, 2), _lb(2, 4096, 16, True, "TABLE")), ("eqw2_begin", (1 << 16, 9), _lb(2, 1 << 15, 64, False, "TABLE", "full")),
        ("eqw2_begin_eq", (256, 2), _lb(2, 128, 1, False, "LDS")), ("eqw2_begin_eq", (1 << 12, 9), _lb(2, 2048, 8, True, "LDS", "full")),
        ("eqw2_begin_eq", (1 << 15, 2), _lb(2, 1 << 14, 64, False, "LDS")),
        ("eqw2_begin_eq_ahead", (1 << 12, 2), _lb(2, 2048, 8, True, "GATED", gate=True)), ("eqw2_begin_eq_ahead", (256, 9), _lb(2, 128, 1, False, "GATED", "full", gate=True)),
        ("eqw2_begin_eq_ahead", (1 << 15, 3), _lb(2, 1 << 14, 64, False, "GATED", gate=True)),
        ("eqw2_begin_eq", (1 << 16, 2), _outer(1 << 15, 128, 8, 7, False)), ("eqw2_begin_eq", (1 << 17, 1), _outer(1 << 16, 256, 8, 8, False)),
        ("eqw2_begin_eq", (1 << 16, 9), _outer(1 << 15, 64, 8, 7, False, "full")),
        ("eqw2_begin_eq_ahead", (1 << 16, 3), _outer(1 << 15, 128, 8, 7, True)), ("eqw2_begin_eq_ahead", (1 << 17, 2), _outer(1 << 16, 256, 8, 8, True))])
    # k_cubic_eqw_fused<2, false, ..>: single-width accumulators, reduced every 128 terms (CUBIC_ACCUMULATE2) — with the challenge and launched ahead, waiting both ways
    + _rows({"LASSO_CUBIC_WIDE": "0"}, [
        ("eqw2_begin_r", (512, 1), _fused(2, 128, 1, False, False)), ("eqw2_begin_r", (1 << 11, 33), _fused(2, 512, 2, True, False, "full")),
        ("eqw2_begin_r", (1 << 15, 2), _fused(2, 8192, 32, False, False)),
        ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, True, False, "inkernel")), ("eqw2_begin_ahead", (1 << 10, 33), _ahead(256, 1, False, False, "gate", "full"))])
    # k_cubic_eqw_lb<2, false, TP, EqNone, true>: the non-temporal loads — only where the round reads its table and nothing ran in front of it; the round 0 in front of the round
    # launched ahead is one more of them
    + _rows({"LASSO_LB_NT": "1"}, [
        ("eqw2_begin", (256, 1), _lb(2, 128, 1, False, "TABLE", nt=True)), ("eqw2_begin", (1 << 13, 2), _lb(2, 4096, 16, True, "TABLE", nt=True)),
        ("eqw2_begin", (1 << 16, 9), _lb(2, 1 << 15, 64, False, "TABLE", "full", nt=True)),
        ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, True, True, "inkernel")),
        ("eqw_round", (1 << 13, 2), _lb(3, 4096, 16, True, "TABLE", pipe=0)), ("eqw2_begin_eq", (1 << 12, 2), _lb(2, 2048, 8, True, "LDS")),
        ("eqw2_begin_eq", (1 << 16, 2), _outer(1 << 15, 128, 8, 7, False))])
    # the plain loop of the evaluation-only round: wherever it reads its table, behind k_eq_outer too; the rounds that build their table stay pipelined
    + _rows({"LASSO_LB_PIPELINE": "0"}, [
        ("eqw2_begin", (256, 1), _lb(2, 128, 1, False, "TABLE", pipe=0)), ("eqw2_begin", (1 << 13, 2), _lb(2, 4096, 16, True, "TABLE", pipe=0)),
        ("eqw2_begin", (1 << 16, 9), _lb(2, 1 << 15, 64, False, "TABLE", "full", pipe=0)),
        ("eqw2_begin_eq", (1 << 12, 2), _lb(2, 2048, 8, True, "LDS")), ("eqw2_begin_eq", (1 << 16, 2), _outer(1 << 15, 128, 8, 7, False, pipe=0)),
        ("eqw2_begin_eq_ahead", (1 << 16, 3), _outer(1 << 15, 128, 8, 7, True, pipe=0))])
    # the non-temporal form exists only pipelined
    + _rows({"LASSO_LB_NT": "1", "LASSO_LB_PIPELINE": "0"}, [
        ("eqw2_begin", (256, 1), _lb(2, 128, 1, False, "TABLE", pipe=0)), ("eqw2_begin", (1 << 13, 2), _lb(2, 4096, 16, True, "TABLE", pipe=0))])
    # EqGlobal: the product of the factor tables inside round 0, ungated and behind the point gate; up to 2^14 entries nothing changes
    + _rows({"LASSO_EQ_INLINE_BIG": "1"}, [
        ("eqw2_begin_eq", (1 << 16, 2), _factors(1 << 15, 128, 8, 7, False)), ("eqw2_begin_eq", (1 << 17, 1), _factors(1 << 16, 256, 8, 8, False)),
        ("eqw2_begin_eq", (1 << 16, 9), _factors(1 << 15, 64, 8, 7, False, "full")),
        ("eqw2_begin_eq_ahead", (1 << 16, 3), _factors(1 << 15, 128, 8, 7, True)), ("eqw2_begin_eq_ahead", (1 << 17, 2), _factors(1 << 16, 256, 8, 8, True)),
        ("eqw2_begin_eq", (1 << 15, 2), _lb(2, 1 << 14, 64, False, "LDS")), ("eqw2_begin_eq_ahead", (1 << 15, 3), _lb(2, 1 << 14, 64, False, "GATED", gate=True))])
    # the in-launch second stage at the grids whose block sums go out direct by default
    + _rows({"LASSO_DIRECT_NX": "0"}, [
        ("eqw2_begin_r", (1 << 12, 2), _fused(2, 1024, 4, False, True)), ("eqw_round_fused", (1 << 12, 9), _fused(3, 1024, 4, False, False, "full")),
        ("eqw2_begin", (1 << 11, 2), _lb(2, 1024, 4, False, "TABLE")), ("eqw_round", (1 << 13, 9), _lb(3, 4096, 16, False, "TABLE", "full", pipe=0)),
        ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, False, True, "inkernel")), ("eqw2_begin_eq", (1 << 12, 9), _lb(2, 2048, 8, False, "LDS", "full"))])
    # block sums direct from 32 and 64 workgroups per circuit: the host adds up to 64 groups (wait_flag)
    + _rows({"LASSO_DIRECT_NX": "64"}, [
        ("eqw2_begin_r", (1 << 16, 2), _fused(2, 1 << 14, 64, True, True)), ("eqw2_begin_r", (1 << 15, 9), _fused(2, 8192, 32, True, True, "full")),
        ("eqw_round_fused", (1 << 15, 2), _fused(3, 8192, 32, True, False)),
        ("eqw2_begin", (1 << 15, 9), _lb(2, 1 << 14, 64, True, "TABLE", "full")), ("eqw_round", (1 << 15, 2), _lb(3, 1 << 14, 64, True, "TABLE", pipe=0)),
        ("eqw2_begin_ahead", (1 << 15, 2), _ahead(8192, 32, True, True, "gate")), ("eqw2_begin_eq", (1 << 15, 2), _lb(2, 1 << 14, 64, True, "LDS")),
        ("eqw2_begin_eq_ahead", (1 << 15, 3), _lb(2, 1 << 14, 64, True, "GATED", gate=True))])
    # the gate in front of one workgroup
    + _rows({"LASSO_AHEAD_INKERNEL_WGS": "0"}, [
        ("eqw2_begin_ahead", (512, 1), _ahead(128, 1, False, True, "gate")), ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, True, True, "gate"))])
    # 36, 64 and 256 workgroups waiting inside the round's kernel (workgroup 0 polls the mailbox, the others its tag)
    + _rows({"LASSO_AHEAD_INKERNEL_WGS": "4096"}, [
        ("eqw2_begin_ahead", (1 << 12, 9), _ahead(1024, 4, True, True, "inkernel", "full")), ("eqw2_begin_ahead", (1 << 15, 2), _ahead(8192, 32, False, True, "inkernel")),
        ("eqw2_begin_ahead", (1 << 15, 8), _ahead(8192, 32, False, True, "inkernel"))])
    # the x-extent capped at 64 where the default gives 128: two passes per workgroup in every streaming kernel
    + _rows({"LASSO_CUBIC_NX": "64"}, [
        ("eqw2_begin_r", (1 << 17, 1), _fused(2, 1 << 15, 64, False, True)), ("eqw_round_fused", (1 << 17, 1), _fused(3, 1 << 15, 64, False, False)),
        ("eqw2_begin", (1 << 16, 2), _lb(2, 1 << 15, 64, False, "TABLE")), ("eqw2_begin_ahead", (1 << 17, 2), _ahead(1 << 15, 64, False, True, "gate")),
        ("eqw2_begin_eq", (1 << 16, 2), _outer(1 << 15, 64, 8, 7, False))])
    # ... and at 17, one past the last grid whose block sums go out direct — the only way to an x-extent that is no power of two: 32 blocks of indices over 17 workgroups, two
    # passes for the first 15 of them and one for the rest
    + _rows({"LASSO_CUBIC_NX": "17"}, [
        ("eqw2_begin_r", (1 << 15, 2), _fused(2, 8192, 17, False, True)), ("eqw2_begin", (1 << 14, 2), _lb(2, 8192, 17, False, "TABLE")),
        ("eqw2_begin_ahead", (1 << 15, 2), _ahead(8192, 17, False, True, "gate")), ("eqw2_begin_r", (1 << 14, 2), _fused(2, 4096, 16, True, True))])
    # the flag protocol: nobody takes block sums direct
    + _rows({"LASSO_TAGGED_RESULTS": "0"}, [
        ("eqw2_begin", (128, 33), _small(False, 64, "full")), ("eqw2_begin_r", (1 << 14, 2), _fused(2, 4096, 16, False, True)),
        ("eqw2_begin", (1 << 13, 2), _lb(2, 4096, 16, False, "TABLE")), ("eqw_round", (1 << 13, 9), _lb(3, 4096, 16, False, "TABLE", "full", pipe=0)),
        ("eqw2_begin_ahead", (1 << 14, 2), _ahead(4096, 16, False, True, "inkernel")), ("eqw2_begin_ahead", (1 << 15, 2), _ahead(8192, 32, False, True, "gate")),
        ("eqw2_begin_eq", (1 << 12, 2), _lb(2, 2048, 8, False, "LDS")), ("eqw2_begin_eq_ahead", (1 << 12, 2), _lb(2, 2048, 8, False, "GATED", gate=True)),
        ("eqw2_begin_eq_ahead", (1 << 16, 3), _outer(1 << 15, 128, 8, 7, True))])
)
ENVS = []
for _r in TABLE:
    if _r.env not in ENVS:
        ENVS.append(_r.env)
assert len({r.id for r in TABLE}) == len(TABLE)
# the variables cubic_plan's switches are read from: a child process starts without the caller's
SWITCHES = ("LASSO_CUBIC_WIDE", "LASSO_DIRECT_NX", "LASSO_EQ_INLINE_BIG", "LASSO_LB_PIPELINE", "LASSO_LB_NT", "LASSO_AHEAD_INKERNEL_WGS", "LASSO_CUBIC_NX", "LASSO_TAGGED_RESULTS",
            "LASSO_ROUNDS_AHEAD", "LASSO_LAYER_AHEAD", "LASSO_SEQ_START")


def env_id(env):
    return "default" if not env else ",".join(f"{k}={v}" for k, v in sorted(env.items()))


def rows_of(env):
    return [r for r in TABLE if r.env == env]


# ---- the plan of a call (CPU)

_PLAN_EXE = {}


def plan_program(curve):
    """tests/cpp/cubic_plan_dump.cpp built for `curve` into tests/_build/"""
    if curve not in _PLAN_EXE:
        out_dir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(out_dir, exist_ok=True)
        exe = os.path.join(out_dir, "cubic_plan_dump" + ("_bn254" if curve == "bn254" else ""))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", *(["-DLASSO_BN254"] if curve == "bn254" else []), "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", "cubic_plan_dump.cpp")])
        _PLAN_EXE[curve] = exe
    return _PLAN_EXE[curve]


def plans(env, calls, curve):
    """calls: (id, entry, Shape).  One run of the plan program under `env` (a fresh process: the switches are read once) -> {id: plan}"""
    lines = [f"{cid} {entry} {shape.n} {shape.ncirc} {ell_of(shape)} {shape.prof}" for cid, entry, shape in calls]
    e = {k: v for k, v in os.environ.items() if not k.startswith("LASSO_")}
    e.update(env)
    res = subprocess.run([plan_program(curve)], input="\n".join(lines) + "\n", env=e, capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    out = {}
    for ln in res.stdout.splitlines():
        p = json.loads(ln)
        out[p["id"]] = p
    assert set(out) == {c[0] for c in calls}
    return out


def plan_value(plan, key):
    """"form" -> plan["form"], "lb.eq" -> plan["lb"]["eq"]; None where the round has no evaluation-only plan"""
    part, _, field = key.rpartition(".")
    d = plan[part] if part else plan
    return None if d is None else d.get(field)


def plan_mismatches(plan, expect):
    return [f"{key}: planned {plan_value(plan, key)!r}, the table expects {want!r}" for key, want in expect.items() if plan_value(plan, key) != want]


# ---- inputs and runs (the oracle's mock and the device take the same calls)

def _vp(x):
    return np.ascontiguousarray(x, dtype=np.uint64).ctypes.data_as(C.c_void_p)


def inputs_of(row):
    """A, B (one array of n per circuit), tables for the rounds that read one, the eq point and scale, two challenges — a function of entry and shape alone"""
    from gpuutil import rand_fr
    n, k = row.shape.n, row.shape.ncirc
    rng = np.random.default_rng([n, k, ENTRIES.index(row.entry)])
    A = [rand_fr(rng, n) for _ in range(k)]; B = [rand_fr(rng, n) for _ in range(k)]
    E = rand_fr(rng, max(n // 2, 1))
    ell = ell_of(row.shape)
    point = rand_fr(rng, max(ell, 1), edge=False)[:ell]
    scale, r1, r2 = rand_fr(rng, 3, edge=False)
    return A, B, E, point, scale, r1, r2


def _wait(d, count):
    out = np.empty((count, 4), dtype=np.uint64)
    d._chk(d.lib.lasso_result_wait(d.ctx, _vp(out), count))
    return out


def run_row(d, row):
    """the row's call on Device `d` -> {name: array}.  "sums": the round's result; "first": the result that was pending while the round was enqueued; "A" / "B": every array after a
    round that binds, as the device left it (lazily reduced: compare after `canonical`); "E": the table a round wrote; "rc": a refusal's return value"""
    n, k, prof = row.shape
    A, B, E, point, scale, r1, r2 = inputs_of(row)
    ell = ell_of(row.shape)
    pa = [d.upload(x) for x in A]; pb = [d.upload(x) for x in B]
    held = pa + pb
    lib, ctx, PA, PB = d.lib, d.ctx, d._ptrs(pa), d._ptrs(pb)
    bound = lambda m: {"A": np.stack([d.download(p, (m, 4)) for p in pa]), "B": np.stack([d.download(p, (m, 4)) for p in pb])}
    if prof:
        d.prof_enable(prof)
    try:
        if row.entry == "eqw_round":
            pe = d.upload(E); held.append(pe)
            return {"sums": d.sumcheck_cubic_eqw_round(pa, pb, pe, n)}
        if row.entry == "eqw_round_fused":
            pe = d.upload(E[:n // 4]); held.append(pe)
            return {"sums": d.sumcheck_cubic_eqw_round_fused(pa, pb, pe, n, r1), **bound(n // 2)}
        if row.entry == "eqw2_begin":
            pe = d.upload(E); held.append(pe)
            return {"sums": d.sumcheck_cubic_eqw2(pa, pb, pe, n)}
        if row.entry == "eqw2_begin_r":
            pe = d.upload(E[:n // 4]); held.append(pe)
            return {"sums": d.sumcheck_cubic_eqw2(pa, pb, pe, n, r1), **bound(n // 2)}
        if row.entry == "eqw2_begin_ahead":
            # the prover's schedule (test_cubic_round_launched_ahead): round 0 in flight, the next round enqueued behind it without its challenge, round 0's result collected,
            # the challenge posted, the round's result collected
            pe = d.upload(E); held.append(pe)
            d._chk(lib.lasso_sumcheck_cubic_eqw2_begin(ctx, PA, PB, k, C.c_void_p(pe), n, None))
            rc = lib.lasso_sumcheck_cubic_eqw2_begin_ahead(ctx, PA, PB, k, C.c_void_p(pe), n)
            first = _wait(d, 2 * k)
            if row.expect.get("form") == "REFUSED":      # nothing was launched: the caller runs the ordinary round once it has the challenge
                return {"rc": np.array([rc], dtype=np.int64), "first": first, "sums": d.sumcheck_cubic_eqw2(pa, pb, pe, n, r1), **bound(n // 2)}
            d._chk(rc)
            d._chk(lib.lasso_challenge_post(ctx, _vp(r1)))
            return {"first": first, "sums": _wait(d, 2 * k), **bound(n // 2)}
        e_out = d.alloc(32 * (n // 2)); held.append(e_out)
        if row.entry == "eqw2_begin_eq":
            return {"sums": d.sumcheck_cubic_eqw2_eq(pa, pb, e_out, n, point, scale), "E": d.download(e_out, (n // 2, 4))}
        assert row.entry == "eqw2_begin_eq_ahead"
        # test_layer_enqueued_ahead_of_its_point's schedule: the current layer is a resident tail over two arrays of 256 that hands over at 4; the row's round 0 is enqueued
        # in the middle of it, the point posted after its last turn
        rng = np.random.default_rng([n, k, 1000])
        from gpuutil import rand_fr
        n1, k1, ms1 = 256, 2, 4
        A1 = [rand_fr(rng, n1) for _ in range(k1)]; B1 = [rand_fr(rng, n1) for _ in range(k1)]
        ell1 = 7; pt1 = rand_fr(rng, ell1, edge=False); sc1 = rand_fr(rng, 1, edge=False)[0]
        turns1 = ell1 + 1 - 2; chal1 = rand_fr(rng, turns1, edge=False)
        pa1 = [d.upload(x) for x in A1]; pb1 = [d.upload(x) for x in B1]; held += pa1 + pb1
        d._chk(lib.lasso_tail_handover_next(ctx, ms1))
        d._chk(lib.lasso_sumcheck_cubic_tail_begin_eq(ctx, d._ptrs(pa1), d._ptrs(pb1), k1, n1, _vp(pt1), ell1, _vp(sc1)))
        prev = []
        for t in range(turns1 + 1):
            if t == 1:
                d._chk(lib.lasso_sumcheck_cubic_eqw2_begin_eq_ahead(ctx, PA, PB, k, C.c_void_p(e_out), n, ell))
            prev.append(_wait(d, 2 * k1 * (ms1 if t == turns1 else 1)))
            if t < turns1:
                d._chk(lib.lasso_sumcheck_cubic_tail_next(ctx, _vp(chal1[t])))
        d._chk(lib.lasso_point_post(ctx, _vp(point), ell, _vp(scale)))
        return {"sums": _wait(d, 2 * k), "E": d.download(e_out, (n // 2, 4)), "first": np.concatenate(prev)}
    finally:
        if prof:
            d.prof_enable(0)
        for p in held:
            d.free(p)


def reference_key(row):
    """rows that must give the same bytes — the same call on the same inputs, whatever the switches and the profiling mask: one run of the mock serves them all"""
    return (row.entry, row.shape.n, row.shape.ncirc)


def canonical(arr):
    """the canonical representative of every element (the device keeps lazily reduced ones in the arrays it binds): gpuutil.canon over the bytes, for arrays of up to 2^18 elements"""
    from fieldref import L as FR_P
    raw = np.ascontiguousarray(arr, dtype=np.uint64).tobytes()
    out = b"".join((int.from_bytes(raw[i:i + 32], "little") % FR_P).to_bytes(32, "little") for i in range(0, len(raw), 32))
    return np.frombuffer(out, dtype=np.uint64).reshape(np.shape(arr))


LAZY = ("A", "B")      # outputs compared as residues; everything else byte for byte


def comparable(out):
    return {name: (canonical(a) if name in LAZY else np.asarray(a)) for name, a in out.items()}


def reference(mock, row):
    """the expected outputs, from the oracle's mock"""
    return comparable(run_row(mock, row))


DTYPES = {"sums": np.uint64, "first": np.uint64, "A": np.uint64, "B": np.uint64, "E": np.uint64, "rc": np.int64}


def child_main(index):
    """run the rows of ENVS[index] on the device (the environment is the parent's business) and print `ROW <id> <name> <hex>` per output"""
    sys.path.insert(0, ROOT)
    from fieldref import CURVE
    from lasso_amd import Device
    d = Device(0, curve=CURVE)
    for row in rows_of(ENVS[index]):
        for name, arr in run_row(d, row).items():
            print("ROW", row.id, name, np.ascontiguousarray(arr, dtype=DTYPES[name]).tobytes().hex(), flush=True)
    d.close()
    print("DONE", len(rows_of(ENVS[index])))


if __name__ == "__main__":
    child_main(int(sys.argv[1]))
