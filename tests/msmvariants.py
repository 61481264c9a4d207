"""The MSM kernels a switch or a shape selects (lasso_amd/csrc/launch_plan.cuh msm_plan, msm_direct_plan, bullet_plan), as ONE table of calls: switch setting, entry point, shape,
and the plan the call must be given.  Three users:

  tests/test_msm_reach_cpu.py    holds every row to the plan tests/cpp/msm_plan_dump.cpp prints for it (the real plan functions over the real switch table, one child process per
                                 setting), and the union of the rows to every kernel, result path and loop shape listed there — without a GPU;
  tests/test_gpu_msm_variants.py runs every row on the device, one child process per setting, against the oracle's mock;
  tests/test_gpu_kernels.py      imports the shape lists of its three commitment tests from here, where the kernels their comments name are checked facts.

Run as a program (`python tests/msmvariants.py <index into ENVS>`) it is that child process: it runs the setting's rows on the device and prints every output as hex.
The curve is fieldref.CURVE (LASSO_TEST_CURVE), as for tests/gpuutil.py."""
import json
import os
import subprocess
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# ---- the shape lists of tests/test_gpu_kernels.py (default switches), each shape with the kernel that serves it: (lasso_hyrax_commit, lasso_hyrax_commit_compressed)

# test_hyrax_commit: (rows, columns, values below maxv — None: full-width scalars), 301 generators
HYRAX_COMMIT_SHAPES = [(1, 1, 5), (4, 8, 256), (16, 256, 1 << 16), (8, 300, 1 << 24), (3, 100, 1 << 32), (2, 64, None),
                       # >= 32 rows of scalars <= 16 bits: the byte-table kernel (k_msm_rows8), one and two byte windows, ragged columns (every row of these is one chunk: the
                       # chunked rows are (64, 300, 16) of HYRAX_COMMIT_U32_SHAPES and TABLE's rows8_chunked), and just past its limits (17 and 24 bits: the bucket kernel again)
                       (64, 256, 256), (40, 77, 2), (300, 300, 1 << 16), (33, 129, 1 << 12), (32, 5, 1 << 9), (64, 100, 1 << 17), (48, 64, 1 << 24),
                       # >= 1024 rows: one wave per row (k_msm_rows8w), one and two byte windows, fewer columns than lanes, ragged rows (not a multiple of 4), all-zero values
                       (1024, 64, 256), (1500, 100, 1 << 16), (2049, 33, 2), (1027, 300, 1 << 12), (1024, 8, 1)]
HYRAX_COMMIT_KERNELS = [("BUCKETS", "BUCKETS")] * 5 + [("DIRECT", "BUCKETS")] + [("ROWS8", "ROWS8")] * 5 + [("BUCKETS", "BUCKETS")] * 2 + [("ROWS8W", "ROWS8W")] * 5
# test_hyrax_commit_u32: (rows, columns, bits of the table's largest value)
HYRAX_COMMIT_U32_SHAPES = [(1, 1, 1), (4, 8, 8), (16, 256, 16), (8, 300, 24), (3, 100, 32), (128, 128, 8), (64, 300, 16), (32, 33, 1), (40, 64, 17)]
HYRAX_COMMIT_U32_KERNELS = ["BUCKETS"] * 5 + ["ROWS8"] * 3 + ["BUCKETS"]
# test_hyrax_commit_full_width_wide_windows: (rows, columns, scalar class) under LASSO_MSM_PIP_MIN_COLS=32 — k_msm_pip_*, "groups" (LASSO_MSM_PIP_SCRATCH_MB=16) in several groups of
# rows — and under LASSO_MSM_PIP=0 the bucket kernel
FULL_WIDTH_WIDE_SHAPES = [(256, 300, "random"), (300, 257, "edges"), (256, 64, "equal"), (512, 300, "sparse"), (333, 300, "groups")]

NGENS_300 = 301   # gpuutil.gens(.., 300): 300 generators and the blinding one, all of them columns of the bases object

# ---- the table

Row = namedtuple("Row", "id env entry shape expect")
# shape: rows, columns, scalar class, points of the bases object.  msm / msm_dev_scaled: one row of n columns; bullet_round: rows = n, cols = nk (a folding round).
# Scalar classes: ("below", maxv) — integers in [0, maxv) with 0 and maxv - 1 present; "cycle4" — the values 0..3 in turn; the full-width ones: "random", "byte_edges" (canonical
# values built from the signed-BYTE digit edges of msm_recode<8>: bytes 0x7f / 0x80 / 0x81 / 0xff in every window, the all-0x80 and all-0xff carry chains, 0, 1, p - 1, p - 2,
# 2^252 - 1), "equal" (every scalar of a row the same), "sparse" (97 % zeros).
# Slab mode (one proof over `world` ranks, include/lasso_hip.h): bullet_round_slab is rows = n, cols = nk, msm_dev_slab one row of n columns, both over the WHOLE generator vector;
# ngens is what ONE rank's bases object holds (its n / world generators, then Q and H).  A row runs every rank 0 .. world - 1 in turn, so `rank` stays 0 in the table.  form:
# bullet_round_slab "fold" (a folding round) or "first" (u == NULL: the inputs are the state); msm_dev_slab runs its three forms (SLAB_MSM_FORMS) in the one row.
Shape = namedtuple("Shape", "rows cols scalars ngens world rank form", defaults=(1, 0, ""))


def _rows(env, entries):
    tag = "default" if not env else "+".join(k.replace("LASSO_", "").replace("MSM_", "").lower() + "=" + v for k, v in sorted(env.items()))
    return [Row(f"{tag}:{name}", env, entry, Shape(*shape), expect) for name, entry, shape, expect in entries]


def _msm3(w8, k1, k33, k301, cap301):
    """lasso_msm at n = 1, 33, 301 by k_msm_direct: chunks per row expected at each n; cap301: items per chunk at its cap at n = 301"""
    return [(f"msm{n}", "msm", (1, n, "random", NGENS_300), {"kernel": "DIRECT", "direct.w8": w8, "direct.K": k, **({"direct.ipc": "cap"} if n == 301 and cap301 else {})})
            for n, k in ((1, k1), (33, k33), (301, k301))]


def _bullet(w8, shapes):
    """lasso_bullet_round as one k_bullet_msm launch: (n, nk, chunks per row, items per chunk at the cap)"""
    return [(f"bullet{n}_{nk}", "bullet_round", (n, nk, "random", n + 2), {"bullet.w8": w8, "bullet.K": k, **({"bullet.ipc": "cap"} if cap else {})}) for n, nk, k, cap in shapes]


def _bullet_slab(w8, shapes):
    """lasso_bullet_round_slab, every rank: (n, nk, world, folding round, wide mapping (nk / 2 >= world), chunks per row, items per chunk at the cap)"""
    return [(f"slab_bullet{n}_{nk}_w{world}" + ("" if fold else "_first"), "bullet_round_slab", (n, nk, "random", n // world + 2, world, 0, "fold" if fold else "first"),
             {"bullet.w8": w8, "bullet.wide": wide, "bullet.K": k, **({"bullet.ipc": "cap"} if cap else {})}) for n, nk, world, fold, wide, k, cap in shapes]


def _msm_slab(w8, shapes):
    """lasso_msm_dev_slab, every rank, in its three forms: (n, world, chunks of the row of n / world + 2 columns, items per chunk at the cap)"""
    return [(f"slab_msm{n}_w{world}", "msm_dev_slab", (1, n, "random", n // world + 2, world), {"direct.w8": w8, "direct.K": k, **({"direct.ipc": "cap"} if cap else {})}) for n, world, k, cap in shapes]


FULL8 = {"LASSO_MSM_FULL8": "1"}
TABLE = (
    # default switches: what no shape of test_gpu_kernels.py reaches — a chunked row of k_msm_rows8 at an odd width, wire bytes of more than 2^16 rows (hipMemcpy instead of the mapped
    # buffer; one column, so that the oracle's reference is four commitments), row sums left on the device
    _rows({}, [("rows8_chunked", "hyrax_commit", (33, 257, ("below", 1 << 16), NGENS_300), {"kernel": "ROWS8", "W8": 2, "K": 2, "result": "MEMCPY"}),
               ("wire_65537", "hyrax_commit_compressed", (65537, 1, "cycle4", 2), {"kernel": "ROWS8W", "rpw": 1, "result": "COMPRESSED_MEMCPY"}),
               ("wire_65537_u32", "hyrax_commit_compressed_u32", (65537, 1, "cycle4", 2), {"kernel": "ROWS8W", "rpw": 1, "result": "COMPRESSED_MEMCPY"}),
               ("rows_dev", "hyrax_commit_rows_dev", (40, 77, ("below", 2), NGENS_300), {"kernel": "ROWS8", "W8": 1, "K": 1, "result": "DEVICE_ROWS"}),
               ("rows_dev_full", "hyrax_commit_rows_dev", (5, 33, "random", NGENS_300), {"kernel": "BUCKETS", "bps": 32, "K": ">1", "result": "DEVICE_ROWS"})]
          + _msm3(True, 1, 5, 38, False) + _bullet(True, [(8, 2, 1, False), (256, 128, 16, False)]))
    # k_msm_rows_full<8>: full-width commitments over the signed byte-multiple table.  Chunked rows, a chunk of 130 columns (an LDS batch of 128 and a ragged one of 2), whole rows of
    # 257 columns (128 + 128 + 1) and of 64, few rows with wire bytes (the compressed form never takes the latency-shaped kernel)
    + _rows(FULL8, [("17x33", "hyrax_commit", (17, 33, "random", NGENS_300), {"kernel": "FULL8", "K": 3, "result": "MEMCPY"}),
                    ("40x257", "hyrax_commit_compressed", (40, 257, "byte_edges", NGENS_300), {"kernel": "FULL8", "K": 6, "cols_per_chunk": 43, "result": "COMPRESSED_MAPPED"}),
                    ("86x259", "hyrax_commit_compressed", (86, 259, "random", NGENS_300), {"kernel": "FULL8", "K": 2, "cols_per_chunk": 130}),
                    ("130x257", "hyrax_commit_compressed", (130, 257, "sparse", NGENS_300), {"kernel": "FULL8", "K": 1, "cols_per_chunk": 257}),
                    ("300x64", "hyrax_commit", (300, 64, "equal", NGENS_300), {"kernel": "FULL8", "K": 1, "cols_per_chunk": 64}),
                    ("3x40_wire", "hyrax_commit_compressed", (3, 40, "byte_edges", NGENS_300), {"kernel": "FULL8", "K": 3}),
                    ("rows_dev", "hyrax_commit_rows_dev", (20, 129, "byte_edges", NGENS_300), {"kernel": "FULL8", "K": ">1", "result": "DEVICE_ROWS"})])
    # k_msm_rows8w with several rows per wave (rpw > 1: the wave-local LDS reuse between consecutive rows), the last wave partly filled
    + _rows({"LASSO_MSM_ROWS8W_WAVES": "400"}, [("1027x33", "hyrax_commit_compressed", (1027, 33, ("below", 1 << 12), NGENS_300), {"kernel": "ROWS8W", "W8": 2, "rpw": 3, "waves": 343})])
    + _rows({"LASSO_MSM_ROWS8W_WAVES": "2048"}, [("2049x8", "hyrax_commit_compressed_u32", (2049, 8, ("below", 256), NGENS_300), {"kernel": "ROWS8W", "W8": 1, "rpw": 2, "waves": 1025}),
                                                 ("1027x33", "hyrax_commit", (1027, 33, ("below", 1 << 12), NGENS_300), {"kernel": "ROWS8W", "W8": 2, "rpw": 1})])
    # k_msm_rows8 at >= 1024 rows (grid.y >= 1024)
    + _rows({"LASSO_MSM_ROWS8W": "0"}, [("1027x33", "hyrax_commit_compressed", (1027, 33, ("below", 1 << 12), NGENS_300), {"kernel": "ROWS8", "W8": 2, "K": 1}),
                                        ("2049x8", "hyrax_commit_compressed_u32", (2049, 8, ("below", 256), NGENS_300), {"kernel": "ROWS8", "W8": 1, "K": 1})])
    # the bucket kernel on small scalars where the byte tables would serve
    + _rows({"LASSO_MSM_ROWS8": "0"}, [("40x77", "hyrax_commit_compressed", (40, 77, ("below", 2), NGENS_300), {"kernel": "BUCKETS", "bps": 4, "K": 1}),
                                       ("300x300", "hyrax_commit_compressed_u32", (300, 300, ("below", 1 << 16), NGENS_300), {"kernel": "BUCKETS", "bps": 4, "K": 1}),
                                       ("33x257", "hyrax_commit", (33, 257, ("below", 1 << 16), NGENS_300), {"kernel": "BUCKETS", "bps": 4, "K": 2})])
    # the bucket kernel on the few-row full-width MSMs of the openings
    + _rows({"LASSO_MSM_DIRECT": "0"}, [(f"msm{n}", "msm", (1, n, "random", NGENS_300), {"kernel": "BUCKETS", "bps": 32, "K": k, "result": "FLAG"}) for n, k in ((1, 1), (33, 3), (301, 19))]
            + [("scaled298", "msm_dev_scaled", (1, 298, "random", NGENS_300), {"kernel": "BUCKETS", "bps": 32, "K": 19, "result": "FLAG"}),
               ("commit8x33", "hyrax_commit", (8, 33, "byte_edges", NGENS_300), {"kernel": "BUCKETS", "bps": 32, "K": 3, "result": "FLAG"}),
               ("bullet8_2", "bullet_round", (8, 2, "random", 10), {"kernel": "BUCKETS", "bps": 32, "rows": 2, "n_cols": 10, "result": "FLAG"}),
               ("bullet256_128", "bullet_round", (256, 128, "random", 258), {"kernel": "BUCKETS", "bps": 32, "rows": 2, "n_cols": 258, "K": 17}),
               ("bullet4096_4", "bullet_round", (4096, 4, "random", 4098), {"kernel": "BUCKETS", "bps": 32, "rows": 2, "n_cols": 4098, "K": 125})])
    # k_msm_direct<.., 4> / k_bullet_msm<.., 4>: the digit-multiple table, 64 windows
    + _rows({"LASSO_MSM_DIRECT8": "0"}, _msm3(False, 1, 9, 76, False) + [("scaled33", "msm_dev_scaled", (1, 33, "random", NGENS_300), {"direct.w8": False, "direct.K": 9})]
            + _bullet(False, [(8, 2, 1, False), (256, 128, 32, False)]))
    # LASSO_MSM_DIRECT_WGS: workgroups of a latency-shaped launch — chunks per row and items per chunk of k_msm_direct and k_bullet_msm.  1: one chunk, or as many as the cap of 128
    # columns per chunk needs (k_bullet_msm takes 4 .. 4096: at 1 it keeps its 256); 7: k_bullet_msm with two chunks' worth of workgroups, the cap again; 4096: the most chunks
    + _rows({"LASSO_MSM_DIRECT_WGS": "1"}, _msm3(True, 1, 1, 3, True) + [("scaled33", "msm_dev_scaled", (1, 33, "random", NGENS_300), {"direct.w8": True, "direct.K": 1})]
            + _bullet(True, [(256, 128, 16, False)]))
    + _rows({"LASSO_MSM_DIRECT_WGS": "7"}, _msm3(True, 1, 5, 7, False) + _bullet(True, [(8, 2, 1, False), (256, 128, 2, False), (4096, 4, 16, True)]))
    + _rows({"LASSO_MSM_DIRECT_WGS": "4096"}, _msm3(True, 1, 5, 38, False) + _bullet(True, [(8, 2, 1, False), (256, 128, 16, False), (4096, 4, 256, False)]))
    + _rows({"LASSO_MSM_DIRECT8": "0", "LASSO_MSM_DIRECT_WGS": "1"}, _msm3(False, 1, 1, 3, True))
    + _rows({"LASSO_MSM_DIRECT8": "0", "LASSO_MSM_DIRECT_WGS": "7"}, _bullet(False, [(256, 128, 2, False), (4096, 4, 16, True)]))
    # k_msm_pip_*: the 12-bit-window kernels at the fewest rows and columns that reach them, in one group of rows and in several (the last one partly filled)
    + _rows({"LASSO_MSM_PIP_MIN_COLS": "32"}, [("256x40", "hyrax_commit_compressed", (256, 40, "random", NGENS_300), {"kernel": "PIP", "pip_group": 256})])
    + _rows({"LASSO_MSM_PIP_MIN_COLS": "32", "LASSO_MSM_PIP_SCRATCH_MB": "16"}, [("300x33", "hyrax_commit", (300, 33, "byte_edges", NGENS_300), {"kernel": "PIP", "pip_group": 64})])
    # slab mode of the opening (k_bullet_msm with P > 1, k_msm_direct through sstride / soffset), every rank of each shape.  The narrow mapping (nk / 2 < world: one row of a rank gets
    # all n / world columns, the other none) with one row of every rank empty, at half = 2 < 4 and at world == n (one generator per rank); the boundary half == world (hl == 1) at 2 and
    # at 8 ranks; a first round (the inputs are the state); the wide mapping in several chunks, folding and first round; the narrow mapping in several chunks (the empty row's eight
    # chunk workgroups accumulate nothing); 1024 fold weights, which the two extra workgroups write in two passes of their stride loop
    + _rows({}, _bullet_slab(True, [(8, 2, 2, True, False, 1, False), (8, 4, 4, True, False, 1, False), (8, 2, 8, True, False, 1, False), (8, 4, 2, True, True, 1, False),
                                    (8, 8, 2, False, True, 1, False), (64, 16, 8, True, True, 1, False), (256, 128, 2, True, True, 8, False), (256, 128, 4, False, True, 4, False),
                                    (256, 2, 4, True, False, 8, False), (4096, 4, 8, True, False, 64, False)])
            + _msm_slab(True, [(2, 2, 1, False), (8, 8, 1, False), (64, 4, 3, False), (296, 8, 5, False), (298, 2, 19, False)]))
    + _rows({"LASSO_MSM_DIRECT8": "0"}, _bullet_slab(False, [(8, 2, 2, True, False, 1, False), (256, 128, 2, True, True, 16, False)]) + _msm_slab(False, [(296, 8, 10, False)]))
    + _rows({"LASSO_MSM_DIRECT_WGS": "1"}, _msm_slab(True, [(298, 2, 2, True)]))
    + _rows({"LASSO_MSM_DIRECT_WGS": "7"}, _bullet_slab(True, [(256, 128, 2, True, True, 2, False), (4096, 2, 4, True, False, 8, True)]))
    + _rows({"LASSO_MSM_DIRECT_WGS": "4096"}, _bullet_slab(True, [(256, 2, 4, True, False, 8, False)]))
)
ENVS = []
for _r in TABLE:
    if _r.env not in ENVS:
        ENVS.append(_r.env)
assert len({r.id for r in TABLE}) == len(TABLE)


def env_id(env):
    return "default" if not env else ",".join(f"{k}={v}" for k, v in sorted(env.items()))


def rows_of(env):
    return [r for r in TABLE if r.env == env]


# ---- the plan of a call (CPU)

def scalar_width(scalars):
    """(bytes per scalar, populated nibbles) as hyrax_commit_impl finds them in the data of a scalar class"""
    if scalars == "cycle4":
        top = 3
    elif isinstance(scalars, tuple):
        top = scalars[1] - 1          # the class holds maxv - 1
    else:
        return 32, 64
    if top >= 1 << 32:
        return 32, 64
    return 4, max(1, (top.bit_length() + 3) // 4)


_PLAN_EXE = {}


def plan_program(curve):
    """tests/cpp/msm_plan_dump.cpp built for `curve` into tests/_build/"""
    if curve not in _PLAN_EXE:
        out_dir = os.path.join(ROOT, "tests", "_build")
        os.makedirs(out_dir, exist_ok=True)
        exe = os.path.join(out_dir, "msm_plan_dump" + ("_bn254" if curve == "bn254" else ""))
        subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", *(["-DLASSO_BN254"] if curve == "bn254" else []), "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", "msm_plan_dump.cpp")])
        _PLAN_EXE[curve] = exe
    return _PLAN_EXE[curve]


def plans(env, calls, curve):
    """calls: (id, entry, Shape).  One run of the plan program under `env` (a fresh process: the switches are read once) -> {id: plan}"""
    lines = []
    for cid, entry, shape in calls:
        bps, w = scalar_width(shape.scalars)
        lines.append(f"{cid} {entry} {shape.rows} {shape.cols} {bps} {w} {shape.ngens} {shape.world}")
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
    """"kernel" -> plan["msm"]["kernel"], "direct.K" -> plan["direct"]["K"]; None where the call does not go through that plan"""
    part, _, field = key.rpartition(".")
    d = plan[part or "msm"]
    return None if d is None else d.get(field)


def plan_mismatches(plan, expect):
    """the entries of `expect` the plan does not meet.  Values: a literal; ">1"; "cap" (items per chunk at the kernel's cap of 128 columns)"""
    bad = []
    for key, want in expect.items():
        got = plan_value(plan, key)
        if want == ">1":
            ok = got is not None and got > 1
        elif want == "cap":
            part = key.rpartition(".")[0]
            ok = got is not None and got == plan[part]["ipc_cap"]
        else:
            ok = got == want
        if not ok:
            bad.append(f"{key}: planned {got!r}, the table expects {want!r}")
    return bad


# ---- inputs and runs (the oracle's mock and the device take the same calls)

def byte_edge_values(p):
    low = lambda b, n=31: sum(b << (8 * w) for w in range(n))      # the byte b in the windows below the top one: < 2^248 < p on both curves
    vals = [0, 1, p - 1, p - 2, 2**252 - 1, 0x7f, 0x80, 0x81, 0xff, 0x100, (0x81 << 240) + 0x80, (0x0f << 248) + (0xff << 240), sum((0x80 if w & 1 else 0x7f) << (8 * w) for w in range(31))]
    for b in (0x7f, 0x80, 0x81, 0xff):
        vals += [low(b), (0x0f << 248) + low(b), low(b, 16), low(b) - low(b, 7)]      # every window; under a top byte; a chain that ends half-way; one that starts above zero bytes
    assert all(0 <= v < p for v in vals)
    return vals


def scalars_of(shape, count=None):
    """(field elements (n, 4) uint64 in memory form, their values as uint32 or None)"""
    from fieldref import L as FR_P, limbs, to_mont
    from gpuutil import rand_fr, small_fr
    n = shape.rows * shape.cols if count is None else count
    kind = shape.scalars
    rng = np.random.default_rng([shape.rows, shape.cols, n])
    if kind == "cycle4":
        v = (np.arange(n, dtype=np.uint64) * 7 + 3) % 4
        four = small_fr(range(4))
        return four[v.astype(np.int64)], v.astype(np.uint32)
    if isinstance(kind, tuple):
        v = rng.integers(0, kind[1], size=n, dtype=np.uint64)
        v[0] = 0; v[-1] = kind[1] - 1
        return small_fr(v), v.astype(np.uint32)
    if kind == "random":
        z = rand_fr(rng, n)
        if n > 2:
            z[n // 2] = 0
        return z, None
    if kind == "byte_edges":
        pats = byte_edge_values(FR_P)
        pick = np.concatenate([np.arange(len(pats)), rng.integers(0, len(pats), size=max(n - len(pats), 0))])[:n]      # every pattern where there is room, then at random
        return np.array([limbs(to_mont(pats[int(i)], FR_P)) for i in pick], dtype=np.uint64).reshape(-1, 4), None
    if kind == "equal":
        return np.repeat(rand_fr(rng, shape.rows, edge=False), shape.cols, axis=0), None
    if kind == "sparse":
        z = rand_fr(rng, n, edge=False)
        z[rng.random(n) < 0.97] = 0
        return z, None
    raise ValueError(kind)


_GENS = {}


def gens_of(mock_lib, ngens):
    from gpuutil import gens
    if ngens not in _GENS:
        _GENS[ngens] = gens(mock_lib, b"gens_sparse_poly", ngens - 1)
    return _GENS[ngens]


# ---- slab mode: the two calls (lasso_amd.Device has no method for them: the host prover is their one caller) and the bases object of a rank

def _vp(a):
    import ctypes as C
    return None if a is None else a.ctypes.data_as(C.c_void_p)


def slab_gens(mock_lib, n, world, rank):
    """what PolyCommitmentGens::init (lasso_amd/host/prover.hpp) hands lasso_bases_create for a rank of slab mode: G[rank::world][: n / world], then Q, then H"""
    g = gens_of(mock_lib, n + 2)      # G_0 .. G_{n-1}, Q, H
    return np.concatenate([g[rank:n:world][: n // world], g[n:n + 2]])


def bullet_round_slab(d, bases, n, world, rank, pa, pb, pw, pa2, pb2, pw2, nk, u, ui, blinds):
    """lasso_bullet_round_slab on Device `d` (u None: a first round) -> the rank's partial L and R, (2, 16)"""
    import ctypes as C
    blinds = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(2, 4)
    u = None if u is None else np.ascontiguousarray(u, dtype=np.uint64); ui = None if u is None else np.ascontiguousarray(ui, dtype=np.uint64)
    out = np.empty((2, 16), dtype=np.uint64)
    d._chk(d.lib.lasso_bullet_round_slab(d.ctx, C.c_void_p(bases), n, world, rank, C.c_void_p(pa), C.c_void_p(pb), C.c_void_p(pw), C.c_void_p(pa2), C.c_void_p(pb2), C.c_void_p(pw2), nk,
                                         _vp(u), _vp(ui), _vp(blinds), _vp(out)))
    return out


def msm_dev_slab(d, bases, p_scalars, n, world, rank, scale, tail):
    """lasso_msm_dev_slab on Device `d` (scale / tail None: NULL) -> the rank's partial point, (1, 16)"""
    import ctypes as C
    scale = None if scale is None else np.ascontiguousarray(scale, dtype=np.uint64); tail = None if tail is None else np.ascontiguousarray(tail, dtype=np.uint64).reshape(2, 4)
    out = np.empty((1, 16), dtype=np.uint64)
    d._chk(d.lib.lasso_msm_dev_slab(d.ctx, C.c_void_p(bases), C.c_void_p(p_scalars), n, world, rank, _vp(scale), _vp(tail), _vp(out)))
    return out


# the forms of lasso_msm_dev_slab: (name, scalar class, scale given, tail given).  Without a scale or without a tail the scalars reach the recoder as they are, hence the edge classes
SLAB_MSM_FORMS = (("full", "random", True, True), ("noscale", "byte_edges", False, True), ("notail", "sparse", True, False))


def bullet_inputs(s, fold=True):
    """the state a bullet-round row starts from: a, b (2 nk entries before a fold, nk in a first round), the fold weights, blinds, u, u^-1"""
    from gpuutil import rand_fr
    n, nk = s.rows, s.cols
    rng = np.random.default_rng([s.rows, s.cols, 77])
    length = 2 * nk if fold else nk
    nw = n // length
    a, bb, w = scalars_of(s, length)[0], rand_fr(rng, length, edge=False), rand_fr(rng, nw, edge=False)
    blinds = rand_fr(rng, 2, edge=False); u, ui = rand_fr(rng, 2, edge=False)
    return a, bb, w, blinds, u, ui


def _run_slab_row(d, row, mock_lib):
    """every rank of a slab row on Device `d`, each over a bases object of its own: outputs named `<name>_r<rank>`"""
    s = row.shape
    out = {}
    if row.entry == "bullet_round_slab":
        n, nk, fold = s.rows, s.cols, s.form == "fold"
        a, bb, w, blinds, u, ui = bullet_inputs(s, fold)
        nw = len(w)
        for rank in range(s.world):
            b = d.bases_create(slab_gens(mock_lib, n, s.world, rank))
            pa = d.upload(a); pb = d.upload(bb); pw = d.upload(w)
            try:
                if fold:
                    pa2 = d.alloc(32 * nk); pb2 = d.alloc(32 * nk); pw2 = d.alloc(32 * 2 * nw)
                    out[f"points_r{rank}"] = bullet_round_slab(d, b, n, s.world, rank, pa, pb, pw, pa2, pb2, pw2, nk, u, ui, blinds)
                    out.update({f"a_r{rank}": d.download(pa2, (nk, 4)), f"b_r{rank}": d.download(pb2, (nk, 4)), f"w_r{rank}": d.download(pw2, (2 * nw, 4))})
                    for p in (pa2, pb2, pw2):
                        d.free(p)
                else:
                    out[f"points_r{rank}"] = bullet_round_slab(d, b, n, s.world, rank, pa, pb, pw, 0, 0, 0, nk, None, None, blinds)
            finally:
                for p in (pa, pb, pw):
                    d.free(p)
                d.bases_destroy(b)
        return out
    assert row.entry == "msm_dev_slab"
    from gpuutil import rand_fr
    n = s.cols
    rng = np.random.default_rng([s.rows, s.cols, 77])
    scale, tail = rand_fr(rng, 1, edge=False), rand_fr(rng, 2, edge=False)
    ptrs = {name: d.upload(scalars_of(s._replace(scalars=cls))[0]) for name, cls, _, _ in SLAB_MSM_FORMS}
    for rank in range(s.world):
        b = d.bases_create(slab_gens(mock_lib, n, s.world, rank))
        try:
            for name, _, with_scale, with_tail in SLAB_MSM_FORMS:
                out[f"points_{name}_r{rank}"] = msm_dev_slab(d, b, ptrs[name], n, s.world, rank, scale if with_scale else None, tail if with_tail else None)
        finally:
            d.bases_destroy(b)
    for p in ptrs.values():
        d.free(p)
    return out


def run_row(d, row, mock_lib):
    """the row's call on Device `d` -> {name: array}.  "points...": projective points, compared as wire bytes; everything else is compared as it is"""
    import ctypes as C
    from gpuutil import rand_fr
    s = row.shape
    if row.entry in ("bullet_round_slab", "msm_dev_slab"):
        return _run_slab_row(d, row, mock_lib)
    b = d.bases_create(gens_of(mock_lib, s.ngens))
    try:
        if row.entry.startswith("hyrax_commit"):
            z, u32 = scalars_of(s)
            if row.entry == "hyrax_commit_compressed_u32":
                p = d.upload(u32)
                out = {"wire": d.hyrax_commit_compressed_u32(p, int(u32.max()), s.rows, s.cols, b)}
            else:
                p = d.upload(z)
                if row.entry == "hyrax_commit":
                    out = {"points": d.hyrax_commit(p, s.rows, s.cols, b)}
                elif row.entry == "hyrax_commit_compressed":
                    out = {"wire": d.hyrax_commit_compressed(p, s.rows, s.cols, b)}
                else:      # the row sums left on the device in the kernels' point form, then through lasso_points_reduce_compress as the one part of each row
                    rows = d.alloc(s.rows * d.lib.lasso_point_row_bytes())
                    d._chk(d.lib.lasso_hyrax_commit_rows_dev(d.ctx, C.c_void_p(p), s.rows, s.cols, C.c_void_p(b), C.c_void_p(rows)))
                    wire = np.empty((s.rows, 32), dtype=np.uint8)
                    d._chk(d.lib.lasso_points_reduce_compress(d.ctx, C.c_void_p(rows), 1, s.rows, wire.ctypes.data_as(C.c_void_p)))
                    d.free(rows)
                    out = {"wire": wire}
            d.free(p)
            return out
        if row.entry == "msm":
            return {"points": d.msm(b, scalars_of(s)[0])}
        rng = np.random.default_rng([s.rows, s.cols, 77])
        if row.entry == "msm_dev_scaled":
            p = d.upload(scalars_of(s)[0])
            out = {"points": d.msm_dev_scaled(b, p, s.cols, rand_fr(rng, 1, edge=False), rand_fr(rng, 2, edge=False))}
            d.free(p)
            return out
        assert row.entry == "bullet_round"
        n, nk = s.rows, s.cols
        nw = n // (2 * nk)
        a, bb, w = scalars_of(s, 2 * nk)[0], rand_fr(rng, 2 * nk, edge=False), rand_fr(rng, nw, edge=False)
        blinds = rand_fr(rng, 2, edge=False); u, ui = rand_fr(rng, 2, edge=False)
        pa = d.upload(a); pb = d.upload(bb); pw = d.upload(w); pa2 = d.alloc(32 * nk); pb2 = d.alloc(32 * nk); pw2 = d.alloc(32 * 2 * nw)
        out = {"points": d.bullet_round(b, n, pa, pb, pw, pa2, pb2, pw2, nk, u, ui, blinds)}
        out.update(a=d.download(pa2, (nk, 4)), b=d.download(pb2, (nk, 4)), w=d.download(pw2, (2 * nw, 4)))
        for p in (pa, pb, pw, pa2, pb2, pw2):
            d.free(p)
        return out
    finally:
        d.bases_destroy(b)


def reference_key(row):
    """rows that must give the same bytes: one call of the mock serves them all"""
    return ("commit" if row.entry.startswith("hyrax_commit") else row.entry,) + tuple(row.shape)


def reference(mock, row):
    """the expected outputs, from the oracle's mock: wire bytes for every point"""
    from gpuutil import compress_points
    s = row.shape
    if row.entry.startswith("hyrax_commit"):
        if s.scalars == "cycle4":      # one column of four distinct values: the mock commits to the 4 x 1 matrix of those, each row takes its value's commitment
            from gpuutil import small_fr
            b = mock.bases_create(gens_of(mock.lib, s.ngens)); p = mock.upload(small_fr(range(4)))
            four = mock.hyrax_commit_compressed(p, 4, 1, b)
            mock.free(p); mock.bases_destroy(b)
            return {"wire": four[scalars_of(s)[1].astype(np.int64)]}
        return {"wire": run_row(mock, row._replace(entry="hyrax_commit_compressed"), mock.lib)["wire"]}
    return as_wire(mock.lib, run_row(mock, row, mock.lib))


def as_wire(mock_lib, out):
    """a run's outputs in the form `reference` gives"""
    from gpuutil import compress_points
    out = dict(out)
    for name in [k for k in out if k.startswith("points")]:      # "points", and a slab row's "points_r<rank>", "points_<form>_r<rank>"
        out["wire" + name[len("points"):]] = np.frombuffer(b"".join(compress_points(mock_lib, np.asarray(out.pop(name)).reshape(-1, 16))), dtype=np.uint8).reshape(-1, 32)
    return out


DTYPES = {"points": np.uint64, "wire": np.uint8, "a": np.uint64, "b": np.uint64, "w": np.uint64}


def dtype_of(name):
    """the element type of an output: a slab row's names carry a form and a rank behind the plain name"""
    return DTYPES[name.split("_")[0]]


def child_main(index):
    """run the rows of ENVS[index] on the device (the environment is the parent's business) and print `ROW <id> <name> <hex>` per output"""
    sys.path.insert(0, ROOT)
    from fieldref import CURVE
    from gpuutil import load_mock
    from lasso_amd import Device
    mock_lib = load_mock()
    d = Device(0, curve=CURVE)
    for row in rows_of(ENVS[index]):
        for name, arr in run_row(d, row, mock_lib).items():
            print("ROW", row.id, name, np.ascontiguousarray(arr, dtype=dtype_of(name)).tobytes().hex(), flush=True)
    d.close()
    print("DONE", len(rows_of(ENVS[index])))


if __name__ == "__main__":
    child_main(int(sys.argv[1]))
