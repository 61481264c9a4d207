"""CPU: the lookup results as a vector, and the identity that ties them to a proof (include/lasso_hip_values.h, include/lasso_prover_values.h):

      MLE(values)(r)  ==  the claimed_evaluation inside the proof bytes,       values[k] = combine_lookups(T[dim(k)])

  1. the new headers declare exactly the new names, the pinned headers none of them; both prover libraries export them;
  2. lasso_host_lookup_values_ref against direct statements: x & y / x | y / x ^ y, x < y and x under the built-in operand layouts, and Python integers over the
     tables for every kind on both curves;
  3. the 64-bit form: equal to the field form wherever offered, refused with one text elsewhere; shapes exactly at and exactly past the 2^64 bound;
  4. over the mock with lasso_lookup_values as a literal loop (tests/cpp/mock_values_wrap.cpp): lookup_values(dense) == lookup_values_ref(indices),
     values_evaluate(values, r) == claimed_evaluation(prove(...)), proofs before and after the call are equal; capacity mode; a slab host is refused; the statistics;
     a library linked against the plain mock refuses the device calls with a message and keeps the CPU statement;
  5. claimed_evaluation against the byte walk on the golden artefacts, and its errors;
  6. the integer combine header as a stand-alone program, plain and under -fsanitize=undefined, against Python integers at the 64-bit edge;
  7. the shapes tests/test_gpu_lookup_values.py runs reach several passes per lane, a ragged last workgroup, an odd n and an n below one wave (tests/cpp/values_plan_dump.cpp)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import customutil as U
import mleutil as M
import valuesutil as V
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver
from test_abi_exports import header_functions

ROOT = V.ROOT
CURVES = V.CURVES
DEVICE_NAMES = ["lasso_lookup_values"]
HOST_NAMES = ["lasso_host_dense_len", "lasso_host_lookup_values", "lasso_host_lookup_values_ref", "lasso_host_proof_claimed_evaluation", "lasso_host_values_evaluate", "lasso_host_values_stats"]


@pytest.fixture(scope="module")
def hosts():
    made = {}

    def get(curve="curve25519"):
        if curve not in made:
            made[curve] = HostProver(C.CDLL(V.build_mock_prover_values(curve)), curve=curve)
        return made[curve]
    yield get
    for hp in made.values():
        hp.close()


# ---- 1: headers and libraries

def test_new_headers_declare_exactly_the_new_names():
    assert sorted(header_functions("lasso_hip_values.h")) == DEVICE_NAMES
    assert sorted(header_functions("lasso_prover_values.h")) == HOST_NAMES
    pinned = set(header_functions("lasso_hip.h")) | set(header_functions("lasso_prover.h"))
    assert not pinned & set(DEVICE_NAMES + HOST_NAMES)


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_entries(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_values(dev) == DEVICE_NAMES
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for n in HOST_NAMES:
        getattr(host, n)


# ---- 2: the CPU statement against direct statements

def _pairs(c, b, exhaustive, seed=3):
    """tests/test_operands_cpu.py::_pairs: every operand pair, or 500 random ones with the corner operands in front"""
    top = 1 << (c * b)
    if exhaustive:
        g = np.arange(top, dtype=np.uint64)
        return np.repeat(g, top), np.tile(g, top)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, top, size=500, dtype=np.uint64); y = rng.integers(0, top, size=500, dtype=np.uint64)
    x[:4] = [0, top - 1, 0, top - 1]; y[:4] = [0, top - 1, top - 1, 0]
    return x, y


def _ref_ints(hp, strategy, idx, curve, n):
    return V.words_to_ints(hp.lookup_values_ref(strategy, idx), curve)[:n]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["and", "or", "xor"])
@pytest.mark.parametrize("c,log_m,exhaustive", [(2, 4, True), (4, 16, False), (8, 16, False)])
def test_bitwise_values_are_the_operation_on_the_operands(hosts, curve, kind, c, log_m, exhaustive):
    hp = hosts(curve)
    st = V.builtin(kind, c, log_m)
    x, y = _pairs(c, log_m // 2, exhaustive)
    idx = hp.operand_indices(x, y, layout=hp.operand_layout(st), c=c, log_m=log_m)
    want = {"and": x & y, "or": x | y, "xor": x ^ y}[kind]
    assert _ref_ints(hp, st, idx, curve, len(x)) == [int(v) for v in want]
    assert hp.lookup_values_ref(st, idx, form="u64")[:len(x)].tolist() == [int(v) for v in want]


@pytest.mark.parametrize("curve", CURVES)
def test_lt_value_is_the_comparison(hosts, curve):
    hp = hosts(curve)
    c, log_m = 3, 4
    st = V.builtin("lt", c, log_m)
    x, y = _pairs(c, log_m // 2, True)
    idx = hp.operand_indices(x, y, layout=hp.operand_layout(st), c=c, log_m=log_m)
    want = [int(a < b) for a, b in zip(x.tolist(), y.tolist())]
    assert _ref_ints(hp, st, idx, curve, len(x)) == want
    assert hp.lookup_values_ref(st, idx, form="u64")[:len(x)].tolist() == want


@pytest.mark.parametrize("curve", CURVES)
def test_range_check_value_is_the_operand(hosts, curve):
    hp = hosts(curve)
    c, log_m, log_r = 3, 16, 40
    st = V.builtin("range", c, log_m, log_r)
    rng = np.random.default_rng(9)
    x = rng.integers(0, 1 << log_r, size=400, dtype=np.uint64)
    x[:3] = [0, (1 << log_r) - 1, 1 << (log_r - 1)]
    idx = hp.operand_indices(x, None, layout=hp.operand_layout(st), c=c, log_m=log_m)
    assert _ref_ints(hp, st, idx, curve, len(x)) == x.tolist()
    assert hp.lookup_values_ref(st, idx, form="u64")[:len(x)].tolist() == x.tolist()


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("lookups", [1, 2, 13])
def test_every_kind_is_g_over_the_tables_on_python_integers(hosts, curve, lookups):
    hp = hosts(curve)
    for name, st, desc in V.all_kinds(curve, hp, c=2, log_m=4):
        idx = V.random_indices(2, 4, lookups, seed=lookups)
        got = hp.lookup_values_ref(st, idx)
        s = 1 << max((lookups - 1).bit_length(), 0)
        assert got.shape == (s, 4), name
        assert V.words_to_ints(got, curve) == V.values_int(desc, idx), name      # padding rows included: address 0 in every dimension


# ---- 3: the 64-bit form

def test_the_bound_of_the_u64_form_is_met_exactly_and_exactly_missed():
    """RangeCheck C = 4, log_m = 16: (2^16 - 1)(1 + 2^16 + 2^32 + 2^48) = 2^64 - 1, the largest value a u64 holds; C = 5 at log_m = 13 ((C - 1) * inc = 52 < 64 still
    holds) is the first shape past it — checked here on Python integers before the library is asked"""
    at = sum(((1 << 16) - 1) << (16 * i) for i in range(4))
    assert at == (1 << 64) - 1 and V.u64_offered("range", 4, 16)
    past = sum(((1 << 13) - 1) << (13 * i) for i in range(5))
    assert past >= 1 << 64 and past - (((1 << 13) - 1) << 52) < 1 << 64 and not V.u64_offered("range", 5, 13)
    assert V.u64_offered("xor", 8, 16) and V.u64_offered("and", 4, 16)      # 64 bits of operand exactly


@pytest.mark.parametrize("curve", CURVES)
def test_u64_form_at_the_bound_equals_the_field_form(hosts, curve):
    hp = hosts(curve)
    for kind, c, log_m, log_r in (("range", 4, 16, 64), ("xor", 8, 16, 0), ("or", 8, 16, 0), ("lt", 16, 4, 0)):
        st = V.builtin(kind, c, log_m, log_r)
        idx = V.random_indices(c, log_m, 37, seed=c)
        idx[3, :] = (1 << log_m) - 1                                        # every chunk maximal: RangeCheck and OR reach 2^64 - 1
        u = hp.lookup_values_ref(st, idx, form="u64")
        f = V.words_to_ints(hp.lookup_values_ref(st, idx), curve)
        assert [int(v) for v in u] == f, kind
        if kind in ("range", "or"):
            assert int(u[3]) == (1 << 64) - 1


@pytest.mark.parametrize("curve", CURVES)
def test_u64_form_is_refused_with_one_text_on_both_routes(hosts, curve):
    hp = hosts(curve)
    kinds = {name: (st, desc) for name, st, desc in V.all_kinds(curve, hp, c=2, log_m=4)}
    refused = [kinds["spark"][0], kinds["lte"][0], kinds["xor_as_custom"][0], kinds["field_square"][0]]
    idx = V.random_indices(2, 4, 5, seed=1)
    texts = set()
    for st in refused:
        dense = hp.densify(idx, 4)
        try:
            for call in (lambda: hp.lookup_values_ref(st, idx, form="u64"), lambda: hp.lookup_values(dense, st, form="u64")):
                with pytest.raises(LassoError, match=V.U64_TEXT) as e:
                    call()
                texts.add(str(e.value))
        finally:
            hp.free(dense)
    past = V.builtin("range", 5, 13, 60)
    idx5 = V.random_indices(5, 13, 3, seed=2)
    dense = hp.densify(idx5, 13)
    try:
        for call in (lambda: hp.lookup_values_ref(past, idx5, form="u64"), lambda: hp.lookup_values(dense, past, form="u64")):
            with pytest.raises(LassoError, match=V.U64_TEXT) as e:
                call()
            texts.add(str(e.value))
        assert V.words_to_ints(hp.lookup_values(dense, past), curve) == V.words_to_ints(hp.lookup_values_ref(past, idx5), curve)      # the field form is there
    finally:
        hp.free(dense)
    assert len(texts) == 1, texts


# ---- 4: over the mock

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("lookups", [13, 1, 2])
def test_values_evaluate_to_the_claim_inside_the_proof(hosts, curve, lookups):
    hp = hosts(curve)
    for name, st, desc in V.all_kinds(curve, hp, c=2, log_m=4):
        V.check_identity(hp, curve, name, st, desc, V.random_indices(2, 4, lookups, seed=7 + lookups), 4)


@pytest.mark.parametrize("curve", CURVES)
def test_the_same_in_capacity_mode_with_a_compact_representation(curve):
    """LASSO_LEAFLESS_MIN is read once per process: a child (tests/valuesutil.py CAPACITY_CHILD) runs the identity over a compact representation"""
    env = dict(os.environ, LASSO_LEAFLESS_MIN="64")
    env.pop("LASSO_CAPACITY_COMPACT", None)
    res = subprocess.run([sys.executable, "-c", V.CAPACITY_CHILD, ROOT, V.build_mock_prover_values(curve), curve, "200"], capture_output=True, text=True, timeout=600, env=env)
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    assert json.loads(res.stdout.strip().split("\n")[-1]) == {"compact": True, "kinds": ["and", "lt", "spark", "field_square"]}


def test_mismatched_strategy_and_slab_host_are_refused(hosts):
    hp = hosts()
    idx = V.random_indices(2, 4, 8, seed=1)
    dense = hp.densify(idx, 4)
    try:
        with pytest.raises(LassoError, match="do not match the densified representation"):
            hp.lookup_values(dense, V.builtin("and", 3, 4))
        with pytest.raises(LassoError, match="do not match the densified representation"):
            hp.lookup_values(dense, V.builtin("and", 2, 6))
    finally:
        hp.free(dense)
    # a two-rank slab host: rank 0's representation holds the even lookups only
    slab = HostProver(C.CDLL(V.build_mock_prover_values("curve25519")))
    try:
        from lasso_amd.prover import ALLGATHER_FN
        cb = ALLGATHER_FN(lambda user, send, recv, nbytes: 1)           # never called: densify makes no collective
        slab._allgather = cb
        slab._chk(slab.lib.lasso_host_set_comm(slab.h, 0, 2, cb, None))
        dense = slab.densify(V.random_indices(2, 4, 16, seed=2), 4)
        try:
            with pytest.raises(LassoError, match="slab-mode representation"):
                slab.lookup_values(dense, V.builtin("and", 2, 4))
        finally:
            slab.free(dense)
    finally:
        slab.close()


def test_plain_mock_refuses_the_device_calls_and_keeps_the_cpu_statement():
    from proverutil import build_mock_prover
    hp = HostProver(C.CDLL(build_mock_prover()))
    try:
        st = V.builtin("xor", 2, 4)
        idx = V.random_indices(2, 4, 5, seed=4)
        assert hp.values_stats() == {"device_lookups": 0, "available": False}
        ref = hp.lookup_values_ref(st, idx)
        assert V.words_to_ints(ref, "curve25519") == V.values_int(U.builtin_as_custom("xor", 2, 4), idx)
        dense = hp.densify(idx, 4)
        try:
            with pytest.raises(LassoError, match="lasso_lookup_values, include/lasso_hip_values.h\\) is not available"):
                hp.lookup_values(dense, st)
        finally:
            hp.free(dense)
        with pytest.raises(LassoError, match="include/lasso_hip_mle.h\\) is not available"):
            hp.values_evaluate(ref, hp.gen_random_point(3))
        assert np.array_equal(hp.values_evaluate(ref[:1], np.zeros((0, 4), dtype=np.uint64)), ref[0])       # no variables: answered on the host
    finally:
        hp.close()


# ---- 5: the claim inside the proof bytes

@pytest.mark.parametrize("art,curve", [("artefact_and_c1_2p10", "curve25519"), ("artefact_and_c1_2p24", "curve25519"), ("artefact_bn254_and_c4_2p8", "bn254")])
def test_claimed_evaluation_on_the_golden_artefacts(hosts, art, curve):
    from test_custom_strategy_cpu import _claimed_evaluation as walk_cpu
    hp = hosts(curve)
    proof = open(os.path.join(ROOT, "tests", "golden", art, "proof.bin"), "rb").read()
    got = V.claim_int(hp.claimed_evaluation(proof), curve)
    assert got == walk_cpu(proof) == V.walker_claim(proof)[0]
    # tests/test_gpu_custom_strategy.py carries the same walk (a GPU module: not imported here; its text is held to this one's instead)
    src_gpu = open(os.path.join(ROOT, "tests", "test_gpu_custom_strategy.py")).read()
    src_cpu = open(os.path.join(ROOT, "tests", "test_custom_strategy_cpu.py")).read()
    body = lambda src: [l.strip() for l in src[src.index("def _claimed_evaluation(proof):"):].split("\n")[1:8] if l.strip() and not l.strip().startswith('"""')][:5]
    assert body(src_gpu) == body(src_cpu)


@pytest.mark.parametrize("curve", CURVES)
def test_claimed_evaluation_errors(hosts, curve):
    hp = hosts(curve)
    art = "artefact_bn254_and_c4_2p8" if curve == "bn254" else "artefact_and_c1_2p10"
    proof = open(os.path.join(ROOT, "tests", "golden", art, "proof.bin"), "rb").read()
    _, pos = V.walker_claim(proof)
    with pytest.raises(LassoError, match="truncated"):
        hp.claimed_evaluation(proof[:pos + 17])                       # cut inside the scalar
    with pytest.raises(LassoError, match="truncated"):
        hp.claimed_evaluation(proof[:4])                              # cut inside the first length prefix
    first_round = 8 + 32 * int.from_bytes(proof[:8], "little") + 8
    with pytest.raises(LassoError, match="truncated|implausible vector length"):
        hp.claimed_evaluation(proof[:first_round + 3])                # cut inside a round's length prefix: the round count in front of it can no longer be backed by bytes
    huge = bytearray(proof); huge[:8] = (1 << 60).to_bytes(8, "little")
    with pytest.raises(LassoError, match="implausible vector length"):
        hp.claimed_evaluation(bytes(huge))
    bad = bytearray(proof); bad[pos:pos + 32] = FR_MODULUS[curve].to_bytes(32, "little")
    with pytest.raises(LassoError, match="not canonical"):
        hp.claimed_evaluation(bytes(bad))
    ok = bytearray(proof); ok[pos:pos + 32] = (FR_MODULUS[curve] - 1).to_bytes(32, "little")
    assert V.claim_int(hp.claimed_evaluation(bytes(ok)), curve) == FR_MODULUS[curve] - 1


# ---- 6: the integer combine on the host, against Python integers

def _combine_exe(san):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_values_combine_host{'_ubsan' if san else ''}")
    flags = ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"] if san else ["-O2"]
    subprocess.check_call(["g++", "-std=c++17", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_values_combine_host.cpp")])
    return exe


@pytest.mark.parametrize("san", [False, True], ids=["plain", "ubsan"])
def test_integer_combine_against_python_integers(san):
    exe = _combine_exe(san)
    K = _abi.KINDS
    lines, want = [], []
    rng = np.random.default_rng(5)
    shapes = [("range", 4, 16), ("range", 5, 13), ("range", 2, 32), ("range", 1, 32), ("xor", 8, 16), ("and", 16, 8), ("or", 32, 4), ("xor", 32, 2), ("range", 3, 21), ("range", 4, 21), ("and", 1, 2)]
    for kind, c, log_m in shapes:
        inc = log_m if kind == "range" else log_m // 2
        mx = (1 << log_m) - 1 if kind == "range" else (1 << (log_m // 2)) - 1
        bound = sum(mx << (i * inc) for i in range(c))
        for entries in ([mx] * c, [2**32 - 1] * c, [0] * c, [int(v) for v in rng.integers(0, mx + 1, size=c)]):      # every entry at max_table_value under every weight; u32's own maximum
            lines.append(f"lin {K[kind]} {c} {log_m} {c} " + " ".join(map(str, entries)))
            total = sum(e << (i * inc) for i, e in enumerate(entries))
            want.append([int(bound < 1 << 64), bound >> 64, bound & (2**64 - 1), total >> 64, total & (2**64 - 1)] + [(total >> (29 * k)) & ((1 << 29) - 1 if k < 4 else (1 << 12) - 1) for k in range(5)])
            assert total < 1 << 116 + 12
    lt_cases = [[(1, 0)], [(0, 1), (1, 0)], [(0, 1)] * 15 + [(1, 0)], [(0, 1)] * 16, [(0, 0)] * 16, [(1, 0)] * 16, [(0, 1), (0, 0), (1, 0)]]
    for pairs in lt_cases:
        lines.append(f"lt {len(pairs)} " + " ".join(f"{a} {b}" for a, b in pairs))
        g, run = 0, 1
        for a, b in pairs:
            g += a * run; run *= b
        want.append([g])
    res = subprocess.run([exe], input="\n".join(lines) + "\n", capture_output=True, text=True, timeout=60)
    assert res.returncode == 0, res.stderr[-2000:]
    got = [[int(x) for x in l.split()] for l in res.stdout.strip().split("\n")]
    assert got == want
    assert V.u64_offered("range", 4, 16) and want[0][0] == 1 and want[4][0] == 0        # the library's rule at and past the bound is Python's


# ---- 7: reach of the GPU shapes

def test_gpu_shapes_reach_the_plan_boundaries():
    exe = os.path.join(ROOT, "tests", "_build", "values_plan_dump")
    os.makedirs(os.path.dirname(exe), exist_ok=True)
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "cpp", "values_plan_dump.cpp")])
    ns = V.GPU_NS + [V.GPU_N_PASSES]
    out = subprocess.run([exe, str(V.GPU_NX)] + [str(n) for n in ns], capture_output=True, text=True, check=True).stdout
    plans = [json.loads(l) for l in out.strip().split("\n")]
    for pair in (0, 1):
        mine = {p["n"]: p for p in plans if p["pair"] == pair}
        assert mine[V.GPU_N_PASSES]["passes"] >= 3 and mine[V.GPU_N_PASSES]["nx"] == V.GPU_NX            # a lane with at least three grid-stride passes
        assert any(p["last_block_items"] and p["nx"] > 1 for p in mine.values())                          # a ragged last workgroup behind a full one
        assert any(p["items"] < 64 for p in mine.values())                                                 # n below one wave
        assert any(p["items"] == p["block"] for p in mine.values()) or pair                                # exactly one full workgroup (one lookup per item)
    assert V.GPU_N_PASSES % 2 == 1 and any(n % 2 for n in V.GPU_NS) and any(n % 2 == 0 for n in V.GPU_NS)  # the two-per-lane store: odd tails and none
    free = [json.loads(l) for l in subprocess.run([exe, "0", str(1 << 24)], capture_output=True, text=True, check=True).stdout.strip().split("\n")]
    assert all(p["nx"] == p["max_nx"] for p in free)                                                        # unset: the cap of launch_plan.cuh
