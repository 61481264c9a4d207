"""CPU: densify from operand columns (include/lasso_hip_operands.h, lasso_host_densify_operands).
  1. lasso_amd/csrc/operand_layout.cuh — the text the device kernel and the host library compile — as a stand-alone host program (under UBSan too) against a Python
     big-integer statement of the layout;
  2. the built-in layouts mean what the reference's tables mean: indices formed by lasso_host_operand_indices, looked up in the materialised subtables and combined as
     and.rs / or.rs / xor.rs / lt.rs / range_check.rs combine them, give x op y;
  3. commitment and proof after densify_operands are the BYTES after densify(operand_indices(...)): through the mock with lasso_densify_dim_operands added (the device
     path), through the plain mock (the fallback) and with LASSO_DENSIFY_OPERANDS=0; lasso_host_densify_stats proves which path ran;
  4. refusals read the same on both paths, and the host stays usable."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

from lasso_amd import CustomStrategy, _abi
from lasso_amd.device import LassoError
from proverutil import HostProver
import customutil
import operandutil as U

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
Layout = _abi.OperandLayout


# ---------------------------------------------------------------- 1. the shared header, stand-alone

def _layout_cases():
    cases = []
    for b in (1, 2):                                   # exhaustive: every operand pair that fits, and the first values that do not
        for c in (1, 2, 3):
            top = 1 << (c * b)
            for operands in (1, 2):
                for msb in (0, 1):
                    for x in range(top + 2):
                        for y in (range(top + 2) if operands == 2 else (0,)):
                            cases.append((operands, b, msb, c, 2 * b, x, y))
    rng = np.random.default_rng(7)
    # (C, b, operands): C b = 64 (no range limit); the last dimension shifts by 64 and must read 0; C b = 64 with one operand of 16 bits; a short one
    for c, b, ops in ((8, 8, 2), (5, 16, 1), (4, 16, 2), (4, 16, 1), (3, 4, 2), (3, 4, 1), (2, 32, 1)):
        edge = [0, 1, (1 << min(64, c * b)) - 1, 1 << min(63, c * b), (1 << (c * b)) % (1 << 64), 1 << 63, (1 << 64) - 1, (1 << (c * b - 1)) % (1 << 64)]
        vals = edge + [int(v) << 1 | int(rng.integers(0, 2)) for v in rng.integers(0, 1 << 63, size=40, dtype=np.uint64)] + [int(v) for v in rng.integers(0, 1 << min(63, c * b), size=40, dtype=np.uint64)]
        for msb in (0, 1):
            for i, x in enumerate(vals):
                cases.append((ops, b, msb, c, 32, x, vals[(7 * i + 3) % len(vals)] if ops == 2 else 0))
    # layouts operand_layout_check refuses: codes 2 (operands), 3 (msb_first), 4 (chunk_bits), 5 (log_m)
    cases += [(0, 4, 0, 2, 8, 1, 1), (3, 4, 0, 2, 16, 1, 1), (2, 4, 2, 2, 8, 1, 1), (2, 0, 0, 2, 8, 1, 1), (2, 5, 0, 2, 8, 1, 1), (1, 9, 0, 2, 8, 1, 0), (1, 33, 0, 1, 33, 1, 0), (2, 16, 0, 4, 33, 1, 1)]
    return cases


def _py_line(operands, b, msb, c, log_m, x, y):
    """what tests/cpp/test_operand_layout_host.cpp must print for one case: include/lasso_hip_operands.h on Python integers"""
    if operands not in (1, 2):
        return "2"
    if msb > 1:
        return "3"
    if log_m > 32:
        return "5"
    if b < 1 or operands * b > log_m:
        return "4"
    return " ".join(["0", str(int(U.py_fits(x, c, b))), str(int(U.py_fits(y, c, b)))] + [str(U.py_index((operands, b, msb), x, y, c, d)) for d in range(c)])


@pytest.mark.parametrize("flags,tag", [(["-O2"], "plain"), (["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"], "ubsan")])
def test_layout_header_against_big_integers(flags, tag):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, f"test_operand_layout_{tag}")
    subprocess.check_call(["g++", "-std=c++17", "-Wall", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_operand_layout_host.cpp")])
    cases = _layout_cases()
    path = os.path.join(out_dir, f"operand_layout_{tag}.txt")
    with open(path, "w") as f:
        f.write("".join("%d %d %d %d %d %x %x\n" % cs for cs in cases))
    res = subprocess.run([exe, path], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    lines = res.stdout.strip().split("\n")
    assert lines[-1] == f"OK {len(cases)}"
    want = [_py_line(*cs) for cs in cases]
    print(f"\n{len(cases)} cases; the statement for (operands, b, msb_first, C, log_m, x, y) = {cases[-9]}: {want[-9]!r}")
    bad = [(cs, g, w) for cs, g, w in zip(cases, lines, want) if g != w]
    assert not bad, bad[:5]
    # the boundary of `fits`, and the shift by 64, were really among the cases
    assert (1, 16, 0, 5, 32, (1 << 64) - 1, 0) in cases and want[cases.index((1, 16, 0, 5, 32, (1 << 64) - 1, 0))].split()[-1] == "0"
    i_in, i_out = ([k for k, cs in enumerate(cases) if cs[:6] == (2, 4, 0, 3, 32, v)][0] for v in ((1 << 12) - 1, 1 << 12))
    assert want[i_in].split()[1] == "1" and want[i_out].split()[1] == "0"


# ---------------------------------------------------------------- 2. the layout means what the tables mean

@pytest.fixture(scope="module")
def mock_dev():
    from gpuutil import load_mock
    from lasso_amd import Device
    d = Device(0, lib=load_mock())
    yield d
    d.close()


@pytest.fixture(scope="module")
def hosts():
    """curve -> (host over the mock with lasso_densify_dim_operands, host over the mock without it); both can prove caller-defined strategies"""
    made = {}

    def get(curve="curve25519"):
        if curve not in made:
            made[curve] = (HostProver(C.CDLL(U.build_mock_prover_operands(curve))), HostProver(C.CDLL(customutil.build_mock_prover_custom(curve))))
        return made[curve]
    yield get
    for a, b in made.values():
        a.close(); b.close()


def _pairs(c, b, exhaustive, seed=3):
    top = 1 << (c * b)
    if exhaustive:
        g = np.arange(top, dtype=np.uint64)
        return np.repeat(g, top), np.tile(g, top)
    rng = np.random.default_rng(seed)
    x = rng.integers(0, top, size=500, dtype=np.uint64); y = rng.integers(0, top, size=500, dtype=np.uint64)
    x[:4] = [0, top - 1, 0, top - 1]; y[:4] = [0, top - 1, top - 1, 0]
    return x, y


@pytest.mark.parametrize("kind", ["and", "or", "xor"])
@pytest.mark.parametrize("c,log_m,exhaustive", [(2, 4, True), (4, 16, False)])
def test_bitwise_layout_against_the_subtables(hosts, mock_dev, kind, c, log_m, exhaustive):
    hp = hosts()[0]
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
    lay = hp.operand_layout(S)
    assert (lay.operands, lay.chunk_bits, lay.msb_first) == (2, log_m // 2, 0)
    T = [int(v) for v in mock_dev.materialize_subtable_u32(S, 0)]
    x, y = _pairs(c, log_m // 2, exhaustive)
    idx = hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m)
    op = {"and": lambda a, b: a & b, "or": lambda a, b: a | b, "xor": lambda a, b: a ^ b}[kind]
    for k in range(len(x)):
        assert sum(T[int(idx[k, i])] << (i * (log_m // 2)) for i in range(c)) == op(int(x[k]), int(y[k])), (int(x[k]), int(y[k]))


def test_lt_layout_against_the_subtables(hosts, mock_dev):
    """sum_i LT[idx_i] prod_{j<i} EQ[idx_j] == (x < y) (lt.rs:60-69), exhaustive at log_m = 4, C = 3: true only if dimension 0 is the MOST significant chunk"""
    hp = hosts()[0]
    c, log_m = 3, 4
    S = _abi.Strategy(_abi.KINDS["lt"], c, log_m, 0)
    lay = hp.operand_layout(S)
    assert (lay.operands, lay.chunk_bits, lay.msb_first) == (2, 2, 1)
    LT = [int(v) for v in mock_dev.materialize_subtable_u32(S, 0)]; EQ = [int(v) for v in mock_dev.materialize_subtable_u32(S, 1)]
    x, y = _pairs(c, 2, True)
    idx = hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m)

    def combine(row):
        total, eq = 0, 1
        for i in range(c):
            total += LT[int(row[i])] * eq; eq *= EQ[int(row[i])]
        return total
    for k in range(len(x)):
        assert combine(idx[k]) == int(int(x[k]) < int(y[k])), (int(x[k]), int(y[k]))
    wrong = hp.operand_indices(x, y, layout=Layout(2, 2, 0), c=c, log_m=log_m)       # the other chunk order proves another statement
    assert any(combine(wrong[k]) != int(int(x[k]) < int(y[k])) for k in range(len(x)))


def test_range_layout_against_the_subtables(hosts, mock_dev):
    """sum_i 2^(i log_m) T_sub(i)[idx_i] == x for x < 2^LOG_R (range_check.rs:62-86), RangeCheck<40> at C = 3, log_m = 16"""
    hp = hosts()[0]
    c, log_m, log_r = 3, 16, 40
    S = _abi.Strategy(_abi.KINDS["range"], c, log_m, log_r)
    lay = hp.operand_layout(S)
    assert (lay.operands, lay.chunk_bits, lay.msb_first) == (1, 16, 0)
    tabs = [[int(v) for v in mock_dev.materialize_subtable_u32(S, t)] for t in range(3)]
    sub = [2 if i * log_m > log_r else (1 if (i + 1) * log_m > log_r else 0) for i in range(c)]
    rng = np.random.default_rng(4)
    x = rng.integers(0, 1 << log_r, size=400, dtype=np.uint64); x[:3] = [0, (1 << log_r) - 1, 1 << (log_r - 1)]
    idx = hp.operand_indices(x, layout=lay, c=c, log_m=log_m)
    for k in range(len(x)):
        assert sum(tabs[sub[i]][int(idx[k, i])] << (i * log_m) for i in range(c)) == int(x[k])
    over = hp.operand_indices(np.array([1 << log_r], dtype=np.uint64), layout=lay, c=c, log_m=log_m)     # fits the chunks, not the range: the tables say so
    assert sum(tabs[sub[i]][int(over[0, i])] << (i * log_m) for i in range(c)) != 1 << log_r


def test_operand_indices_is_the_big_integer_statement(hosts):
    hp = hosts()[0]
    rng = np.random.default_rng(9)
    for lay, c, log_m in (((2, 8, 1), 8, 16), ((1, 16, 0), 5, 16), ((2, 1, 0), 1, 2), ((2, 4, 0), 3, 9), ((1, 32, 1), 2, 32)):
        x, y = U.operands_for(lay, c, 300, rng)
        got = hp.operand_indices(x, y, layout=Layout(*lay), c=c, log_m=log_m)
        assert np.array_equal(got, U.py_indices(lay, x, y, c))


# ---------------------------------------------------------------- 3. byte identity

def _bytes_of(hp, dense, gens, S, r):
    """(commitment, proof).  A single lookup (s = 1) can be densified and committed but not proved — the product trees need two leaves, whatever path densified — so its
    "proof" is the refusal's text, which must not depend on the path either."""
    try:
        comm = hp.commit(dense, gens)
        try:
            return comm, hp.prove(dense, gens, S, r)
        except LassoError as e:
            assert "lasso_gp_build" in str(e) and hp.dense_info(dense)["device_bytes"] > 0
            return comm, str(e)
    finally:
        hp.free(dense)


def _identity_case(hp_dev, hp_plain, S, lay, x, y, c, log_m, alpha, capacity=False):
    n = len(x)
    s = 1 << max((n - 1).bit_length(), 0)
    r = hp_dev.gen_random_point(max(s.bit_length() - 1, 0))
    idx = hp_dev.operand_indices(x, y, layout=lay, c=c, log_m=log_m)
    got = {}
    for tag, hp in (("device", hp_dev), ("fallback", hp_plain)):
        if capacity:
            hp.set_capacity(True)
        try:
            gens = hp.gens(c, s, alpha, log_m)
            want = _bytes_of(hp, hp.densify(idx, log_m), gens, S, r)
            hp.densify_stats(reset=True)
            dense = hp.densify_operands(x, y, layout=lay, c=c, log_m=log_m)
            st = hp.densify_stats()
            got[tag] = _bytes_of(hp, dense, gens, S, r)
            assert got[tag] == want, tag
            assert (s == 1 and isinstance(got[tag][1], str)) or hp.verify(gens, S, s, r, got[tag][1], got[tag][0]) is True
            hp.free(gens=gens)
        finally:
            if capacity:
                hp.set_capacity(False)
        assert st == ({"operand_dims_on_device": c, "available": True} if tag == "device" else {"operand_dims_on_device": 0, "available": False})
    assert got["device"] == got["fallback"]


# (kind, C, log_m, log_r, lookups): every built-in strategy; 3 and 100 lookups leave a padded tail; C = 1, 3, 4
IDENTITY = [("and", 1, 8, 0, 1), ("and", 4, 4, 0, 100), ("or", 3, 6, 0, 3), ("xor", 4, 4, 0, 16), ("xor", 1, 6, 0, 100), ("lt", 3, 4, 0, 100), ("lt", 1, 4, 0, 3), ("range", 3, 8, 20, 100), ("range", 4, 4, 6, 16),
            ("range", 1, 8, 5, 1)]


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", IDENTITY)
def test_bytes_equal_the_index_path(hosts, kind, c, log_m, log_r, lookups):
    hp_dev, hp_plain = hosts()
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    lay, x, y = U.case_operands(hp_dev, kind, c, log_m, log_r, lookups, seed=100 + lookups + c)
    assert (lay.operands, lay.chunk_bits, lay.msb_first) == U.builtin_layout(kind, log_m)
    _identity_case(hp_dev, hp_plain, S, lay, x, y, c, log_m, 2 * c if kind == "lt" else c)


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", [IDENTITY[1], IDENTITY[5], IDENTITY[7]])
def test_bytes_equal_the_index_path_bn254(hosts, kind, c, log_m, log_r, lookups):
    hp_dev, hp_plain = hosts("bn254")
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    lay, x, y = U.case_operands(hp_dev, kind, c, log_m, log_r, lookups, seed=100 + lookups + c)
    _identity_case(hp_dev, hp_plain, S, lay, x, y, c, log_m, 2 * c if kind == "lt" else c)


@pytest.mark.parametrize("curve", ["curve25519", "bn254"])
def test_custom_strategy_with_a_caller_layout(hosts, curve):
    """LTE over operand chunks (customutil.lte_strategy: not in the reference) has no built-in layout: the caller passes lt.rs's, most significant chunk first"""
    hp_dev, hp_plain = hosts(curve)
    c, log_m = 3, 4
    cs = customutil.lte_strategy(c, log_m, curve=curve)
    with pytest.raises(LassoError, match="no built-in operand layout"):
        hp_dev.operand_layout(cs)
    lay = Layout(2, 2, 1)
    x, y = U.operands_for((2, 2, 1), c, 100, np.random.default_rng(21))
    _identity_case(hp_dev, hp_plain, cs, lay, x, y, c, log_m, 2 * c)


def test_capacity_mode_compact_form(hosts):
    """capacity mode on, with dim / read REALLY held as 32-bit integers (LASSO_LEAFLESS_MIN=64, read once per process: a child each) — from operands as from indices,
    through the device entry and through the fallback; and the same bytes as without the mode"""
    import customutil
    case = ["xor", 3, 4, 0, 100, 5]
    env = {"OPERANDS_CHILD_CAPACITY": "1", "LASSO_LEAFLESS_MIN": "64"}
    dev = U.run_child(U.build_mock_prover_operands(), "curve25519", [case], env)[0]
    plain = U.run_child(customutil.build_mock_prover_custom(), "curve25519", [case], env)[0]
    assert dev["compact"] == [True, True] and plain["compact"] == [True, True]
    assert dev["stats"] == {"operand_dims_on_device": 3, "available": True} and plain["stats"] == {"operand_dims_on_device": 0, "available": False}
    assert dev["digest"] == dev["digest_index"] == plain["digest"] == plain["digest_index"] and dev["verify"] is True
    hp_dev, hp_plain = hosts()
    kind, c, log_m, log_r, lookups, seed = case
    lay, x, y = U.case_operands(hp_dev, kind, c, log_m, log_r, lookups, seed)
    _identity_case(hp_dev, hp_plain, _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r), lay, x, y, c, log_m, c, capacity=True)     # capacity mode below the compact form's size


def test_switch_off_takes_the_index_path_with_the_same_bytes(hosts):
    """LASSO_DENSIFY_OPERANDS=0 (read once per process: a fresh child each): the entry point exists and is not used; same bytes as the default"""
    import hashlib
    cases = [[k, c, lm, lr, n, 100 + n + c] for k, c, lm, lr, n in (IDENTITY[1], IDENTITY[5], IDENTITY[7])]
    lib = U.build_mock_prover_operands()
    on = U.run_child(lib, "curve25519", cases, {})
    off = U.run_child(lib, "curve25519", cases, {"LASSO_DENSIFY_OPERANDS": "0"})
    assert [o["stats"] for o in on] == [{"operand_dims_on_device": cs[1], "available": True} for cs in cases]
    assert [o["stats"] for o in off] == [{"operand_dims_on_device": 0, "available": True} for cs in cases]
    assert [o["digest"] for o in on] == [o["digest"] for o in off] and all(o["verify"] is True and o["digest"] == o["digest_index"] for o in on + off)
    hp = hosts()[0]                                          # ... and they are the index path's bytes of this process
    for (kind, c, log_m, log_r, lookups, seed), o in zip(cases, on):
        S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
        lay, x, y = U.case_operands(hp, kind, c, log_m, log_r, lookups, seed)
        s = 1 << (lookups - 1).bit_length()
        gens = hp.gens(c, s, 2 * c if kind == "lt" else c, log_m)
        comm, proof = _bytes_of(hp, hp.densify(hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m), log_m), gens, S, hp.gen_random_point(s.bit_length() - 1))
        hp.free(gens=gens)
        assert hashlib.sha256(comm + proof).hexdigest() == o["digest"]


@pytest.mark.parametrize("curve", ["curve25519", "bn254"])
@pytest.mark.parametrize("world", [2, 4])
def test_slab_mode_from_operands(hosts, curve, world):
    """slab mode (one proof over `world` ranks, the threads harness of tests/test_slab_sharding_cpu.py) with every rank densifying from operands: the single-rank index
    path's bytes, through the device entry (every rank, every dimension) and through the fallback"""
    from test_slab_sharding_cpu import slab_prove
    hp = hosts(curve)[0]
    kind, c, log_m, lookups = "xor", 3, 4, 100
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
    lay, x, y = U.case_operands(hp, kind, c, log_m, 0, lookups, seed=world)
    idx = hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m)
    s = 1 << (lookups - 1).bit_length()
    r = hp.gen_random_point(s.bit_length() - 1)
    gens = hp.gens(c, s, c, log_m)
    want = _bytes_of(hp, hp.densify(idx, log_m), gens, S, r)
    hp.free(gens=gens)
    for with_entry in (True, False):
        lib = C.CDLL(U.build_slab_lib_operands(curve, with_entry))
        lib.slab_operand_dims_on_device.restype = C.c_ulonglong
        lib.slab_set_operands(C.byref(lay), x.ctypes.data_as(C.c_void_p), y.ctypes.data_as(C.c_void_p))
        comm, proof, ncoll, _ = slab_prove(lib, world, S, c, np.zeros_like(idx), r)          # the harness's index argument is ignored: all zeros would prove something else
        assert (comm, proof) == want and ncoll > 0
        assert lib.slab_operand_dims_on_device() == (world * c if with_entry else 0)


# ---------------------------------------------------------------- 4. refusals

def _refusal(call):
    with pytest.raises(LassoError) as e:
        call()
    return str(e.value)


def test_refusals_read_the_same_on_both_paths(hosts):
    hp_dev, hp_plain = hosts()
    c, log_m, n = 3, 4, 16
    lay = Layout(2, 2, 0)
    x, y = U.operands_for((2, 2, 0), c, n, np.random.default_rng(1))
    texts = {}
    for tag, hp in (("device", hp_dev), ("fallback", hp_plain)):
        t = []
        for pos in (0, n - 1):                       # an operand that does not fit, first and last, in either column
            for col in (0, 1):
                bad = [x.copy(), y.copy()]; bad[col][pos] = 1 << (c * 2)
                t.append(_refusal(lambda: hp.densify_operands(bad[0], bad[1], layout=lay, c=c, log_m=log_m)))
                assert "does not fit" in t[-1]
        t.append(_refusal(lambda: hp.densify_operands(x, y, layout=Layout(2, 3, 0), c=c, log_m=5)))                # operands * b > log_m (an odd log_m cannot be split evenly)
        assert "operands * chunk_bits at most log_m" in t[-1]
        t.append(_refusal(lambda: hp.densify_operands(x, y, layout=Layout(2, 0, 0), c=c, log_m=log_m)))
        t.append(_refusal(lambda: hp.densify_operands(x, y, layout=Layout(3, 1, 0), c=c, log_m=log_m)))
        t.append(_refusal(lambda: hp.densify_operands(x, y, layout=Layout(1, 4, 0), c=c, log_m=log_m)))                # y given with a one-operand layout
        assert "second operand column" in t[-1]
        t.append(_refusal(lambda: hp.densify_operands(x, None, layout=lay, c=c, log_m=log_m)))                        # ... and missing with two
        t.append(_refusal(lambda: hp.operand_layout(_abi.Strategy(_abi.KINDS["and"], 2, 5, 0))))                      # odd log_m of a two-operand built-in
        assert "log_m must be even" in t[-1]
        t.append(_refusal(lambda: hp.operand_layout(_abi.Strategy(_abi.KINDS["spark"], 2, 4, 0))))                    # no built-in layout
        assert "no built-in operand layout" in t[-1]
        t.append(_refusal(lambda: hp.operand_indices(np.array([1 << 6], dtype=np.uint64), np.array([0], dtype=np.uint64), layout=lay, c=c, log_m=log_m)))
        texts[tag] = t
        # the host is usable afterwards: the valid instance densifies and proves
        S = _abi.Strategy(_abi.KINDS["xor"], c, log_m, 0)
        gens = hp.gens(c, n, c, log_m)
        comm, proof = _bytes_of(hp, hp.densify_operands(x, y, layout=lay, c=c, log_m=log_m), gens, S, hp.gen_random_point(4))
        assert hp.verify(gens, S, n, hp.gen_random_point(4), proof, comm) is True
        hp.free(gens=gens)
    assert texts["device"] == texts["fallback"]


def test_device_pointers_need_the_device_entry(hosts):
    """where = 1 against a device library without lasso_densify_dim_operands: -1 with a message (nothing could expand device-resident operands on the host); with the
    entry (the mock's "device" memory is host memory) the same call densifies"""
    hp_dev, hp_plain = hosts()
    c, log_m, n = 2, 4, 8
    lay = Layout(2, 2, 0)
    x, y = U.operands_for((2, 2, 0), c, n, np.random.default_rng(2))
    vpt = lambda a: a.ctypes.data_as(C.c_void_p)
    d = C.c_void_p()
    assert hp_plain.lib.lasso_host_densify_operands(hp_plain.h, C.byref(lay), vpt(x), vpt(y), n, c, log_m, 1, C.byref(d)) == -1
    assert "device-resident operands need lasso_densify_dim_operands" in hp_plain.lib.lasso_host_last_error().decode()
    assert hp_plain.lib.lasso_host_densify_operands(hp_plain.h, C.byref(lay), vpt(x), vpt(y), n, c, log_m, 2, C.byref(d)) == -1
    assert hp_dev.lib.lasso_host_densify_operands(hp_dev.h, C.byref(lay), vpt(x), vpt(y), n, c, log_m, 1, C.byref(d)) == 0
    S = _abi.Strategy(_abi.KINDS["and"], c, log_m, 0)
    gens = hp_dev.gens(c, n, c, log_m); r = hp_dev.gen_random_point(3)
    got = _bytes_of(hp_dev, d, gens, S, r)
    assert got == _bytes_of(hp_dev, hp_dev.densify(hp_dev.operand_indices(x, y, layout=lay, c=c, log_m=log_m), log_m), gens, S, r)
    hp_dev.free(gens=gens)


def test_tensor_columns_go_down_as_device_pointers(hosts, monkeypatch):
    """HostProver.densify_operands on tensors: validated (one-dimensional contiguous int64 on the host's device), the tensor's current stream synchronised, the data
    pointers passed with where = 1.  On the CPU the mock's "device" memory is host memory, so a stand-in that reports a CPU tensor as resident on GPU 0 drives the
    whole path (the real thing: tests/test_gpu_operands.py, where torch sees a device)."""
    torch = pytest.importorskip("torch")
    import types
    hp_dev, hp_plain = hosts()
    c, log_m, n = 3, 4, 100
    lay = Layout(2, 2, 1)
    x, y = U.operands_for((2, 2, 1), c, n, np.random.default_rng(8))

    class OnGpu:
        """a CPU tensor that says it lives on GPU `index`"""
        def __init__(self, t, index=0):
            self.t, self.is_cuda, self.device = t, True, types.SimpleNamespace(index=index)
        dtype = property(lambda self: self.t.dtype); shape = property(lambda self: self.t.shape)
        def dim(self): return self.t.dim()
        def is_contiguous(self): return self.t.is_contiguous()
        def data_ptr(self): return self.t.data_ptr()
    synced = []
    monkeypatch.setattr(torch.cuda, "current_stream", lambda device=None: types.SimpleNamespace(synchronize=lambda: synced.append(device.index)))
    tx, ty = torch.from_numpy(x.view(np.int64)), torch.from_numpy(y.view(np.int64))
    S = _abi.Strategy(_abi.KINDS["lt"], c, log_m, 0)
    gens = hp_dev.gens(c, 128, 2 * c, log_m); r = hp_dev.gen_random_point(7)
    hp_dev.densify_stats(reset=True)
    got = _bytes_of(hp_dev, hp_dev.densify_operands(OnGpu(tx), OnGpu(ty), layout=lay, c=c, log_m=log_m), gens, S, r)
    assert synced == [0] and hp_dev.densify_stats()["operand_dims_on_device"] == c
    assert got == _bytes_of(hp_dev, hp_dev.densify(hp_dev.operand_indices(x, y, layout=lay, c=c, log_m=log_m), log_m), gens, S, r)
    hp_dev.free(gens=gens)
    for bad_x, bad_y, why in ((OnGpu(tx.to(torch.int32)), OnGpu(ty.to(torch.int32)), "int64"), (OnGpu(tx[::2]), OnGpu(ty[::2]), "contiguous"), (OnGpu(tx, 1), OnGpu(ty, 1), "GPU 0"),
                              (OnGpu(tx), OnGpu(ty[:50]), "one length"), (OnGpu(tx), y, "both")):
        with pytest.raises(LassoError, match=why):
            hp_dev.densify_operands(bad_x, bad_y, layout=lay, c=c, log_m=log_m)
    with pytest.raises(LassoError, match="device-resident operands need"):          # no device entry: nothing could expand device-resident columns
        hp_plain.densify_operands(OnGpu(tx), OnGpu(ty), layout=lay, c=c, log_m=log_m)


# ---------------------------------------------------------------- the symbols

@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=["curve25519", "bn254"])
def test_libraries_export_the_entry_points(suffix):
    import re
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lasso_hip_operands.h")).read(), flags=re.S)
    assert _abi.declare_operands(dev) == sorted(set(re.findall(r"\b(lasso_[a-z0-9_]+)\s*\(", src)))      # AttributeError = not exported
    hip_h = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "lasso_hip.h")).read(), flags=re.S)
    assert "lasso_densify_dim_operands" not in hip_h                                                  # lasso_hip.h stays what its implementations implement
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for name in ("lasso_host_operand_layout", "lasso_host_operand_indices", "lasso_host_densify_operands", "lasso_host_densify_stats"):
        getattr(host, name)


def test_the_mock_of_the_device_header_has_no_operand_entry():
    from gpuutil import load_mock
    from lasso_amd.device import Device
    mock = load_mock()
    with pytest.raises(AttributeError):
        _abi.declare_operands(mock)
    dev = Device(lib=mock)
    with pytest.raises(LassoError, match="does not export lasso_densify_dim_operands"):
        dev.densify_dim_operands(0, 0, 1, Layout(1, 1, 0), 1, 0, 1, 1, 0, 0, 0, 0)
    dev.close()
