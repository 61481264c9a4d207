"""CPU: caller-defined subtable strategies (include/lasso_hip.h lasso_strategy_custom, lasso_amd.CustomStrategy) through the host prover over the oracle's mock of
the device ABI.

  1. the verifier accepts oracle-pinned proofs of every built-in strategy under the EQUIVALENT custom descriptor (tables and g given as data);
  2. ... and rejects them when one coefficient, one term's memory index, one table entry or one proof byte is changed: g and the tables are really used;
  3. every class of malformed descriptor is LASSO_ERR_INVALID with a message, and the host stays usable;
  4. proving: the mock cannot be edited, so tests/cpp/mock_custom_wrap.cpp wraps its two strategy-taking entry points with a literal loop over the term list.
     A built-in strategy proved as a descriptor gives the built-in's commitment and proof BYTES (one rank and two), and two strategies the reference does not ship
     are proved, verified and tamper-rejected."""
import ctypes as C

import numpy as np
import pytest

from lasso_amd import CustomStrategy, _abi
from lasso_amd.device import LassoError
from lasso_amd.custom import FR_MODULUS
from proverutil import HostProver, OracleSession, build_mock_prover
import customutil as U

# (kind, C, log_m, log_r, lookups): AND C = 1, 4; OR; XOR C = 8; LT C = 2, 4; RangeCheck C = 4 whose LOG_R = 6 produces all three subtables (full, remainder, zeros); Spark C = 4
SHAPES = [("and", 1, 8, 0, 1 << 10), ("and", 4, 4, 0, 1 << 6), ("or", 2, 6, 0, 1 << 7), ("xor", 8, 4, 0, 1 << 6), ("lt", 2, 4, 0, 1 << 8), ("lt", 4, 4, 0, 1 << 6),
          ("range", 4, 4, 6, 1 << 7), ("spark", 4, 4, 0, 1 << 6)]
BN254_SHAPES = [("and", 4, 4, 0, 1 << 6), ("lt", 2, 4, 0, 1 << 6), ("spark", 4, 4, 0, 1 << 6)]


def _alpha(kind, c):
    return 2 * c if kind == "lt" else c


@pytest.fixture(scope="module")
def hosts():
    """curve -> (host over the plain mock, host over the wrapped mock)"""
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = (HostProver(C.CDLL(build_mock_prover(curve))), HostProver(C.CDLL(U.build_mock_prover_custom(curve))))
        return made[curve]
    yield get
    for a, b in made.values():
        a.close(); b.close()


def _instance(hp, kind, c, log_m, log_r, lookups, seed=11):
    s = 1 << max((lookups - 1).bit_length(), 0)
    idx = np.ascontiguousarray(np.random.default_rng(seed + lookups + c).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64))
    r = hp.gen_random_point(max(s.bit_length() - 1, 0))
    return s, idx, r


def _prove(hp, S, c, log_m, alpha, s, idx, r):
    gens = hp.gens(c, s, alpha, log_m)
    dense = hp.densify(idx, log_m)
    try:
        return gens, hp.commit(dense, gens), hp.prove(dense, gens, S, r)
    finally:
        hp.free(dense)


def _verdict(hp, gens, S, s, r, proof, comm):
    try:
        return hp.verify(gens, S, s, r, proof, comm)
    except LassoError:
        return None


def _oracle_for(curve):
    import conftest
    return conftest._load_oracle(conftest._build_oracle_bn254() if curve == "bn254" else conftest._build_oracle())


def _variant(cs, coeff=None, mem=None, table=None):
    """the same descriptor with one coefficient, one term's memory index or one table entry changed"""
    terms = [(cf, list(m)) for cf, m in cs.terms]
    tables = [t.copy() for t in cs.tables]
    if coeff is not None:
        terms[coeff] = (terms[coeff][0] + 1, terms[coeff][1])
    if mem is not None:
        t = next(i for i in reversed(range(len(terms))) if terms[i][1])
        terms[t][1][-1] = (terms[t][1][-1] + 1) % cs.num_memories
    if table is not None:
        if cs.field:
            tables[0][table][0] ^= np.uint64(1)
        else:
            tables[0][table] ^= 1
    maps = {} if cs._msub is None else {"memory_subtable": cs._msub, "memory_dimension": cs._mdim}
    return CustomStrategy(cs.c, cs.log_m, tables, terms, num_memories=cs.num_memories, curve=cs.curve, **maps)


def _accept_and_reject(hp, gens, cs, s, r, proof, comm):
    assert hp.verify(gens, cs, s, r, proof, comm) is True
    assert _verdict(hp, gens, _variant(cs, coeff=0), s, r, proof, comm) is not True, "a changed coefficient was accepted"
    if cs.num_memories > 1:
        assert _verdict(hp, gens, _variant(cs, mem=True), s, r, proof, comm) is not True, "a changed memory index was accepted"
    assert _verdict(hp, gens, _variant(cs, table=3), s, r, proof, comm) is not True, "a changed table entry was accepted"
    for pos in (len(proof) // 3, len(proof) - 40):
        bad = bytearray(proof); bad[pos] ^= 4
        assert _verdict(hp, gens, cs, s, r, bytes(bad), comm) is not True, f"proof byte {pos} flipped and accepted"


# ---- 1 + 2: the verifier, on bytes pinned to the oracle

@pytest.mark.parametrize("curve,kind,c,log_m,log_r,lookups", [("curve25519", *x) for x in SHAPES] + [("bn254", *x) for x in BN254_SHAPES])
def test_verifier_accepts_builtin_proofs_under_the_custom_descriptor(hosts, curve, kind, c, log_m, log_r, lookups):
    plain, _ = hosts(curve)
    s, idx, r = _instance(plain, kind, c, log_m, log_r, lookups)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    gens, comm, proof = _prove(plain, S, c, log_m, _alpha(kind, c), s, idx, r)
    try:
        o = OracleSession(_oracle_for(curve), _abi.KINDS[kind], c, log_m, log_r, idx, r)
        assert proof == o.prove() and comm == o.commit(), "the built-in proof is not the oracle's"
        o.close()
        cs = U.builtin_as_custom(kind, c, log_m, log_r, curve, host=plain)
        assert cs.num_memories == _alpha(kind, c)
        _accept_and_reject(plain, gens, cs, s, r, proof, comm)
    finally:
        plain.free(gens=gens)


# ---- 3: descriptor validation

def _good(curve="curve25519"):
    return U.builtin_as_custom("lt", 2, 4, 0, curve)


def _break(name):
    cs = _good()
    d = cs.desc
    if name == "term_mem out of range":
        cs._mem[1] = 4
    elif name == "memory_subtable out of range":
        cs._msub = np.array([0, 1, 0, 2], dtype=np.uint32); cs._mdim = np.array([0, 0, 1, 1], dtype=np.uint32)
        d.memory_subtable, d.memory_dimension = cs._msub.ctypes.data, cs._mdim.ctypes.data
    elif name == "memory_dimension out of range":
        cs._msub = np.array([0, 1, 0, 1], dtype=np.uint32); cs._mdim = np.array([0, 0, 1, 2], dtype=np.uint32)
        d.memory_subtable, d.memory_dimension = cs._msub.ctypes.data, cs._mdim.ctypes.data
    elif name == "only one map":
        cs._msub = np.array([0, 1, 0, 1], dtype=np.uint32)
        d.memory_subtable = cs._msub.ctypes.data
    elif name == "term_start not monotone":
        cs._start[1] = 3; cs._start[2] = 2
    elif name == "term_start[0] not zero":
        cs._start[0] = 1
    elif name == "table pointer null":
        cs._ptrs[1] = None
    elif name == "no tables":
        d.tables_u32 = None
    elif name == "both table forms":
        d.tables_fr = d.tables_u32
    elif name == "num_memories 0":
        d.num_memories = 0
    elif name == "num_memories 33":
        d.num_memories = 33
    elif name == "default map too small":
        d.num_memories = 5          # 5 memories over 2 subtables need 3 dimensions, C = 2
    elif name == "no terms":
        d.num_terms = 0
    elif name == "coeff null":
        d.coeff = None
    elif name == "degree over the bound":
        cs = CustomStrategy(2, 4, cs.tables, [(1, [0] * 17)])
    elif name == "too many terms":
        cs = CustomStrategy(2, 4, cs.tables, [(1, [0])] * (_abi.CUSTOM_MAX_TERMS + 1))
    elif name == "too many factors":
        cs = CustomStrategy(2, 4, cs.tables, [(1, [0] * 16)] * (_abi.CUSTOM_MAX_FACTORS // 16 + 1))
    else:
        raise KeyError(name)
    return cs


BROKEN = ["term_mem out of range", "memory_subtable out of range", "memory_dimension out of range", "only one map", "term_start not monotone", "term_start[0] not zero",
          "table pointer null", "no tables", "both table forms", "num_memories 0", "num_memories 33", "default map too small", "no terms", "coeff null", "degree over the bound",
          "too many terms", "too many factors"]


@pytest.mark.parametrize("name", BROKEN)
def test_bad_descriptor_is_invalid_with_a_message_and_the_host_stays_usable(hosts, name):
    _, hp = hosts("curve25519")
    bad = _break(name)
    rc = hp.lib.lasso_host_strategy_check(bad.ptr())
    assert rc == -1, f"{name}: rc {rc}"                      # LASSO_ERR_INVALID
    msg = hp.lib.lasso_host_last_error().decode()
    assert msg.startswith("custom strategy:") and len(msg) > 20, msg
    # the same through prove and verify, then a valid call on the same host
    s, idx, r = _instance(hp, "lt", 2, 4, 0, 64)
    good = _good()
    gens, comm, proof = _prove(hp, good, 2, 4, 4, s, idx, r)
    try:
        dense = hp.densify(idx, 4)
        with pytest.raises(LassoError, match="custom strategy"):
            hp.prove(dense, gens, bad, r)
        with pytest.raises(LassoError, match="custom strategy"):
            hp.verify(gens, bad, s, r, proof, comm)
        assert hp.prove(dense, gens, good, r) == proof
        assert hp.verify(gens, good, s, r, proof, comm) is True
        hp.free(dense)
    finally:
        hp.free(gens=gens)


def test_caps_exactly_reached_are_valid(hosts):
    _, hp = hosts("curve25519")
    t = _good().tables
    hp.strategy_check(CustomStrategy(2, 4, t, [(1, [i % 4] * 8) for i in range(_abi.CUSTOM_MAX_TERMS)]))                 # 256 terms, 2048 factors
    hp.strategy_check(CustomStrategy(2, 4, t, [(1, [0] * 16)] * (_abi.CUSTOM_MAX_FACTORS // 16)))          # longest legal term (sumcheck degree 17), 2048 factors
    hp.strategy_check(CustomStrategy(16, 4, t, [(1, [0])], num_memories=32))                               # LASSO_MAX_ALPHA memories


def test_num_memories_must_match_the_generators(hosts):
    _, hp = hosts("curve25519")
    s, idx, r = _instance(hp, "lt", 2, 4, 0, 64)
    good = _good()
    gens_small = hp.gens(2, s, 1, 4)          # made for ONE memory: the derefs set is too small for four
    gens = hp.gens(2, s, 4, 4)
    dense = hp.densify(idx, 4)
    try:
        with pytest.raises(LassoError, match="num_memories does not match the generators"):
            hp.prove(dense, gens_small, good, r)
        proof = hp.prove(dense, gens, good, r)     # the host is usable afterwards
        with pytest.raises(LassoError, match="num_memories does not match the generators"):
            hp.verify(gens_small, good, s, r, proof, hp.commit(dense, gens))
    finally:
        hp.free(dense, gens); hp.free(gens=gens_small)


# ---- 4: proving on the CPU through the wrapped mock

@pytest.mark.parametrize("curve,kind,c,log_m,log_r,lookups", [("curve25519", *x) for x in SHAPES] + [("bn254", *x) for x in BN254_SHAPES])
def test_custom_as_builtin_proves_the_builtin_bytes(hosts, curve, kind, c, log_m, log_r, lookups):
    plain, hp = hosts(curve)
    s, idx, r = _instance(plain, kind, c, log_m, log_r, lookups)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    g0, comm0, proof0 = _prove(plain, S, c, log_m, _alpha(kind, c), s, idx, r)
    plain.free(gens=g0)
    cs = U.builtin_as_custom(kind, c, log_m, log_r, curve, host=plain)
    gens, comm, proof = _prove(hp, cs, c, log_m, cs.num_memories, s, idx, r)
    try:
        assert comm == comm0, "commitment differs from the built-in's"
        assert proof == proof0, "proof differs from the built-in's"
        assert hp.verify(gens, cs, s, r, proof, comm) is True
        assert hp.verify(gens, S, s, r, proof, comm) is True
    finally:
        hp.free(gens=gens)


def _slab_lib():
    """tests/cpp/slab_threads.cpp (the ranks of one proof as threads) over the wrapped mock"""
    return C.CDLL(build_mock_prover(ext=("custom",), harness=["slab_threads.cpp"], extra_flags=["-pthread"]))


def _slab_prove(lib, world, sptr, num_memories, idx, r, capacity=False):
    idx = np.ascontiguousarray(idx, dtype=np.uint64); r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
    comm = (C.c_uint8 * (1 << 20))(); proof = (C.c_uint8 * (1 << 22))(); cl = C.c_size_t(); pl = C.c_size_t(); nc = C.c_size_t(); nb = C.c_size_t(); err = C.create_string_buffer(512)
    rc = lib.slab_prove_threads_ex(world, sptr, C.c_size_t(num_memories), idx.ctypes.data_as(C.c_void_p), C.c_size_t(idx.shape[0]), r.ctypes.data_as(C.c_void_p), C.c_size_t(r.shape[0]),
                                   None, 1 if capacity else 0, 1, comm, C.c_size_t(len(comm)), C.byref(cl), proof, C.c_size_t(len(proof)), C.byref(pl), C.byref(nc), C.byref(nb), None, None, None,
                                   err, C.c_size_t(512))
    assert rc == 0, err.value.decode()
    return bytes(comm[: cl.value]), bytes(proof[: pl.value])


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups,capacity", [("and", 2, 8, 0, 1 << 9, False), ("lt", 2, 6, 0, 1 << 8, False), ("spark", 2, 6, 0, 1 << 8, True)])
def test_two_ranks_prove_the_single_rank_bytes(hosts, kind, c, log_m, log_r, lookups, capacity):
    """slab mode (one linear and two non-linear shapes, one of them in capacity mode): a custom strategy works wherever Spark works"""
    plain, hp = hosts("curve25519")
    s, idx, r = _instance(plain, kind, c, log_m, log_r, lookups)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    g0, comm0, proof0 = _prove(plain, S, c, log_m, _alpha(kind, c), s, idx, r)
    plain.free(gens=g0)
    cs = U.builtin_as_custom(kind, c, log_m, log_r, host=plain)
    comm, proof = _slab_prove(_slab_lib(), 2, cs.ptr(), cs.num_memories, idx, r, capacity)
    assert comm == comm0 and proof == proof0


def _claimed_evaluation(proof):
    """surge.rs:92-104 in wire order: comm_derefs (u64 n, n x 32 B), the primary sumcheck (u64 rounds, per round u64 k + k x 32 B), then claimed_evaluation"""
    pos = 8 + 32 * int.from_bytes(proof[:8], "little")
    rounds = int.from_bytes(proof[pos:pos + 8], "little"); pos += 8
    for _ in range(rounds):
        pos += 8 + 32 * int.from_bytes(proof[pos:pos + 8], "little")
    return int.from_bytes(proof[pos:pos + 32], "little")


def expected_claim(cs, idx, r_words, s, values_of):
    """sum_k eq(r, k) g(E_1(k), .., E_alpha(k)) on Python ints: E_i(k) = T_{subtable(i)}[idx[k][dimension(i)]], padded lookups read address 0"""
    p = FR_MODULUS[cs.curve]
    rinv = pow(1 << 256, -1, p)
    r = [(int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192) * rinv % p for w in np.asarray(r_words).reshape(-1, 4)]
    eq = U.eq_evals_int(r, p)
    total = 0
    for k in range(s):
        row = idx[k] if k < idx.shape[0] else [0] * cs.c
        vals = []
        for i in range(cs.num_memories):
            sub, dim = cs.memory_map(i)
            vals.append(values_of(sub, int(row[dim])))
        total += eq[k] * U.g_int(cs.terms, vals, p)
    return total % p


@pytest.mark.parametrize("curve", ["curve25519", "bn254"])
@pytest.mark.parametrize("which,lookups", [("lte", 1 << 7), ("lte", 100), ("field", 1 << 6)])
def test_new_strategies_are_proved_verified_and_bound_to_g(hosts, curve, which, lookups):
    _, hp = hosts(curve)
    c, log_m = 3, 4
    cs = U.lte_strategy(c, log_m, curve) if which == "lte" else U.field_square_strategy(c, log_m, 5, curve)
    assert not cs.linear and len({len(m) for _, m in cs.terms}) > 1
    s, idx, r = _instance(hp, which, c, log_m, 0, lookups)
    gens, comm, proof = _prove(hp, cs, c, log_m, cs.num_memories, s, idx, r)
    try:
        _accept_and_reject(hp, gens, cs, s, r, proof, comm)
        values_of = (lambda sub, a: cs.table_values[sub][a]) if which == "field" else (lambda sub, a: int(cs.tables[sub][a]))
        assert _claimed_evaluation(proof) == expected_claim(cs, idx, r, s, values_of)
        if which == "lte":      # and the claim really is "x <= y chunk-wise, most significant chunk first": a direct statement of LTE over the operands
            p = FR_MODULUS[curve]
            bits = log_m // 2

            def lte(row):
                for a in row:
                    x, y = int(a) >> bits, int(a) & ((1 << bits) - 1)
                    if x != y:
                        return int(x < y)
                return 1
            rinv = pow(1 << 256, -1, p)
            rr = [(int(w[0]) | int(w[1]) << 64 | int(w[2]) << 128 | int(w[3]) << 192) * rinv % p for w in np.asarray(r).reshape(-1, 4)]
            eq = U.eq_evals_int(rr, p)
            want = sum(eq[k] * lte(idx[k] if k < idx.shape[0] else [0] * c) for k in range(s)) % p
            assert _claimed_evaluation(proof) == want
    finally:
        hp.free(gens=gens)
