"""-m gpu: caller-defined subtable strategies (include/lasso_hip.h lasso_strategy_custom) on the real library.

  5. kernel level: lasso_sumcheck_combine_round / lasso_combine_claim with random term lists against Python big-integer arithmetic — n = 2 .. 2^14, alpha in
     {1, 2, 3, 8, 17, 32}, every sumcheck degree 1 .. 17 with one term and with several (every instantiation of k_combine_round_custom), repeated memories, zero and
     p - 1 coefficients, constant terms, the caps exactly reached, field-edge values and lazily reduced inputs up to LAZY_BOUND;
  6. whole proofs: a built-in strategy proved as a descriptor gives the built-in's commitment and proof bytes, both curves, capacity mode, Spark C = 4 at 2^20, LT C = 16 at 2^12;
  7. two strategies the reference does not ship, proved, verified, tamper-rejected; the claimed evaluation against big integers;
  8. a LINEAR custom strategy takes the built-in linear route: same launch counts per kernel family as built-in AND at 2^16;
  9. an invalid descriptor sent straight to the device entry points is LASSO_ERR_INVALID, nothing launched, context usable."""
import ctypes as C

import numpy as np
import pytest

import customutil as U
from fieldref import CURVE, L as FR_P, R
from gpuutil import EDGE, edge_fr, full_fr, ints, lift, words
from lasso_amd import CustomStrategy, _abi
from lasso_amd.device import LassoError

pytestmark = pytest.mark.gpu

RINV = pow(R, -1, FR_P)
ALPHAS = [1, 2, 3, 8, 17, 32]


@pytest.fixture(scope="module")
def dev():
    from lasso_amd import Device
    d = Device(0, curve=CURVE)
    yield d
    d.close()


def vals(rows):
    return [x * RINV % FR_P for x in ints(rows)]


def dummy_tables():
    return [np.zeros(4, dtype=np.uint32)]


def descriptor(alpha, terms):
    """a descriptor for the two device entry points, which read c, num_memories and the term list only"""
    return CustomStrategy(alpha, 2, dummy_tables(), terms, num_memories=alpha, memory_subtable=[0] * alpha, memory_dimension=list(range(alpha)), curve=CURVE)


def random_terms(rng, alpha, longest, nterms, coeffs=None):
    """nterms terms over alpha memories, the first of length `longest`, the others shorter or equal (mixed), memories drawn with repetition"""
    terms = []
    for t in range(nterms):
        ln = longest if t == 0 else int(rng.integers(0 if longest == 0 else 1, longest + 1))
        cf = int.from_bytes(rng.bytes(40), "little") % FR_P if coeffs is None else coeffs[t % len(coeffs)]
        terms.append((cf, [int(x) for x in rng.integers(0, alpha, size=ln)]))
    return terms


def want_round(terms, polys, eq, n, degree):
    half = n // 2
    P = [vals(p) for p in polys]; E = vals(eq)
    out = [0] * (degree + 1)
    for i in range(half):
        lo = [p[i] for p in P]; d = [p[half + i] - p[i] for p in P]
        for x in range(degree + 1):
            v = [(lo[j] + x * d[j]) % FR_P for j in range(len(P))]
            out[x] += (E[i] + x * (E[half + i] - E[i])) * U.g_int(terms, v, FR_P)
    return words([o % FR_P * R % FR_P for o in out])


def want_claim(terms, polys, eq, n):
    P = [vals(p) for p in polys]; E = vals(eq)
    return words([sum(E[k] * U.g_int(terms, [p[k] for p in P], FR_P) for k in range(n)) % FR_P * R % FR_P])


def inputs(rng, alpha, n, edges=True):
    polys = [full_fr(rng, n) for _ in range(alpha)]
    eq = full_fr(rng, n)
    if edges:
        for j, p in enumerate(polys + [eq]):     # every EDGE word somewhere, at a different offset per array
            k = min(n, len(EDGE))
            p[:k] = edge_fr(range(j, j + k))
    return polys, eq


def run(dev, cs, polys, eq, n):
    pp = [dev.upload(p) for p in polys]; pe = dev.upload(eq)
    try:
        return dev.sumcheck_combine_round(cs, pp, pe, n, cs.degree), dev.combine_claim(cs, pp, pe, n)
    finally:
        for p in pp + [pe]:
            dev.free(p)


def check(dev, terms, alpha, n, rng, lazy=True):
    cs = descriptor(alpha, terms)
    polys, eq = inputs(rng, alpha, n)
    got_r, got_c = run(dev, cs, polys, eq, n)
    assert np.array_equal(got_r, want_round(terms, polys, eq, n, cs.degree)), "round differs from big-integer arithmetic"
    assert np.array_equal(got_c, want_claim(terms, polys, eq, n)), "claim differs from big-integer arithmetic"
    if lazy:   # every field array replaced by its largest representative below LAZY_BOUND: same bytes out
        lr, lc = run(dev, cs, [lift(p) for p in polys], lift(eq), n)
        assert np.array_equal(lr, got_r) and np.array_equal(lc, got_c), "lazily reduced inputs change the result"


# ---- 5: kernel level

@pytest.mark.parametrize("degree", range(1, 18))
def test_every_degree_one_term_and_several(dev, degree):
    rng = np.random.default_rng(1000 + degree)
    alpha = ALPHAS[degree % len(ALPHAS)]
    longest = degree - 1
    check(dev, random_terms(rng, alpha, longest, 1), alpha, 64, rng)                                 # one term: the PROD-shaped instantiations
    check(dev, [(1, [int(x) for x in rng.integers(0, alpha, size=longest)])], alpha, 64, rng)        # ... with coefficient 1: no coefficient product at all
    check(dev, random_terms(rng, alpha, longest, 5), alpha, 64, rng)                                 # several terms of mixed length


@pytest.mark.parametrize("log_n", [1, 2, 5, 10, 14])
@pytest.mark.parametrize("alpha", ALPHAS)
def test_sizes_and_memory_counts(dev, log_n, alpha):
    rng = np.random.default_rng(77 * log_n + alpha)
    longest = [2, 3, 4][(log_n + alpha) % 3]
    check(dev, random_terms(rng, alpha, longest, 3), alpha, 1 << log_n, rng, lazy=log_n <= 10)


def test_repeated_memories_special_coefficients_and_constants(dev):
    rng = np.random.default_rng(5)
    terms = [(FR_P - 1, [0, 0, 0]), (0, [1, 2]), (7, []), (1, [2, 2]), (FR_P - 1, []), (2, [1]), (1, [0, 1, 2]), (0, [])]
    check(dev, terms, 3, 256, rng)
    check(dev, [(5, [])], 2, 64, rng)                                   # a constant g: sumcheck degree 1
    check(dev, [(0, [0, 1])], 2, 64, rng)                               # g = 0
    check(dev, [(1, [0]), (FR_P - 1, [0])], 1, 64, rng)                 # cancels to 0 through p - 1
    check(dev, [(3, [0]), (4, [1]), (5, [0])], 2, 128, rng)             # linear g through the general kernel (the prover takes the eq-weighted path instead)
    check(dev, [(1, [i]) for i in range(32)] * 8, 32, 32, rng)          # 256 single-factor terms: v is folded after every one


def test_caps_exactly_reached(dev):
    rng = np.random.default_rng(6)
    terms = random_terms(rng, 32, 8, 1) + [(int.from_bytes(rng.bytes(40), "little") % FR_P, [int(x) for x in rng.integers(0, 32, size=8)]) for _ in range(255)]
    assert len(terms) == _abi.CUSTOM_MAX_TERMS and sum(len(m) for _, m in terms) == _abi.CUSTOM_MAX_FACTORS
    check(dev, terms, 32, 32, rng)
    terms = [(int.from_bytes(rng.bytes(40), "little") % FR_P, [int(x) for x in rng.integers(0, 17, size=16)]) for _ in range(128)]     # the longest legal terms, 2048 factors
    check(dev, terms, 17, 16, rng)


def test_all_inputs_at_the_lazy_bound_and_two_factor_terms_with_coefficient_one(dev):
    """the magnitude argument's worst case (poly_kernels.cuh k_combine_round_custom): every value the largest representative, terms of two raw lines with coefficient 1"""
    rng = np.random.default_rng(8)
    alpha, n = 8, 256
    terms = [(1, [int(a), int(b)]) for a, b in rng.integers(0, alpha, size=(24, 2))]
    cs = descriptor(alpha, terms)
    polys = [lift(np.tile(words([FR_P - 1, 0, 1, FR_P - 2]), (n // 4, 1))) for _ in range(alpha)]
    for j, p in enumerate(polys):
        polys[j] = np.roll(p, j, axis=0)            # lo and hi differ: the lines have the steepest slopes the inputs allow
    eq = lift(np.roll(np.tile(words([0, FR_P - 1]), (n // 2, 1)), 1, axis=0))
    got_r, got_c = run(dev, cs, polys, eq, n)
    assert np.array_equal(got_r, want_round(terms, polys, eq, n, cs.degree))
    assert np.array_equal(got_c, want_claim(terms, polys, eq, n))


# ---- 9: error paths on the device (validation only: nothing is launched)

def test_invalid_descriptor_at_the_device_entry_points(dev):
    rng = np.random.default_rng(9)
    polys, eq = inputs(rng, 2, 64)
    pp = [dev.upload(p) for p in polys]; pe = dev.upload(eq)
    good = descriptor(2, [(3, [0, 1]), (1, [1])])
    try:
        before = dev.sumcheck_combine_round(good, pp, pe, 64, good.degree)
        bad = []
        b = descriptor(2, [(3, [0, 1]), (1, [1])]); b._mem[0] = 2; bad.append(b)                       # memory index out of range
        b = descriptor(2, [(3, [0, 1]), (1, [1])]); b._start[1] = 3; b._start[2] = 2; bad.append(b)    # term_start not monotone
        b = descriptor(2, [(3, [0, 1]), (1, [1])]); b.desc.num_memories = 33; bad.append(b)
        b = descriptor(2, [(3, [0, 1]), (1, [1])]); b.desc.num_terms = 0; bad.append(b)
        b = descriptor(2, [(3, [0, 1]), (1, [1])]); b.desc.coeff = None; bad.append(b)
        bad.append(descriptor(2, [(1, [0] * 17)]))                                                     # degree over the bound
        bad.append(descriptor(2, [(1, [0])] * (_abi.CUSTOM_MAX_TERMS + 1)))
        bad.append(descriptor(2, [(1, [0] * 16)] * 129))                                               # 2064 factors
        for b in bad:
            out = np.zeros((18, 4), dtype=np.uint64)
            for rc in (dev.lib.lasso_sumcheck_combine_round(dev.ctx, b.ptr(), dev._ptrs(pp), C.c_void_p(pe), 64, 3, out.ctypes.data_as(C.c_void_p)),
                       dev.lib.lasso_combine_claim(dev.ctx, b.ptr(), dev._ptrs(pp), C.c_void_p(pe), 64, out.ctypes.data_as(C.c_void_p))):
                assert rc == -1                                                                        # LASSO_ERR_INVALID
                assert dev.lib.lasso_last_error(dev.ctx).decode().startswith("custom strategy:")
            assert not out.any()
        with pytest.raises(LassoError):
            dev.sumcheck_combine_round(good, pp, pe, 64, good.degree + 1)                              # a degree that is not the descriptor's
        assert np.array_equal(dev.sumcheck_combine_round(good, pp, pe, 64, good.degree), before)       # the context is usable, the cached term list intact
    finally:
        for p in pp + [pe]:
            dev.free(p)


# ---- 6 .. 8: whole proofs

@pytest.fixture(scope="module")
def hosts():
    from lasso_amd import HostProver
    made = {}

    def get(curve):
        if curve not in made:
            made[curve] = HostProver(curve=curve)
        return made[curve]
    yield get
    for h in made.values():
        h.close()


def _instance(hp, c, log_m, lookups, seed):
    s = 1 << max((lookups - 1).bit_length(), 0)
    idx = np.ascontiguousarray(np.random.default_rng(seed).integers(0, 1 << log_m, size=(lookups, c), dtype=np.uint64))
    return s, idx, hp.gen_random_point(max(s.bit_length() - 1, 0))


def _prove(hp, S, c, log_m, alpha, s, idx, r):
    gens = hp.gens(c, s, alpha, log_m); dense = hp.densify(idx, log_m)
    try:
        return gens, hp.commit(dense, gens), hp.prove(dense, gens, S, r)
    finally:
        hp.free(dense)


# the shapes of the CPU test at 2^10 .. 2^14, then Spark C = 4 at 2^20 and LT C = 16 at 2^12 (the longest terms)
PARITY = [("and", 1, 16, 0, 1 << 14), ("and", 4, 8, 0, 1 << 12), ("or", 2, 8, 0, 1 << 10), ("xor", 8, 4, 0, 1 << 11), ("lt", 2, 8, 0, 1 << 13), ("lt", 4, 4, 0, 1 << 10),
          ("range", 4, 4, 6, 1 << 12), ("spark", 4, 8, 0, 1 << 12)]
BIG = [("spark", 4, 16, 0, 1 << 20), ("lt", 16, 4, 0, 1 << 12)]


def _parity(hp, curve, kind, c, log_m, log_r, lookups):
    alpha = 2 * c if kind == "lt" else c
    s, idx, r = _instance(hp, c, log_m, lookups, seed=lookups + c)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    g0, comm0, proof0 = _prove(hp, S, c, log_m, alpha, s, idx, r)
    hp.free(gens=g0)
    cs = U.builtin_as_custom(kind, c, log_m, log_r, curve, host=hp)
    gens, comm, proof = _prove(hp, cs, c, log_m, cs.num_memories, s, idx, r)
    try:
        assert comm == comm0, "commitment differs from the built-in's"
        assert proof == proof0, "proof differs from the built-in's"
        if lookups <= 1 << 14:
            assert hp.verify(gens, cs, s, r, proof, comm) is True
    finally:
        hp.free(gens=gens)


@pytest.mark.parametrize("curve", ["curve25519", "bn254"])
@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", PARITY)
def test_custom_as_builtin_proves_the_builtin_bytes(hosts, curve, kind, c, log_m, log_r, lookups):
    _parity(hosts(curve), curve, kind, c, log_m, log_r, lookups)


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", BIG)
def test_custom_as_builtin_large_shapes(hosts, kind, c, log_m, log_r, lookups):
    _parity(hosts("curve25519"), "curve25519", kind, c, log_m, log_r, lookups)


@pytest.mark.parametrize("kind,c,log_m,log_r,lookups", [("spark", 4, 8, 0, 1 << 12), ("and", 2, 8, 0, 1 << 12)])
def test_custom_as_builtin_in_capacity_mode(kind, c, log_m, log_r, lookups):
    from lasso_amd import HostProver
    hp = HostProver()
    try:
        hp.set_capacity(True)
        _parity(hp, "curve25519", kind, c, log_m, log_r, lookups)
    finally:
        hp.close()


def _claimed_evaluation(proof):
    pos = 8 + 32 * int.from_bytes(proof[:8], "little")
    rounds = int.from_bytes(proof[pos:pos + 8], "little"); pos += 8
    for _ in range(rounds):
        pos += 8 + 32 * int.from_bytes(proof[pos:pos + 8], "little")
    return int.from_bytes(proof[pos:pos + 32], "little")


@pytest.mark.parametrize("which", ["lte", "field"])
@pytest.mark.parametrize("log_s", [12, 16])
def test_new_strategies_end_to_end(hosts, which, log_s):
    from test_custom_strategy_cpu import expected_claim
    hp = hosts("curve25519")
    c, log_m = (4, 8) if which == "lte" else (3, 8)
    cs = U.lte_strategy(c, log_m) if which == "lte" else U.field_square_strategy(c, log_m, 5)
    s, idx, r = _instance(hp, c, log_m, 1 << log_s, seed=log_s)
    gens, comm, proof = _prove(hp, cs, c, log_m, cs.num_memories, s, idx, r)
    try:
        assert hp.verify(gens, cs, s, r, proof, comm) is True
        for pos in (len(proof) // 3, len(proof) - 40):
            bad = bytearray(proof); bad[pos] ^= 4
            try:
                assert hp.verify(gens, cs, s, r, bytes(bad), comm) is False
            except LassoError:
                pass
        other = U.lte_strategy(c, log_m) if which == "lte" else U.field_square_strategy(c, log_m, 5)
        other._coeff[0][0] ^= np.uint64(1)                                # one coefficient changed: g is really used
        try:
            assert hp.verify(gens, other, s, r, proof, comm) is False
        except LassoError:
            pass
        if log_s == 12:
            values_of = (lambda sub, a: cs.table_values[sub][a]) if which == "field" else (lambda sub, a: int(cs.tables[sub][a]))
            assert _claimed_evaluation(proof) == expected_claim(cs, idx, r, s, values_of)
    finally:
        hp.free(gens=gens)


def test_linear_custom_strategy_takes_the_builtin_linear_route(hosts):
    """AND as a descriptor with u32 tables issues the launches of built-in AND, family by family (lasso_prof_get), at 2^16: the integer gather, the u32 commitment, the
    eq-weighted linear rounds and their resident tail — what keeps the headline path's speed for linear custom tables"""
    from lasso_amd import load_device_library
    hp = hosts("curve25519")
    lib = load_device_library()
    ctx = hp.ctx()
    c, log_m, lookups = 1, 16, 1 << 16
    s, idx, r = _instance(hp, c, log_m, lookups, seed=3)
    gens = hp.gens(c, s, c, log_m); dense = hp.densify(idx, log_m)
    S = _abi.Strategy(_abi.KINDS["and"], c, log_m, 0)
    cs = U.builtin_as_custom("and", c, log_m)

    def counts(strategy):
        hp.prove(dense, gens, strategy, r)          # warm: buffers sized, tables built
        assert lib.lasso_prof_reset(ctx) == 0 and lib.lasso_prof_enable(ctx, (1 << _abi.K_COUNT) - 1) == 0
        proof = hp.prove(dense, gens, strategy, r)
        out = []
        for k in range(_abi.K_COUNT):
            n = C.c_uint64(); ms = C.c_double(); b = C.c_double()
            assert lib.lasso_prof_get(ctx, k, C.byref(n), C.byref(ms), C.byref(b)) == 0
            out.append((n.value, b.value))
        assert lib.lasso_prof_enable(ctx, 0) == 0
        return proof, out
    try:
        p0, builtin = counts(S)
        p1, custom = counts(cs)
        assert p0 == p1
        assert sum(n for n, _ in builtin) > 50
        assert custom == builtin, {_abi.KERNEL_NAMES[k]: (builtin[k], custom[k]) for k in range(_abi.K_COUNT) if builtin[k] != custom[k]}
    finally:
        hp.free(dense, gens)
