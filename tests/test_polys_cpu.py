"""CPU: several caller vectors under one commitment, opened at r in one proof (include/lasso_prover_polys.h), over the mock with the three entries of
include/lasso_hip_poly.h ("poly": the 64-bit vectors are read as they are) and over the plain mock ("plain": the host lifts them), both curves.  Every comparison is exact.

  1. polys_commit == poly_commit of the merge materialised in Python, byte for byte; padding rows are the identity's encoding;
  2. polys_commit of E_i = T[dim_i] over the Lasso generators' set 2 == comm_derefs inside an oracle-made proof (AND C = 2, LT C = 2);
  3. polys_open == CombinedTableEvalProof::prove's schedule restated on a Transcript object with Python integers, then the existing poly_open of the materialised merge
     at ch || r; evals == Python-integer MLEs == polys_evaluate;
  4. polys_verify accepts, and rejects a flipped byte of proof and commitment, a changed eval, two evals swapped, k off by one under the same K;
  5. every refusal by its message;
  6. end to end: (x, y, x & y, x < y) under one commitment, both Lasso proofs and the one opening on one transcript, a verifier that holds bytes and the public x, y."""
import ctypes as C

import numpy as np
import pytest

import gensutil as GU
import polysutil as S
import polyutil as P
import valuesutil as V
import customutil as U
from lasso_amd import _abi
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver, Transcript
from proverutil import OracleSession

CURVES = S.CURVES
ROUTES = {"poly": ("poly",), "plain": ()}


@pytest.fixture(scope="module")
def hosts():
    made = {}

    def get(curve="curve25519", route="poly"):
        if (curve, route) not in made:
            made[curve, route] = HostProver(C.CDLL(S.build(curve, ROUTES[route])), curve=curve)
        return made[curve, route]
    yield get
    for hp in made.values():
        hp.close()


def _shape_id(v):
    return f"nv{v[0]}k{v[1]}"


# ---- 1: the commitment is the merge's

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=_shape_id)
def test_commitment_is_poly_commit_of_the_merge(hosts, curve, route, shape):
    hp = hosts(curve, route)
    nv, k = shape
    kap = S.kappa(k)
    pg = hp.poly_gens(nv + kap)
    try:
        for forms in S.FORMS:
            ints, vecs = S.make_vectors(nv, k, forms, curve)
            base, pbase = hp.polys_stats(), hp.poly_stats()
            comm = hp.polys_commit(pg, vecs)
            assert comm == hp.poly_commit(pg, S.merged_words(ints, curve)), forms
            assert hp.polys_stats()["vectors_committed"] == base["vectors_committed"] + k
            n64 = sum(1 for v in vecs if v.ndim == 1) if route == "poly" else 0
            assert hp.poly_stats()["u64_commit_elements"] == pbase["u64_commit_elements"] + n64 * (1 << nv)
            rows = P.split_commitment(comm)
            left = (nv + kap) // 2
            per = 1 << (left - kap)
            assert len(rows) == 1 << left
            identity = (b"\x01" + bytes(31)) if curve == "curve25519" else (bytes(31) + b"\x40")          # ark-serialize: (0, 1) on the Edwards curve; the infinity flag on G1
            assert all(row == identity for row in rows[k * per:]) and len(rows[k * per:]) == ((1 << kap) - k) * per
            for b, v in enumerate(ints):
                if not any(v):
                    assert all(row == identity for row in rows[b * per:(b + 1) * per])
    finally:
        hp.free(poly_gens=pg)


# ---- 2: against the oracle's Subtables::commit

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", ["and", "lt"])
def test_commitment_is_comm_derefs_of_an_oracle_proof(hosts, curve, kind):
    hp = hosts(curve)
    orc_lib = GU.load_oracle(curve)
    orc_lib.orc_session_new.restype = C.c_void_p; orc_lib.orc_last_error.restype = C.c_char_p
    c, log_m, s = 2, 4, 1 << 6
    idx = V.random_indices(c, log_m, s, seed=7)
    r = hp.gen_random_point(6)
    orc = OracleSession(orc_lib, _abi.KINDS[kind], c, log_m, 0, idx, r)
    try:
        proof = orc.prove()
    finally:
        orc.close()
    desc = U.builtin_as_custom(kind, c, log_m, 0, curve)
    tables = V.table_ints(desc)
    alpha = desc.num_memories
    assert alpha == (2 * c if kind == "lt" else c)
    E = []
    for i in range(alpha):
        sub, dim = desc.memory_map(i)
        E.append(np.array([tables[sub][int(a)] for a in idx[:, dim]], dtype=np.uint64))
    gens = hp.gens(c, s, alpha, log_m)
    pg = hp.poly_gens(6 + S.kappa(alpha), points=hp.gens_points(gens, 2))
    try:
        rows = 1 << ((6 + S.kappa(alpha)) // 2)
        assert int.from_bytes(proof[:8], "little") == rows
        assert hp.polys_commit(pg, E) == proof[:8 + 32 * rows]                    # comm_derefs: the proof's first field (surge.rs:101)
        assert hp.polys_commit(pg, [P.lift(e.tolist(), curve) for e in E]) == proof[:8 + 32 * rows]
    finally:
        hp.free(gens=gens); hp.free(poly_gens=pg)


# ---- 3: the opening is the schedule, then the existing opening of the merge

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("shape", S.SHAPES, ids=_shape_id)
def test_opening_is_the_restated_schedule_over_poly_open(hosts, curve, route, shape):
    hp = hosts(curve, route)
    nv, k = shape
    pg = hp.poly_gens(nv + S.kappa(k))
    r = hp.gen_random_point(nv)
    try:
        for forms in S.FORMS:
            ints, vecs = S.make_vectors(nv, k, forms, curve, seed=1)
            pbase = hp.poly_stats()
            proof, evals = S.open_(hp, pg, vecs, r)
            n64 = sum(1 for v in vecs if v.ndim == 1) if route == "poly" else 0
            assert hp.poly_stats()["u64_open_elements"] == pbase["u64_open_elements"] + n64 * (1 << nv)
            t, tape = S.pairs(hp, b"outer state")
            try:
                want_proof, want_evals = S.restated_open(hp, pg, ints, r, t, tape, curve)
            finally:
                t.close(); tape.close()
            assert proof == want_proof, forms
            assert S.evals_ints(evals, curve) == want_evals, forms
            assert np.array_equal(hp.polys_evaluate(vecs, r), evals), forms
    finally:
        hp.free(poly_gens=pg)


# ---- 4: the verifier

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("shape", [(3, 2), (5, 3), (5, 4)], ids=_shape_id)
def test_verify_accepts_and_rejects(hosts, curve, shape):
    hp = hosts(curve)
    nv, k = shape
    pg = hp.poly_gens(nv + S.kappa(k))
    r = hp.gen_random_point(nv)
    try:
        ints, vecs = S.make_vectors(nv, k, "mixed", curve, seed=2)
        ints[-1] = [v + 1 for v in ints[-1][:-1]] + [5]; vecs[-1] = np.array(ints[-1], dtype=np.uint64) if vecs[-1].ndim == 1 else P.lift(ints[-1], curve)          # no zero vector in the last place
        comm = hp.polys_commit(pg, vecs)
        proof, evals = S.open_(hp, pg, vecs, r)
        assert S.verify_(hp, pg, r, evals, proof, comm) is True

        def rejected(**kw):
            a = dict(r=r, evals=evals, proof=proof, comm=comm, seed=b"outer state"); a.update(kw)
            try:
                return S.verify_(hp, pg, a["r"], a["evals"], a["proof"], a["comm"], seed=a["seed"]) is False
            except LassoError:
                return True          # the flipped bit made an encoding invalid: refused while reading
        flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
        lg = int.from_bytes(proof[:8], "little")
        assert lg == (nv + S.kappa(k)) - (nv + S.kappa(k)) // 2 and len(proof) == 2 * (8 + 32 * lg) + 4 * 32
        z1_at = 2 * (8 + 32 * lg) + 64
        assert rejected(proof=flip(proof, 8 + 3)) and rejected(proof=flip(proof, z1_at)) and rejected(proof=flip(proof, z1_at + 32))
        last = k * (1 << ((nv + S.kappa(k)) // 2 - S.kappa(k))) - 1          # the last row of the last vector (behind it: identity rows, where BN254's encoding ignores all but the flag)
        assert rejected(comm=flip(comm, 8 + 5)) and rejected(comm=flip(comm, 8 + 32 * last + 7))
        e = evals.copy(); e[k - 1, 0] ^= np.uint64(1)
        assert rejected(evals=e)
        e = evals.copy(); e[[0, 1]] = e[[1, 0]]
        assert not np.array_equal(e, evals) and rejected(evals=e)
        assert rejected(seed=b"another state") and rejected(seed=None)
        # k off by one under the same K: one eval fewer (the dropped one is not zero), or one more that is not zero.  (One more that IS zero is the same statement: the
        # blocks behind k are the zero polynomial.)
        K = 1 << S.kappa(k)
        if k - 1 > K // 2:
            assert V.claim_int(evals[k - 1], curve) != 0 and rejected(evals=evals[:k - 1])
        if k + 1 <= K:
            assert rejected(evals=np.concatenate([evals, evals[:1]]))
            assert S.verify_(hp, pg, r, np.concatenate([evals, np.zeros((1, 4), dtype=np.uint64)]), proof, comm) is True
        # bytes that do not deserialize: the reader's text
        with pytest.raises(LassoError, match="trailing data"):
            S.verify_(hp, pg, r, evals, proof + b"\0", comm)
        with pytest.raises(LassoError, match="truncated|implausible"):
            S.verify_(hp, pg, r, evals, proof[:-1], comm)
        with pytest.raises(LassoError, match="trailing data|truncated|implausible"):
            S.verify_(hp, pg, r, evals, proof, comm[:-1])
        with pytest.raises(LassoError, match="wrong number of rows"):
            S.verify_(hp, pg, r, evals, proof, (1).to_bytes(8, "little") + comm[8:40])
    finally:
        hp.free(poly_gens=pg)


# ---- 5: refusals

def test_every_refusal_has_its_message(hosts):
    hp = hosts()
    lib = hp._ext("polys")
    nv, k = 3, 3
    ints, vecs = S.make_vectors(nv, k, "mixed", "curve25519")
    pg = hp.poly_gens(nv + 2)
    r = hp.gen_random_point(nv)
    try:
        with pytest.raises(LassoError, match=r"no vectors \(k = 0\)"):
            hp.polys_commit(pg, [])
        with pytest.raises(LassoError, match=r"no vectors \(k = 0\)"):
            hp.polys_evaluate([], r)
        with pytest.raises(LassoError, match=r"no vectors \(k = 0\)"):
            S.verify_(hp, pg, r, np.zeros((0, 4), dtype=np.uint64), b"\0" * 8, b"\0" * 8)
        with pytest.raises(LassoError, match="must be a power of two"):
            hp.polys_commit(pg, [v[:6] for v in vecs])
        # nv + kappa > 30: refused on the numbers alone (the pointers are never read)
        arr = (_abi.PolyVec * 3)(*[_abi.PolyVec(C.c_void_p(v.ctypes.data), 1 if v.ndim == 1 else 0, 0) for v in vecs])
        out = (C.c_uint8 * 64)(); n = C.c_size_t(); ev = np.zeros((3, 4), dtype=np.uint64)
        assert lib.lasso_host_polys_evaluate(hp.h, arr, 3, 1 << 29, r.ctypes.data_as(C.c_void_p), 29, ev.ctypes.data_as(C.c_void_p)) == -1
        assert "3 vectors of 2^29 values merge into a polynomial of 31 variables; at most 30 are offered" in hp.lib.lasso_host_last_error().decode()
        with pytest.raises(LassoError, match=r"the generators were made for 5 variables, but 2 vectors of 2\^3 values merge into a polynomial of 4 variables"):
            hp.polys_commit(pg, vecs[:2])
        with pytest.raises(LassoError, match=r"the generators were made for 5 variables, but 3 vectors of 2\^4 values merge into a polynomial of 6 variables"):
            S.open_(hp, pg, S.make_vectors(4, 3, "u64", "curve25519")[1], hp.gen_random_point(4))
        for bad_len in (2, 4, 5):
            with pytest.raises(LassoError, match=rf"the point must have log2\(s\) = 3 coordinates \(the 2 above them are challenges\), got {bad_len}"):
                S.open_(hp, pg, vecs, hp.gen_random_point(bad_len))
        with pytest.raises(LassoError, match=r"the point must have log2\(s\) = 3 coordinates"):
            hp.polys_evaluate(vecs, hp.gen_random_point(5))
        with pytest.raises(LassoError, match=r"the generators were made for 5 variables, but 3 evaluations at a point of 4 coordinates are an opening in 6"):
            S.verify_(hp, pg, hp.gen_random_point(4), np.zeros((3, 4), dtype=np.uint64), b"\0" * 8, b"\0" * 8)
        # a row of the merged matrix would span several vectors: five vectors of two values are a 4 x 4 matrix
        pg4 = hp.poly_gens(4)
        try:
            with pytest.raises(LassoError, match=r"a row of the merged matrix \(2\^2 values\) would span several vectors of 2 values"):
                hp.polys_commit(pg4, S.make_vectors(1, 5, "u64", "curve25519")[1])
            with pytest.raises(LassoError, match=r"would span several vectors"):
                hp.polys_evaluate(S.make_vectors(1, 5, "field", "curve25519")[1], hp.gen_random_point(1))
        finally:
            hp.free(poly_gens=pg4)
        # per vector, poly_check's refusals with the vector's index; raised before anything is read
        buf = np.zeros(40, dtype=np.uint64)
        good = buf.ctypes.data - buf.ctypes.data % 16 + 16

        def refused(i, values, form, on_device, text):
            a = (_abi.PolyVec * 3)(*[_abi.PolyVec(C.c_void_p(good), 1, 0) for _ in range(3)])
            a[i] = _abi.PolyVec(C.c_void_p(values), form, on_device)
            for rc in (lib.lasso_host_polys_commit(hp.h, pg, a, 3, 8, out, 64, C.byref(n)),
                       lib.lasso_host_polys_evaluate(hp.h, a, 3, 8, r.ctypes.data_as(C.c_void_p), 3, ev.ctypes.data_as(C.c_void_p))):
                assert rc == -1 and f": vector {i}: {text}" in hp.lib.lasso_host_last_error().decode(), hp.lib.lasso_host_last_error().decode()
        refused(1, None, 1, 0, "null argument")
        refused(2, good, 7, 0, "form is neither LASSO_VALUES_FR (0) nor LASSO_VALUES_U64 (1)")
        refused(0, good, 0, 2, "`on_device` is neither 0 (host) nor 1 (device)")
        refused(1, good + 4, 1, 0, "the values pointer is misaligned for its form (host memory: 8 bytes, device memory: 16 bytes)")
        refused(2, good + 8, 0, 1, "the values pointer is misaligned for its form (host memory: 8 bytes, device memory: 16 bytes)")
        assert lib.lasso_host_polys_commit(hp.h, pg, arr, 3, 8, out, 8, C.byref(n)) == -2 and n.value == 8 + 32 * 4
        with pytest.raises(LassoError, match="the vectors must have one length"):
            hp.polys_commit(pg, [vecs[0], vecs[1][:4], vecs[2]])
        with pytest.raises(LassoError, match="`s` is needed"):
            hp.polys_commit(pg, [(good, "u64")])
        with pytest.raises(LassoError, match="an array has shape"):
            hp.polys_commit(pg, [np.zeros((8, 3), dtype=np.uint64)])
    finally:
        hp.free(poly_gens=pg)
    # the generators of another host; a two-rank slab host
    other = HostProver(C.CDLL(S.build("curve25519", ("poly",))))
    try:
        og = other.poly_gens(5)
        try:
            with pytest.raises(LassoError, match="the generators belong to another host"):
                hp.polys_commit(og, vecs)
        finally:
            other.free(poly_gens=og)
        from lasso_amd.prover import ALLGATHER_FN
        og = other.poly_gens(5)
        cb = ALLGATHER_FN(lambda user, send, recv, nbytes: 1)
        other._allgather = cb
        other._chk(other.lib.lasso_host_set_comm(other.h, 0, 2, cb, None))
        for call in (lambda: other.polys_commit(og, vecs), lambda: S.open_(other, og, vecs, r), lambda: other.polys_evaluate(vecs, r),
                     lambda: S.verify_(other, og, r, np.zeros((3, 4), dtype=np.uint64), b"\0" * 8, b"\0" * 8)):
            with pytest.raises(LassoError, match=r"slab-mode host \(world > 1\)"):
                call()
        other.free(poly_gens=og)
    finally:
        other.close()


def test_a_library_without_the_header_is_refused_in_the_bindings_words(hosts):
    """_abi.PROVER_EXTENSIONS has the row, and the binding names the header when a prover library does not export it"""
    assert _abi.PROVER_EXTENSIONS["polys"][0] == "lasso_prover_polys.h"

    class Without:          # stands for a prover library built before the header existed
        lib = C.CDLL(None)
    with pytest.raises(LassoError, match=r"this prover library does not export lasso_host_polys_commit \(include/lasso_prover_polys.h\)"):
        _abi.declared_ext(Without(), "polys", _abi.PROVER_EXTENSIONS, "prover", LassoError)


# ---- 6: end to end

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ROUTES)
def test_end_to_end_two_tables_one_commitment_one_opening(hosts, curve, route):
    """AND C = 2 and LT C = 2 at log_m = 4 over the same 4-bit operands: 50 lookups padded to 2^6"""
    S.end_to_end(hosts(curve, route), curve, ("and", 2), ("lt", 2), 4, 50, 4)
