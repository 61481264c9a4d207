"""Helpers of the tests of include/lasso_prover_polys.h (tests/test_polys_cpu.py, tests/test_gpu_polys.py): k vectors under one commitment, opened at r in one proof.
The vectors and their forms, the merge materialised in Python, CombinedTableEvalProof::prove's schedule restated on a Transcript object with Python integers, and the
end-to-end story over any host (a mock build or the product library)."""
import numpy as np

import polyutil as P
import valuesutil as V
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from lasso_amd.prover import Transcript
from mockbuild import build_mock_prover

CURVES = P.CURVES
SHAPES = [(1, 1), (1, 2), (2, 3), (3, 2), (5, 5), (9, 3)]            # (nv, k): k = 1 (no challenge), K = k and K > k, one row per vector, an odd joint variable count
GPU_SHAPES = [(1, 2), (2, 3), (3, 2), (5, 5), (9, 3), (12, 2)]       # (12, 2): 32 rows per vector
FORMS = ["u64", "field", "mixed"]
KINDS = ["random", "ones", "zero", "narrow"]                           # 2^64 - 1 everywhere, all zero, below 2^32: by position, the start moved by nv so every shape's k sees other kinds


def build(curve, ext):
    return build_mock_prover(curve, ext=ext)


def kappa(k):
    return (k - 1).bit_length()


def make_vectors(nv, k, forms, curve, seed=0):
    """k vectors of 2^nv values: ([the Python integers of vector b], [what the calls take: a (s,) uint64 array or (s, 4) uint64 memory words]).  A field-form vector
    of kind "random" holds field elements of full width, the others the lift of 64-bit integers."""
    s, p = 1 << nv, FR_MODULUS[curve]
    rng = np.random.default_rng(1000 * nv + 10 * k + seed)
    ints, vecs = [], []
    for b in range(k):
        kind = KINDS[(b + nv) % len(KINDS)]
        field = forms == "field" or (forms == "mixed" and b % 2 == 1)
        if kind == "ones":
            v = [P.M64] * s
        elif kind == "zero":
            v = [0] * s
        elif kind == "narrow":
            v = [int(x) for x in rng.integers(0, 1 << 32, size=s, dtype=np.uint64)]
        elif field:
            v = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(s)]
            v[0] = p - 1
        else:
            v = [int(x) for x in rng.integers(0, 1 << 64, size=s, dtype=np.uint64, endpoint=False)]
            v[s - 1] = P.M64
        ints.append(v)
        vecs.append(P.lift(v, curve) if field else np.array(v, dtype=np.uint64))
    return ints, vecs


def merged_words(ints, curve):
    """DensePolynomial::merge on Python integers (concatenate, zero-pad to K * s) as (K * s, 4) memory words"""
    k, s = len(ints), len(ints[0])
    flat = [x for v in ints for x in v] + [0] * (((1 << kappa(k)) - k) * s)
    return P.lift(flat, curve)


def scalar_bytes(x):
    return int(x).to_bytes(32, "little")


def restate_schedule(t, evals_int, curve):
    """CombinedTableEvalProof::prove (subtables/mod.rs:285-313) up to the PolyEvalProof, on a Transcript object with Python integers: returns (ch as integers, the joint
    claim as an integer)"""
    p = FR_MODULUS[curve]
    k = len(evals_int)
    ev = list(evals_int) + [0] * ((1 << kappa(k)) - k)
    t.append_message(b"protocol-name", b"Lasso CombinedTableEvalProof")
    t.append_message(b"evals_ops_val", b"begin_append_vector")
    for e in ev:
        t.append_message(b"evals_ops_val", scalar_bytes(e))
    t.append_message(b"evals_ops_val", b"end_append_vector")
    ch = [int.from_bytes(t.challenge_bytes(b"challenge_combine_n_to_one", 64), "little") % p for _ in range(kappa(k))]
    for c in reversed(ch):                                                # bound_poly_var_bot from the last challenge down
        ev = [(ev[2 * j] + c * (ev[2 * j + 1] - ev[2 * j])) % p for j in range(len(ev) // 2)]
    assert len(ev) == 1
    t.append_message(b"joint_claim_eval", scalar_bytes(ev[0]))
    return ch, ev[0]


def restated_open(hp, pg, ints, r, t, tape, curve):
    """the opening of the materialised merge by the schedule above and the existing poly_open at ch || r: (proof bytes, evals as integers)"""
    evals_int = [V.mle_int(v, r, curve) for v in ints]
    ch, joint = restate_schedule(t, evals_int, curve)
    r_joint = np.concatenate([P.lift(ch, curve).reshape(-1, 4), np.asarray(r, dtype=np.uint64).reshape(-1, 4)])
    proof, zr = hp.poly_open(pg, merged_words(ints, curve), r_joint, t.pair(), tape.pair())
    assert V.claim_int(zr, curve) == joint
    return proof, evals_int


def pairs(hp, seed=None):
    t, tape = Transcript(hp.lib, b"example"), Transcript(hp.lib, b"proof", tape=True)
    if seed:
        t.append_message(b"outer protocol", seed)
    return t, tape


def open_(hp, pg, vecs, r, seed=b"outer state", s=None):
    t, tape = pairs(hp, seed)
    try:
        return hp.polys_open(pg, vecs, r, t.pair(), tape.pair(), s=s)
    finally:
        t.close(); tape.close()


def verify_(hp, pg, r, evals, proof, comm, seed=b"outer state"):
    t, tape = pairs(hp, seed)
    try:
        return hp.polys_verify(pg, r, evals, proof, comm, t.pair())
    finally:
        t.close(); tape.close()


def evals_ints(evals, curve):
    return V.words_to_ints(np.asarray(evals).reshape(-1, 4), curve)


# ---- the end-to-end story, over any host

def end_to_end(hp, curve, first, second, log_m, lookups, operand_bits, device=False, mock=None):
    """Two tables over the same rows, one commitment to (x, y, v_first, v_second), both Lasso proofs on one transcript, one opening; then a verifier that holds bytes and
    the public x, y.  first / second = (kind, c); a kind without an operand layout (Spark) runs on indices of its own over the same rows.  device: the result vectors
    are written by the device and stay there (HostProver.values_vector); otherwise they come from lasso_host_lookup_values_ref.  mock: a host over the mock build whose
    commitment and opening bytes must be the same."""
    s = 1 << max((lookups - 1).bit_length(), 0)
    nv = s.bit_length() - 1
    rng = np.random.default_rng(lookups + operand_bits)
    x = np.zeros(s, dtype=np.uint64); y = np.zeros(s, dtype=np.uint64)             # the rows behind `lookups` are what densify pads with: address 0
    top = (1 << operand_bits) - 1
    x[:lookups] = rng.integers(0, top, size=lookups, dtype=np.uint64, endpoint=True); y[:lookups] = rng.integers(0, top, size=lookups, dtype=np.uint64, endpoint=True)
    x[0], y[0], x[1], y[1] = top, top, 0, top
    r = hp.gen_random_point(nv)
    pg = hp.poly_gens(nv + 2)
    live, made = [], []

    def transcript(label=b"example", tape=False):
        live.append(Transcript(hp.lib, label, tape=tape))
        return live[-1]
    tables = []
    try:
        for kind, c in (first, second):
            st = V.builtin(kind, c, log_m)
            if kind == "spark":
                idx = V.random_indices(c, log_m, lookups, seed=lookups + c)
            else:
                idx = hp.operand_indices(x[:lookups], y[:lookups], layout=hp.operand_layout(st), c=c, log_m=log_m)
            gens = hp.gens(c, s, 2 * c if kind == "lt" else c, log_m); dense = hp.densify(idx, log_m)
            made.append((dense, gens))
            form = "field" if kind == "spark" else "u64"
            host = hp.lookup_values_ref(st, idx, form=form)
            vec = hp.values_vector(dense, st) if device else host
            if device:
                made.append(vec); assert vec.form == form
            tables.append((st, dense, gens, hp.commit(dense, gens), vec, host))
        (st1, d1, g1, comm1, v1, h1), (st2, d2, g2, comm2, v2, h2) = tables
        if first[0] == "and":
            assert h1.tolist() == (x & y).tolist()
        if first[0] == "xor":
            assert h1.tolist() == (x ^ y).tolist()
        if second[0] == "lt":
            assert h2.tolist() == (x < y).astype(np.uint64).tolist()
        vecs = [x, y, v1, v2]
        base, pbase = hp.polys_stats(), hp.poly_stats()
        # the prover: one commitment appended, both proofs, one opening
        c_all = hp.polys_commit(pg, vecs)
        t, tape = transcript(), transcript(b"proof", tape=True)
        hp.poly_commitment_append(t.pair(), b"comm_columns", c_all)
        proof1 = hp.prove_with(d1, g1, st1, r, t.pair(), tape.pair())
        proof2 = hp.prove_with(d2, g2, st2, r, t.pair(), tape.pair())
        opening, evals = hp.polys_open(pg, vecs, r, t.pair(), tape.pair())
        now, pnow = hp.polys_stats(), hp.poly_stats()
        assert now == {"vectors_committed": base["vectors_committed"] + 4, "vectors_opened": base["vectors_opened"] + 4}
        wide = (2 + sum(1 for kind, _ in (first, second) if kind != "spark")) * s if pnow["available"] else 0
        assert pnow["u64_commit_elements"] == pbase["u64_commit_elements"] + wide and pnow["u64_open_elements"] == pbase["u64_open_elements"] + wide
        # the verifier: bytes, and the public x, y
        v = transcript()
        hp.poly_commitment_append(v.pair(), b"comm_columns", c_all)
        assert hp.verify_with(g1, st1, s, r, proof1, comm1, v.pair()) is True
        assert hp.verify_with(g2, st2, s, r, proof2, comm2, v.pair()) is True
        assert np.array_equal(evals[2], hp.claimed_evaluation(proof1)) and np.array_equal(evals[3], hp.claimed_evaluation(proof2))
        own = hp.polys_evaluate([x, y], r)
        assert np.array_equal(evals[:2], own)
        assert evals_ints(own, curve) == [V.mle_int(x.tolist(), r, curve), V.mle_int(y.tolist(), r, curve)]
        assert hp.polys_verify(pg, r, evals, opening, c_all, v.pair()) is True
        assert hp.polys_verify(pg, r, evals, opening, c_all, transcript().pair()) is False          # not the continued transcript
        if mock is not None:
            mpg = mock.poly_gens(nv + 2)
            mt, mtape = transcript(), transcript(b"proof", tape=True)
            ft, ftape = transcript(), transcript(b"proof", tape=True)
            try:
                assert mock.polys_commit(mpg, [x, y, h1, h2]) == c_all
                m_open, m_evals = mock.polys_open(mpg, [x, y, h1, h2], r, mt.pair(), mtape.pair())
                f_open, f_evals = hp.polys_open(pg, vecs, r, ft.pair(), ftape.pair())
                assert m_open == f_open and np.array_equal(m_evals, f_evals) and np.array_equal(f_evals, evals)
            finally:
                mock.free(poly_gens=mpg)
        # one element of the first table's results changed before committing
        bad = h1.copy()
        if bad.ndim == 1:
            bad[3] ^= np.uint64(1)
        else:
            bad[3] = P.lift([V.words_to_ints(bad[3:4], curve)[0] + 1], curve)[0]
        bad_vecs = [x, y, bad, v2]
        c_bad = hp.polys_commit(pg, bad_vecs)
        assert c_bad != c_all
        t2, tape2 = transcript(), transcript(b"proof", tape=True)
        hp.poly_commitment_append(t2.pair(), b"comm_columns", c_bad)
        for d, g, st, proof in ((d1, g1, st1, proof1), (d2, g2, st2, proof2)):          # the proofs are about the tables: their claims do not move
            assert np.array_equal(hp.claimed_evaluation(hp.prove_with(d, g, st, r, t2.pair(), tape2.pair())), hp.claimed_evaluation(proof))
        o_bad, e_bad = hp.polys_open(pg, bad_vecs, r, t2.pair(), tape2.pair())
        assert not np.array_equal(e_bad[2], hp.claimed_evaluation(proof1)) and np.array_equal(e_bad[3], evals[3])
    finally:
        for z in live:
            z.close()
        for m in made:
            if isinstance(m, tuple):
                hp.free(*m)
            else:
                m.free()
        hp.free(poly_gens=pg)


# argv: root, curve, JSON list of [nv, k].  Commitment, opening and evaluations of every shape on the product library, mixed forms, every other vector resident on the
# device (lasso_alloc), against the wrapped-mock prover library loaded beside it and Python integers; the 64-bit counter.  Prints one JSON line.
SHAPES_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd.prover import HostProver, DeviceVector
import polysutil as S
curve, shapes = sys.argv[2], json.loads(sys.argv[3])
hp = HostProver(curve=curve)
mock = HostProver(C.CDLL(S.P.build_mock_prover_poly(curve)), curve=curve)
assert hp.poly_stats()["available"] is True
failures, done = [], []
for nv, k in shapes:
    s = 1 << nv
    ints, vecs = S.make_vectors(nv, k, "mixed", curve)
    r = hp.gen_random_point(nv)
    pg, mpg = hp.poly_gens(nv + S.kappa(k)), mock.poly_gens(nv + S.kappa(k))
    resident, mixed = [], []
    for b, v in enumerate(vecs):
        if b % 2 == (nv % 2):          # on the device: by turns the 64-bit and the field vectors
            dv = DeviceVector(hp, "u64" if v.ndim == 1 else "field", s)
            hp._chk(hp.lib.lasso_upload(C.c_void_p(hp.ctx()), C.c_void_p(dv.ptr), v.ctypes.data_as(C.c_void_p), C.c_size_t(v.nbytes)))
            resident.append(dv)
            mixed.append((dv.ptr, dv.form) if b % 4 < 2 else dv)
        else:
            mixed.append(v)
    tag = f"({nv}, {k})"
    base = hp.poly_stats()
    comm = hp.polys_commit(pg, mixed, s=s)
    proof, evals = S.open_(hp, pg, mixed, r, s=s)
    now = hp.poly_stats()
    n64 = sum(1 for v in vecs if v.ndim == 1)
    if now["u64_open_elements"] != base["u64_open_elements"] + n64 * s or now["u64_commit_elements"] != base["u64_commit_elements"] + n64 * s:
        failures.append(tag + f": the 64-bit counters grew by {now['u64_commit_elements'] - base['u64_commit_elements']}, {now['u64_open_elements'] - base['u64_open_elements']}, not {n64 * s}")
    if comm != mock.polys_commit(mpg, vecs):
        failures.append(tag + ": commitment differs from the mock's")
    m_proof, m_evals = S.open_(mock, mpg, vecs, r)
    if proof != m_proof:
        failures.append(tag + ": opening differs from the mock's")
    want = [S.V.mle_int(v, r, curve) for v in ints]
    if S.evals_ints(evals, curve) != want or S.evals_ints(hp.polys_evaluate(mixed, r, s=s), curve) != want:
        failures.append(tag + ": evals differ from the Python integers")
    if S.verify_(hp, pg, r, evals, proof, comm) is not True:
        failures.append(tag + ": the opening does not verify")
    for dv in resident:
        dv.free()
    hp.free(poly_gens=pg); mock.free(poly_gens=mpg)
    done.append([nv, k])
hp._chk(hp.lib.lasso_sync(C.c_void_p(hp.ctx())))          # LASSO_SCRATCH_GUARD: verified here
print(json.dumps({"done": done, "failures": failures[:20]}))
mock.close(); hp.close()
"""

# argv: root, curve, JSON [[kind, c], [kind, c], log_m, lookups, operand_bits].  end_to_end on the product library, the result vectors never leaving the device, with the
# wrapped-mock prover library beside it.
E2E_CHILD = r"""
import ctypes as C, json, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd.prover import HostProver
import polysutil as S
curve = sys.argv[2]
first, second, log_m, lookups, bits = json.loads(sys.argv[3])
hp = HostProver(curve=curve)
mock = HostProver(C.CDLL(S.P.build_mock_prover_poly(curve)), curve=curve)
assert hp.poly_stats()["available"] is True
S.end_to_end(hp, curve, tuple(first), tuple(second), log_m, lookups, bits, device=True, mock=mock)
print(json.dumps({"done": True, "stats": hp.polys_stats()}))
mock.close(); hp.close()
"""
