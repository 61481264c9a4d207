"""Helpers of the vector-commitment tests (tests/test_poly_commit_cpu.py, tests/test_gpu_poly_commit.py): the CPU build of the host prover against the mock with the three
entries of include/lasso_hip_poly.h added (tests/cpp/mock_poly_wrap.cpp), Python big-integer references, and the shapes and children the GPU tests run."""
import os

import numpy as np

import valuesutil as V
from lasso_amd.custom import FR_MODULUS
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]
R = 1 << 256
M64 = (1 << 64) - 1


def build_mock_prover_poly(curve="curve25519"):
    """build_mock_prover_values' library with lasso_u64_or, lasso_hyrax_commit_compressed_u64 and lasso_matvec_left_u64_dev on top (tests/cpp/mock_poly_wrap.cpp:
    literal loops), so lasso_host_poly_commit / lasso_host_poly_open take the 64-bit route on the CPU"""
    return build_mock_prover(curve, ext=("custom", "mle", "values", "poly"))


# ---- Python integers

def lift(ints, curve):
    """integers -> (n, 4) uint64 memory words (x * 2^256 mod p), canonical"""
    p = FR_MODULUS[curve]
    return V.M.int_words([int(v) * R % p for v in ints])


def lift_array(z, curve):
    """lift() of a uint64 array without a Python big-integer product per element where the array allows it: one word row repeated (all elements equal), or rows taken
    from the table of the lifted values 0 .. 2^16 - 1"""
    z = np.asarray(z, dtype=np.uint64)
    if z.size and (z == z[0]).all():
        return np.tile(lift([int(z[0])], curve), (z.size, 1))
    if z.size > 4096 and int(z.max()) < (1 << 16):
        return lift(range(1 << 16), curve)[z.astype(np.int64)]
    return lift([int(x) for x in z], curve)


def eq_int(r_ints, p):
    """EqPolynomial(r).evals() on Python ints: r[0] <-> the top index bit"""
    ev = [1]
    for rj in r_ints:
        ev = [x for e in ev for x in (e * (1 - rj) % p, e * rj % p)]
    return ev


def matvec_int(z, L_ints, l, r, p):
    return [sum(L_ints[j] * int(z[j * r + col]) for j in range(l)) % p for col in range(r)]


def oracle_points(orc, count, label=None):
    """the first `count` points of a label's generator stream by the oracle (orc_gens): ((count, 8) uint64 Montgomery limbs as lasso_bases_create and
    lasso_host_poly_gens_from_points take them, the canonical coordinates as a flat list of 8 * count words for orc_msm)"""
    import ctypes
    import gensutil as GU
    label = label or GU.LABEL
    out = (ctypes.c_uint64 * (8 * count))()
    assert orc.orc_gens(label, ctypes.c_size_t(count - 1), out) == 0
    return GU.oracle_gens(orc, count, label), list(out)


def oracle_msm_compressed(orc, canon, scalars, curve):
    """the oracle's VariableBaseMSM over the first len(scalars) points and its serialize_compressed: 32 bytes"""
    import ctypes
    import gensutil as GU
    n, p = len(scalars), FR_MODULUS[curve]
    B = (ctypes.c_uint64 * (8 * n))(*canon[:8 * n])
    S = (ctypes.c_uint64 * (4 * n))(*[w for v in scalars for w in GU.int_limbs(int(v) * R % p)])
    o = (ctypes.c_uint64 * 8)(); buf = (ctypes.c_uint8 * 32)()
    orc.orc_msm(B, S, ctypes.c_size_t(n), o)
    orc.orc_pt_compress(o, buf)
    return bytes(buf)


def split_commitment(c):
    """[u64 L][L x 32 B] -> the rows"""
    n = int.from_bytes(c[:8], "little")
    assert len(c) == 8 + 32 * n
    return [c[8 + 32 * i: 40 + 32 * i] for i in range(n)]


# ---- what tests/test_gpu_poly_commit.py runs
PATTERN = 0xA5
TAIL = 64 << 10
MATVEC_SHAPES = [(1, 1), (1, 2), (3, 5), (7, 300), (2, 257), (1025, 2), (64, 512), (1024, 1024),
                 (32769, 3)]      # the last one: 33 rows per chunk of matvec_plan (1024 chunks), more than the carry period of 15, an odd r_size with a half-filled last lane
MATVEC_FILLS = ["zero", "ones", "random64", "random8"]
COMMIT_ROWS = [1, 3, 32, 33]
COMMIT_COLS = [1, 2, 255, 512]
COMMIT_WIDTHS = [1, 8, 16, 17, 32, 33, 64]
OR_NS = [1, 63, 64, 65, (1 << 16) + 3]


def fill(kind, n, seed):
    rng = np.random.default_rng(seed)
    if kind == "zero":
        return np.zeros(n, dtype=np.uint64)
    if kind == "ones":
        return np.full(n, M64, dtype=np.uint64)
    if kind == "random8":
        return rng.integers(0, 256, size=n, dtype=np.uint64)
    return rng.integers(0, 1 << 64, size=n, dtype=np.uint64, endpoint=False)


def width_values(bits, n, seed, mode="random"):
    """n integers below 2^bits: random with the top bit set somewhere, "equal": all the same, "top": every one 2^bits - 1"""
    top = (1 << bits) - 1
    if mode == "top":
        return np.full(n, top, dtype=np.uint64)
    rng = np.random.default_rng(seed)
    if mode == "equal":
        return np.full(n, int(rng.integers(0, top, endpoint=True, dtype=np.uint64)) | (1 << (bits - 1)), dtype=np.uint64)
    v = rng.integers(0, top, size=n, dtype=np.uint64, endpoint=True)
    v[n // 2] = top
    return v


# argv: root, curve, group ("small": shapes up to 2^16 elements and lasso_u64_or; "large": the others).  lasso_matvec_left_u64_dev against Python integers and against lasso_matvec_left_dev of the lifted array, d_out followed by a pattern; lasso_u64_or.
# Prints one JSON line.  The caller sets LASSO_POISON and LASSO_SCRATCH_GUARD (read once per process).
MATVEC_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import Device
import polyutil as P
curve, group = sys.argv[2], sys.argv[3]
p = P.FR_MODULUS[curve]
dev = Device(0, curve=curve)
cases, failures = 0, []
for (l, r) in P.MATVEC_SHAPES:
    if (l * r > (1 << 16)) != (group == "large"):
        continue
    rng = np.random.default_rng(l * 1000 + r)
    L_ints = [int.from_bytes(rng.bytes(32), "little") % p for _ in range(l)]
    L_ints[0] = p - 1
    d_L = dev.upload(P.lift(L_ints, curve))
    for kind in P.MATVEC_FILLS:
        z = P.fill(kind, l * r, seed=l + r)
        d_z = dev.upload(z)
        buf = np.full(32 * r + P.TAIL, P.PATTERN, dtype=np.uint8)
        d_out = dev.upload(buf)
        dev.matvec_left_u64_dev(d_z, d_L, l, r, d_out)
        dev.sync()
        got = dev.download(d_out, buf.shape, dtype=np.uint8)
        tag = f"matvec {l}x{r} {kind}"
        cases += 1
        if not (got[32 * r:] == P.PATTERN).all():
            failures.append(tag + ": bytes behind the r_size elements were written")
        words = got[:32 * r].view(np.uint64).reshape(r, 4)
        if P.V.words_to_ints(words, curve) != P.matvec_int(z.tolist(), L_ints, l, r, p):
            failures.append(tag + ": differs from the Python integers")
        d_zf = dev.upload(P.lift_array(z, curve))
        d_ref = dev.alloc(32 * r)
        dev.matvec_left_dev(d_zf, d_L, l, r, d_ref)
        dev.sync()
        if not np.array_equal(dev.download(d_ref, (r, 4)), words):
            failures.append(tag + ": differs from lasso_matvec_left_dev of the lifted array")
        dev.free(d_ref); dev.free(d_zf); dev.free(d_out); dev.free(d_z)
    dev.free(d_L)
for n in (P.OR_NS if group == "small" else []):
    for kind, v in (("random", P.fill("random64", n, n)), ("sparse", np.zeros(n, dtype=np.uint64)), ("zero", np.zeros(n, dtype=np.uint64))):
        if kind == "sparse":
            v[n - 1] = 1 << 63; v[0] |= 1; v[n // 2] |= 1 << 31
        d_v = dev.upload(v)
        got = dev.u64_or(d_v, n)
        dev.free(d_v)
        cases += 1
        if got != int(np.bitwise_or.reduce(v)):
            failures.append(f"u64_or n={n} {kind}: {got:#x}")
dev.sync()          # LASSO_SCRATCH_GUARD: verified here; raises if a guard is damaged
print(json.dumps({"cases": cases, "failures": failures[:20]}))
dev.close()
"""

# argv: root, curve.  lasso_hyrax_commit_compressed_u64 against lasso_hyrax_commit_compressed of the lifted array and (up to 64 columns) orc_msm rows.
COMMIT_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd import Device
import polyutil as P
import gensutil as GU
curve = sys.argv[2]
dev = Device(0, curve=curve)
orc = GU.load_oracle(curve)
pts, canon = P.oracle_points(orc, max(P.COMMIT_COLS) + 2)
bases = dev.bases_create(pts)
cases, failures, routes = 0, [], set()
for rows in P.COMMIT_ROWS:
    for cols in P.COMMIT_COLS:
        n = rows * cols
        sets = [(f"w{b}", P.width_values(b, n, seed=b + n), (1 << b) - 1) for b in P.COMMIT_WIDTHS]
        sets += [("equal40", P.width_values(40, n, 3, "equal"), (1 << 40) - 1), ("top64", P.width_values(64, n, 0, "top"), P.M64), ("top32", P.width_values(32, n, 0, "top"), (1 << 32) - 1)]
        zr = P.width_values(64, n, seed=n); zr[:cols] = 0                       # an all-zero row in front of full-width rows
        sets += [("zero_row", zr, P.M64), ("all_zero", np.zeros(n, dtype=np.uint64), 0), ("all_zero_wide_bound", np.zeros(n, dtype=np.uint64), P.M64)]
        for name, v, bound in sets:
            d_v = dev.upload(v)
            got = dev.hyrax_commit_compressed_u64(d_v, bound, rows, cols, bases)
            dev.free(d_v)
            d_f = dev.upload(P.lift([int(x) for x in v], curve))
            ref = dev.hyrax_commit_compressed(d_f, rows, cols, bases)
            dev.free(d_f)
            cases += 1
            routes.add("narrow" if bound < (1 << 32) else "wide")
            tag = f"commit {rows}x{cols} {name}"
            if not np.array_equal(got, ref):
                failures.append(tag + ": differs from lasso_hyrax_commit_compressed of the lifted array")
            if cols <= 64 and name in ("w1", "w17", "w33", "w64", "top64", "zero_row"):
                for i in range(rows):
                    row = [int(x) for x in v[i * cols:(i + 1) * cols]]
                    if not any(row):
                        continue          # the identity: held to the lifted array's commitment above
                    want = P.oracle_msm_compressed(orc, canon, row, curve)
                    if bytes(got[i]) != want:
                        failures.append(tag + f": row {i} differs from the oracle's MSM"); break
dev.sync()
print(json.dumps({"cases": cases, "failures": failures[:20], "routes": sorted(routes)}))
dev.close()
"""


# ---- the end-to-end story, over any host (mock or product library)

def end_to_end(hp, curve, kind, c, log_m, log_r, lookups, expect_u64, mock=None):
    """densify, commit, prove, values_commit (the vector stays on the device), open at the proof's r on the CONTINUED transcript and tape; then a verifier that holds only
    bytes: lasso_host_verify on its own transcript, the claim read out of the proof, poly_verify of the opening against that claim on the continued transcript.  With v[0]
    changed before committing, the opening verifies only against a Zr that differs from the claim.  The Lasso proof's bytes do not depend on the new calls; Zr equals
    values_evaluate of the lifted vector.  `mock`: a host over tests/cpp/mock_poly_wrap.cpp — commitment and (fresh-transcript) opening bytes must equal its bytes."""
    from lasso_amd.prover import Transcript
    s = 1 << max((lookups - 1).bit_length(), 0)
    nv = s.bit_length() - 1
    st = V.builtin(kind, c, log_m, log_r)
    alpha = 2 * c if kind == "lt" else c
    idx = V.random_indices(c, log_m, lookups, seed=lookups + c)
    r = hp.gen_random_point(nv)
    gens = hp.gens(c, s, alpha, log_m); pg = hp.poly_gens(nv); dense = hp.densify(idx, log_m)
    live = []

    def transcript(label=b"example", tape=False):
        live.append(Transcript(hp.lib, label, tape=tape))
        return live[-1]
    try:
        comm = hp.commit(dense, gens)
        before = hp.prove(dense, gens, st, r)
        base = hp.poly_stats()
        c_v, vec = hp.values_commit(dense, st, pg)
        try:
            assert vec.form == ("u64" if expect_u64 else "field"), vec.form
            t, tape = transcript(), transcript(b"proof", tape=True)
            proof = hp.prove_with(dense, gens, st, r, t.pair(), tape.pair())
            assert proof == before                                   # the new calls in between changed nothing
            opening, zr = hp.poly_open(pg, vec, r, t.pair(), tape.pair())
            t0, tape0 = transcript(), transcript(b"proof", tape=True)
            fresh_opening, fresh_zr = hp.poly_open(pg, vec, r, t0.pair(), tape0.pair())
        finally:
            vec.free()
        assert hp.prove(dense, gens, st, r) == before
        now = hp.poly_stats()
        grown = s if (expect_u64 and now["available"]) else 0
        assert now["u64_commit_elements"] == base["u64_commit_elements"] + grown and now["u64_open_elements"] == base["u64_open_elements"] + 2 * grown
        # the verifier: bytes only
        v = transcript()
        assert hp.verify_with(gens, st, s, r, proof, comm, v.pair()) is True
        claim = hp.claimed_evaluation(proof)
        assert np.array_equal(zr, claim) and np.array_equal(fresh_zr, claim)
        assert hp.poly_verify(pg, r, claim, opening, c_v, v.pair()) is True
        assert hp.poly_verify(pg, r, claim, opening, c_v, transcript().pair()) is False        # not the continued transcript
        assert hp.poly_verify(pg, r, claim, fresh_opening, c_v, transcript().pair()) is True
        # the vector itself: the same commitment from host memory in either form, Zr = values_evaluate
        vals = hp.lookup_values(dense, st)
        assert hp.poly_commit(pg, vals) == c_v
        assert np.array_equal(hp.values_evaluate(vals, r), zr)
        ints = V.words_to_ints(vals, curve)
        if expect_u64:
            u = hp.lookup_values(dense, st, form="u64")
            assert u.tolist() == ints and hp.poly_commit(pg, u) == c_v
        if mock is not None:
            mpg = mock.poly_gens(nv)
            mt, mtape = Transcript(mock.lib, b"example"), Transcript(mock.lib, b"proof", tape=True)
            try:
                host_vals = u if expect_u64 else vals
                assert mock.poly_commit(mpg, host_vals) == c_v
                m_open, m_zr = mock.poly_open(mpg, host_vals, r, mt.pair(), mtape.pair())
                assert m_open == fresh_opening and np.array_equal(m_zr, claim)
            finally:
                mt.close(); mtape.close(); mock.free(poly_gens=mpg)
        # v[0] changed before committing
        bad = vals.copy(); bad[0] = lift([ints[0] + 1], curve)[0]
        c_bad = hp.poly_commit(pg, bad)
        assert c_bad != c_v
        t2, tape2 = transcript(), transcript(b"proof", tape=True)
        assert hp.prove_with(dense, gens, st, r, t2.pair(), tape2.pair()) == proof
        o_bad, zr_bad = hp.poly_open(pg, bad, r, t2.pair(), tape2.pair())
        assert not np.array_equal(zr_bad, claim)
        for z, verdict in ((zr_bad, True), (claim, False)):
            v3 = transcript()
            assert hp.verify_with(gens, st, s, r, proof, comm, v3.pair()) is True
            assert hp.poly_verify(pg, r, z, o_bad, c_bad, v3.pair()) is verdict
    finally:
        for x in live:
            x.close()
        hp.free(dense, gens); hp.free(poly_gens=pg)
