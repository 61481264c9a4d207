"""Helpers of the tests of include/lasso_prover_blind.h (tests/test_blind_cpu.py, tests/test_gpu_blind.py): the mock builds of the host prover with the oracle harness
tests/cpp/blind_oracle.cpp linked in, the harness's two functions as Python calls, the vectors and their forms, tapes (the library's own, and one whose every draw is
zero), tamperings, and the child the GPU tests run.  Every comparison made with these is byte equality."""
import ctypes as C

import numpy as np

import polysutil as S
import polyutil as P
import valuesutil as V
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from lasso_amd.prover import DeviceVector, Transcript
from mockbuild import build_mock_prover

CURVES = P.CURVES
ROUTES = {"poly": ("custom", "mle", "values", "poly"),      # the 64-bit vectors are read as they are: lasso_hyrax_commit_compressed_u64, then the decode route
          "lift": ("custom", "mle", "values"),              # no entries of lasso_hip_poly.h: the host lifts the integers
          "plain": ()}
GENS_LABEL, T_LABEL, TAPE_LABEL = b"gens_poly", b"example", b"proof"
NUM_VARS = [1, 2, 5, 8]                                      # one row; 2 x 2; an odd split (4 rows of 8); 16 x 16
FORMS = ["field", "narrow", "wide"]                          # field elements of full width; 64-bit integers below 2^32; 64-bit integers with bit 63 set somewhere
IDENTITY = {"curve25519": b"\x01" + bytes(31), "bn254": bytes(31) + b"\x40"}


def build(curve, route="poly"):
    return build_mock_prover(curve, ext=ROUTES[route], harness=("blind_oracle.cpp",))


def make_values(nv, form, curve, seed=0):
    """(the Python integers, what the calls take: (s, 4) uint64 memory words or a (s,) uint64 array)"""
    s, p = 1 << nv, FR_MODULUS[curve]
    rng = np.random.default_rng(100 * nv + seed + FORMS.index(form))
    if form == "field":
        v = [int.from_bytes(rng.bytes(40), "little") % p for _ in range(s)]
        v[0] = p - 1
        return v, P.lift(v, curve)
    if form == "narrow":
        v = [int(x) for x in rng.integers(0, 1 << 32, size=s, dtype=np.uint64)]
        v[s - 1] = (1 << 32) - 1
    else:
        v = [int(x) for x in rng.integers(0, 1 << 64, size=s, dtype=np.uint64, endpoint=False)]
        v[s - 1] = 1 << 63
    return v, np.array(v, dtype=np.uint64)


def scalar(x, curve):
    """one field element as (4,) uint64 memory words"""
    return P.lift([x % FR_MODULUS[curve]], curve)[0]


def resident(hp, arr):
    """`arr` uploaded into a DeviceVector of the host's context (the mock's device memory is host memory): free() it"""
    dv = DeviceVector(hp, "u64" if arr.ndim == 1 else "field", arr.shape[0])
    hp._ext("poly").lasso_upload.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t]
    hp._chk(hp.lib.lasso_upload(C.c_void_p(hp.ctx()), C.c_void_p(dv.ptr), arr.ctypes.data_as(C.c_void_p), C.c_size_t(arr.nbytes)))
    return dv


class Live:
    """transcripts and tapes of one test, closed together"""

    def __init__(self, hp):
        self.hp, self.made = hp, []

    def t(self, label=T_LABEL, seed=None):
        x = Transcript(self.hp.lib, label)
        if seed:
            x.append_message(b"outer protocol", seed)
        self.made.append(x)
        return x.pair()

    def tape(self, label=TAPE_LABEL):
        self.made.append(Transcript(self.hp.lib, label, tape=True))
        return self.made[-1].pair()

    def close(self):
        for x in self.made:
            x.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class ZeroTape:
    """a tape whose every draw is zero: the callbacks of lasso_transcript_vtbl in Python.  pair() as Transcript.pair()"""

    def __init__(self):
        def challenge(user, label, label_len, out, n):
            C.memset(out, 0, n)
        self._fns = (_abi.APPEND_FN(lambda *a: None), _abi.CHALLENGE_FN(challenge))
        self._vt = _abi.TranscriptVtbl(*self._fns)

    def pair(self):
        return (C.pointer(self._vt), C.c_void_p(0))


# ---- the oracle harness

def _words(a):
    a = np.ascontiguousarray(a, dtype=np.uint64)
    return a, a.ctypes.data_as(C.c_void_p)


def oracle_commit_open(lib, curve, nv, ints, r, with_blinds, blind_Zr=None, t_label=T_LABEL, tape_label=TAPE_LABEL, gens_label=GENS_LABEL):
    """blind_orc_commit_open: {"blinds": (L, 4) uint64, "commitment": lasso_host_poly_commit's layout, "Zr": (4,) uint64, "C_Zr": 32 bytes, "proof": bytes}"""
    L = 1 << (nv // 2)
    z, zp = _words(P.lift(ints, curve)); rr, rp = _words(r)
    bz = bzp = None
    if blind_Zr is not None:
        bz, bzp = _words(blind_Zr)
    blinds = np.zeros((L, 4), dtype=np.uint64); rows = (C.c_uint8 * (32 * L))(); zr = np.zeros(4, dtype=np.uint64); c_zr = (C.c_uint8 * 32)()
    cap = 1 << 16
    proof = (C.c_uint8 * cap)(); n = C.c_size_t()
    fn = lib.blind_orc_commit_open
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_char_p, C.c_char_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t,
                   C.POINTER(C.c_size_t)]
    assert fn(gens_label, nv, zp, rp, 1 if with_blinds else 0, bzp, t_label, tape_label, blinds.ctypes.data_as(C.c_void_p), rows, zr.ctypes.data_as(C.c_void_p), c_zr, proof, cap, C.byref(n)) == 0
    return {"blinds": blinds, "commitment": L.to_bytes(8, "little") + bytes(rows), "Zr": zr, "C_Zr": bytes(c_zr), "proof": bytes(proof[:n.value])}


def oracle_verify(lib, nv, r, c_zr, proof, commitment, t_label=T_LABEL, gens_label=GENS_LABEL):
    """blind_orc_verify: True / False; bytes that do not deserialize are an AssertionError"""
    rr, rp = _words(r)
    rows = b"".join(P.split_commitment(commitment))
    fn = lib.blind_orc_verify
    fn.restype = C.c_int
    fn.argtypes = [C.c_char_p, C.c_size_t, C.c_void_p, C.c_char_p, C.c_char_p, C.c_char_p, C.c_size_t, C.c_char_p, C.c_size_t]
    rc = fn(gens_label, nv, rp, bytes(c_zr), t_label, bytes(proof), len(proof), rows, len(rows) // 32)
    assert rc in (0, 1), rc
    return rc == 1


def gen_multiples(orc, curve, right_len, which, scalars, label=GENS_LABEL):
    """scalars[i] * P as wire bytes by the ORACLE library's point arithmetic, P one of the n + 2 points [G[0 .. n), G_1, h] of the label's stream (n = right_len):
    which = "G_1" or "h".  scalars: (count, 4) uint64 memory words"""
    import gensutil as GU
    _, canon = P.oracle_points(orc, right_len + 2, label)
    at = right_len + (1 if which == "h" else 0)
    pxy = (C.c_uint64 * 8)(*canon[8 * at: 8 * (at + 1)])
    out = []
    for b in V.words_to_ints(np.asarray(scalars).reshape(-1, 4), curve):
        if b == 0:
            out.append(IDENTITY[curve]); continue
        sc = (C.c_uint64 * 4)(*GU.int_limbs(b)); o = (C.c_uint64 * 8)(); buf = (C.c_uint8 * 32)()
        orc.orc_pt_mul(pxy, sc, o); orc.orc_pt_compress(o, buf)
        out.append(bytes(buf))
    return out


# ---- one blinded commitment and opening on fresh transcripts, as a dict shaped like oracle_commit_open's

def commit_open(hp, pg, values, r, blind_Zr=None, with_blinds=True, t_label=T_LABEL, tape_label=TAPE_LABEL, committed=True):
    with Live(hp) as live:
        tape = live.tape(tape_label)
        comm, blinds = hp.poly_commit(pg, values, tape=tape)
        res = hp.poly_open(pg, values, r, live.t(t_label), tape, blinds=blinds if with_blinds else None, blind_Zr=blind_Zr, committed=committed)
    return {"blinds": blinds, "commitment": comm, "Zr": res[1], "C_Zr": res[2] if len(res) > 2 else None, "proof": res[0]}


def same(a, b):
    """the keys two such dicts differ in"""
    return [k for k in ("blinds", "commitment", "Zr", "C_Zr", "proof") if not (np.array_equal(a[k], b[k]) if isinstance(a[k], np.ndarray) else a[k] == b[k])]


def flip(b, at, bit=1):
    return b[:at] + bytes([b[at] ^ bit]) + b[at + 1:]


def verdict(call):
    """True / False of a verifier call; a tampering that makes an encoding invalid is refused while reading: False"""
    from lasso_amd.device import LassoError
    try:
        return call()
    except LassoError:
        return False


# ---- what tests/test_gpu_blind.py runs
GPU_NUM_VARS = [1, 5, 11]          # 11: L = 32 rows of 64 values, the smallest that takes the multi-row MSM kernels
GPU_POLYS = (5, 3)                 # (nv, k): mixed forms, an identity-free zero block of 2 rows

# argv: root, curve.  On the product library, for every num_vars x form x residence: commitment, blinds, opening, Zr and C_Zr equal the mock build's (same tape); the
# product verifier accepts, and rejects one tampering of each kind; blind_stats names the route; the polys case likewise.  LASSO_WIRE_DEVICE_MIN in the environment
# moves the decode route's threshold.  Prints one JSON line.
GPU_CHILD = r"""
import ctypes as C, json, sys
import numpy as np
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, sys.argv[1] + "/tests")
from lasso_amd.prover import HostProver
import blindutil as B
curve = sys.argv[2]
hp = HostProver(curve=curve)
mock = HostProver(C.CDLL(B.build(curve, "poly")), curve=curve)
assert hp.poly_stats()["available"] is True
failures, cases, routes = [], 0, {"rows_device": 0, "rows_host": 0, "wire": 0}
bz = B.scalar(0x1234567890ABCDEF1234567890ABCDEF1234567, curve)
for nv in B.GPU_NUM_VARS:
    L = 1 << (nv // 2)
    r = hp.gen_random_point(nv)
    pg, mpg = hp.poly_gens(nv), mock.poly_gens(nv)
    for form in B.FORMS:
        ints, arr = B.make_values(nv, form, curve)
        want = B.commit_open(mock, mpg, arr, r, blind_Zr=bz)
        for where in ("host", "device"):
            tag = f"nv={nv} {form} {where}"
            vec = B.resident(hp, arr) if where == "device" else arr
            base, pbase, wbase = hp.blind_stats(), hp.poly_stats(), hp.wire_stats()
            got = B.commit_open(hp, pg, vec, r, blind_Zr=bz)
            now, pnow, wnow = hp.blind_stats(), hp.poly_stats(), hp.wire_stats()
            if where == "device":
                vec.free()
            cases += 1
            diff = B.same(got, want)
            if diff:
                failures.append(tag + ": differs from the mock build in " + ", ".join(diff))
            dev, host = now["rows_device"] - base["rows_device"], now["rows_host"] - base["rows_host"]
            if (dev, host) != ((L, 0) if form == "field" else (0, L)):
                failures.append(tag + f": blind_stats grew by ({dev}, {host})")
            if form != "field" and (pnow["u64_commit_elements"] - pbase["u64_commit_elements"], pnow["u64_open_elements"] - pbase["u64_open_elements"]) != (1 << nv, 1 << nv):
                failures.append(tag + ": the 64-bit elements did not go through the 8-byte entries")
            routes["rows_device"] += dev; routes["rows_host"] += host
            routes["wire"] += wnow["device_points"] - wbase["device_points"]
        # the product verifier: acceptance, one rejection of each kind
        with B.Live(hp) as live:
            ok = hp.poly_verify_committed(pg, r, got["C_Zr"], got["proof"], got["commitment"], live.t())
            plain = B.verdict(lambda: hp.poly_verify(pg, r, got["Zr"], got["proof"], got["commitment"], live.t()))
            bad = [B.verdict(lambda: hp.poly_verify_committed(pg, r, B.flip(got["C_Zr"], 3), got["proof"], got["commitment"], live.t())),
                   B.verdict(lambda: hp.poly_verify_committed(pg, r, got["C_Zr"], B.flip(got["proof"], 8 + 3), got["commitment"], live.t())),
                   B.verdict(lambda: hp.poly_verify_committed(pg, r, got["C_Zr"], got["proof"], B.flip(got["commitment"], 8 + 5), live.t()))]
            other = got["blinds"].copy(); other[0] = B.scalar(7, curve)
            tape = live.tape()
            hp.poly_commit(pg, arr, tape=tape)
            p2, z2, c2 = hp.poly_open(pg, arr, r, live.t(), tape, blinds=other, blind_Zr=bz)
            bad.append(B.verdict(lambda: hp.poly_verify_committed(pg, r, c2, p2, got["commitment"], live.t())))
        if ok is not True or plain is not False or any(bad):
            failures.append(f"nv={nv} {form}: verdicts {ok}, {plain}, {bad}")
    hp.free(poly_gens=pg); mock.free(poly_gens=mpg)
# several vectors under one blinded commitment: mixed forms, every other vector resident on the device
nv, k = B.GPU_POLYS
kap = B.S.kappa(k)
ints, vecs = B.S.make_vectors(nv, k, "mixed", curve)
r = hp.gen_random_point(nv)
pg, mpg = hp.poly_gens(nv + kap), mock.poly_gens(nv + kap)
held = [B.resident(hp, v) if b % 2 else v for b, v in enumerate(vecs)]
with B.Live(hp) as live, B.Live(mock) as mlive:
    tape, mtape = live.tape(), mlive.tape()
    comm, blinds = hp.polys_commit(pg, held, tape=tape)
    m_comm, m_blinds = mock.polys_commit(mpg, vecs, tape=mtape)
    proof, evals = hp.polys_open(pg, held, r, live.t(seed=b"outer state"), tape, blinds=blinds)
    m_proof, m_evals = mock.polys_open(mpg, vecs, r, mlive.t(seed=b"outer state"), mtape, blinds=m_blinds)
    cases += 1
    if comm != m_comm or not np.array_equal(blinds, m_blinds) or proof != m_proof or not np.array_equal(evals, m_evals):
        failures.append("polys: differs from the mock build")
    if hp.polys_verify(pg, r, evals, proof, comm, live.t(seed=b"outer state")) is not True:
        failures.append("polys: the opening does not verify")
    if B.verdict(lambda: hp.polys_verify(pg, r, evals, proof, B.flip(comm, 8 + 32 * (len(blinds) - 1) + 5), live.t(seed=b"outer state"))) is not False:
        failures.append("polys: a flipped bit in a zero-block row is accepted")
for v in held:
    if not isinstance(v, np.ndarray):
        v.free()
hp.free(poly_gens=pg); mock.free(poly_gens=mpg)
hp._chk(hp.lib.lasso_sync(C.c_void_p(hp.ctx())))          # LASSO_SCRATCH_GUARD: verified here
print(json.dumps({"cases": cases, "failures": failures[:20], "routes": routes}))
mock.close(); hp.close()
"""
