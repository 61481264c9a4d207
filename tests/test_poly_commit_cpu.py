"""CPU: a commitment to the caller's vector and its opening at a point (include/lasso_hip_poly.h, include/lasso_prover_poly.h), and the chain they close:

      commit(values)  --open at r-->  Zr  ==  the claimed_evaluation inside the Lasso proof bytes

  1. the new headers declare exactly the new names, the pinned headers none of them; both product libraries export them;
  2. fr29_mul_acc_u64 as a stand-alone program (tests/cpp/test_mul_acc_u64_host.cpp), plain and under -fsanitize=undefined, both curves; its two all-ones sums against
     Python integers;
  3. commitment rows against the oracle's MSM and point compression; label-derived generators against the oracle's stream;
  4. the 64-bit and the field form of the same integers: identical commitment and opening bytes, whichever library made them — the mock with the three device entries as
     literal loops (tests/cpp/mock_poly_wrap.cpp), a mock without them (the host lifts the integers), the plain mock;
  5. poly_verify accepts, and rejects one flipped byte in the proof, the commitment, Zr, r, and a transcript seeded differently;
  6. the end-to-end story for AND, XOR, LT, RangeCheck and Spark: a verifier that holds only bytes; a changed value opens to another Zr; the Lasso proof's bytes do not
     depend on the new calls; Zr equals values_evaluate of the lifted vector;
  7. every refusal has its message;
  8. msm_plan serves 8-byte scalars with the bucket kernel and leaves its 4- and 32-byte answers alone (tests/cpp/test_launch_plan_host.cpp walks those)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import gensutil as GU
import polyutil as P
import valuesutil as V
from lasso_amd import _abi
from lasso_amd.custom import FR_MODULUS
from lasso_amd.device import LassoError
from lasso_amd.prover import HostProver, Transcript
from test_abi_exports import header_functions

ROOT = P.ROOT
CURVES = P.CURVES
DEVICE_NAMES = ["lasso_hyrax_commit_compressed_u64", "lasso_matvec_left_u64_dev", "lasso_u64_or"]
HOST_NAMES = ["lasso_host_poly_commit", "lasso_host_poly_commitment_append", "lasso_host_poly_gens_free", "lasso_host_poly_gens_from_points", "lasso_host_poly_gens_new",
              "lasso_host_poly_open", "lasso_host_poly_stats", "lasso_host_poly_verify"]


def _library(route, curve):
    if route == "wrapped":
        return P.build_mock_prover_poly(curve)
    if route == "lift":
        return V.build_mock_prover_values(curve)          # lasso_lookup_values exists, include/lasso_hip_poly.h does not
    from proverutil import build_mock_prover
    return build_mock_prover(curve)


@pytest.fixture(scope="module")
def hosts():
    made = {}

    def get(curve="curve25519", route="wrapped"):
        if (curve, route) not in made:
            made[curve, route] = HostProver(C.CDLL(_library(route, curve)), curve=curve)
        return made[curve, route]
    yield get
    for hp in made.values():
        hp.close()


def _pairs(hp):
    return Transcript(hp.lib, b"example"), Transcript(hp.lib, b"proof", tape=True)


def _open(hp, pgens, values, r, form=None, seed=None):
    t, tape = _pairs(hp)
    if seed:
        t.append_message(b"outer protocol", seed)
    try:
        return hp.poly_open(pgens, values, r, t.pair(), tape.pair(), form=form)
    finally:
        t.close(); tape.close()


def _verify(hp, pgens, r, zr, proof, comm, seed=None):
    t = Transcript(hp.lib, b"example")
    if seed:
        t.append_message(b"outer protocol", seed)
    try:
        return hp.poly_verify(pgens, r, zr, proof, comm, t.pair())
    finally:
        t.close()


def _ints(n, seed, bits=64):
    v = np.random.default_rng(seed).integers(0, (1 << bits) - 1, size=n, dtype=np.uint64, endpoint=True)
    v[0] = (1 << bits) - 1
    if n > 2:
        v[1] = 0
    return v


# ---- 1: headers and libraries

def test_new_headers_declare_exactly_the_new_names():
    assert sorted(header_functions("lasso_hip_poly.h")) == DEVICE_NAMES
    assert sorted(header_functions("lasso_prover_poly.h")) == HOST_NAMES
    pinned = set(header_functions("lasso_hip.h")) | set(header_functions("lasso_prover.h"))
    assert not pinned & set(DEVICE_NAMES + HOST_NAMES)


@pytest.mark.parametrize("suffix", ["", "_bn254"], ids=CURVES)
def test_libraries_export_the_entries(suffix):
    import __graft_entry__ as g
    g.build()
    dev = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_hip{suffix}.so"))
    assert _abi.declare_poly(dev) == DEVICE_NAMES
    host = C.CDLL(os.path.join(ROOT, "lasso_amd", f"liblasso_prover{suffix}.so"))
    for n in HOST_NAMES:
        getattr(host, n)


# ---- 2: the integer-times-field product

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("san", [[], ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "ubsan"])
def test_mul_acc_u64_program(curve, san):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_mul_acc_u64_host_" + curve + ("_ubsan" if san else ""))
    flags = ["-DLASSO_BN254"] if curve == "bn254" else []
    subprocess.check_call(["g++", "-O1" if san else "-O2", "-std=c++17", "-Wno-unknown-pragmas", *san, *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_mul_acc_u64_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "runtime error" not in res.stderr and res.stdout.rstrip().endswith("OK"), res.stdout[-2000:] + res.stderr[-3000:]
    printed = dict(line.split(" = ") for line in res.stdout.splitlines() if " = " in line)
    # 15 (and 30) products of 2^64 - 1 with the all-ones memory word W: the s-form of W is 32 W, so the memory word of the sum is k (2^64 - 1) W mod p
    p, W, z = FR_MODULUS[curve], (1 << 256) - 1, (1 << 64) - 1
    assert int(printed["ONES15"], 16) == 15 * z * W % p
    assert int(printed["ONES30"], 16) == 30 * z * W % p
    src = open(os.path.join(ROOT, "lasso_amd", "csrc", "mont29.cuh")).read()
    assert "#define M29_U64_ACC_PERIOD 15" in src
    # the bound the header derives, on integers: a column after a carry pass, 15 products of all-ones limbs, the carry it takes during the next pass
    limb = (1 << 29) - 1
    assert limb + 15 * (2 * limb * limb + 63 * limb) + (1 << 34) < 1 << 63 <= limb + 16 * (2 * limb * limb + 63 * limb) + (1 << 34)


# ---- 3: commitment rows against the oracle

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("num_vars", [1, 2, 5, 6])
def test_commitment_rows_are_the_oracles_msm(hosts, curve, num_vars):
    hp = hosts(curve)
    orc = GU.load_oracle(curve)
    s, rows, cols = 1 << num_vars, 1 << (num_vars // 2), 1 << (num_vars - num_vars // 2)
    pts, canon = P.oracle_points(orc, cols + 2, label=b"poly test label")
    own = hp.poly_gens(num_vars, points=pts)
    by_label = hp.poly_gens(num_vars, label=b"poly test label")
    try:
        for bits in (64, 20):
            v = _ints(s, seed=num_vars + bits, bits=bits)
            comm = hp.poly_commit(own, v)
            got = P.split_commitment(comm)
            assert len(got) == rows
            for i in range(rows):
                assert got[i] == P.oracle_msm_compressed(orc, canon, v[i * cols:(i + 1) * cols].tolist(), curve), (bits, i)
            assert hp.poly_commit(by_label, v) == comm          # PolyCommitmentGens::new(num_vars, label) is the oracle's stream
            assert hp.poly_commit(own, P.lift(v.tolist(), curve)) == comm
    finally:
        hp.free(poly_gens=own); hp.free(poly_gens=by_label)


# ---- 4: forms and routes

@pytest.mark.parametrize("curve", CURVES)
def test_forms_and_routes_give_identical_bytes(hosts, curve):
    num_vars = 5
    s = 1 << num_vars
    made = {}
    for route in ("wrapped", "lift", "plain"):
        hp = hosts(curve, route)
        r = hp.gen_random_point(num_vars)
        pg = hp.poly_gens(num_vars)
        try:
            assert hp.poly_stats(reset=True)["available"] is (route == "wrapped")
            for bits in (64, 32, 7):
                v = _ints(s, seed=bits, bits=bits)
                field = P.lift(v.tolist(), curve)
                cu, cf = hp.poly_commit(pg, v), hp.poly_commit(pg, field)
                (ou, zu), (of, zf) = _open(hp, pg, v, r), _open(hp, pg, field, r)
                assert cu == cf and ou == of and np.array_equal(zu, zf), (route, bits)
                made.setdefault(bits, []).append((cu, ou, zu.tobytes()))
                assert _verify(hp, pg, r, zu, ou, cu) is True
            st = hp.poly_stats()
            assert st["u64_commit_elements"] == st["u64_open_elements"] == (3 * s if route == "wrapped" else 0)
        finally:
            hp.free(poly_gens=pg)
    for bits, got in made.items():
        assert got[0] == got[1] == got[2], bits


# ---- 5: the verifier

@pytest.mark.parametrize("curve", CURVES)
def test_verify_accepts_and_rejects_one_flipped_byte(hosts, curve):
    hp = hosts(curve)
    num_vars = 6
    v = _ints(1 << num_vars, seed=6)
    r = hp.gen_random_point(num_vars)
    pg = hp.poly_gens(num_vars)
    try:
        comm = hp.poly_commit(pg, v)
        proof, zr = _open(hp, pg, v, r, seed=b"state")
        assert _verify(hp, pg, r, zr, proof, comm, seed=b"state") is True
        assert V.claim_int(zr, curve) == V.mle_int(v.tolist(), r, curve)

        def rejected(**kw):
            args = dict(r=r, zr=zr, proof=proof, comm=comm, seed=b"state"); args.update(kw)
            try:
                return _verify(hp, pg, args["r"], args["zr"], args["proof"], args["comm"], seed=args["seed"]) is False
            except LassoError:
                return True          # the flipped bit made an encoding invalid: refused while reading
        flip = lambda b, at: b[:at] + bytes([b[at] ^ 1]) + b[at + 1:]
        lg = num_vars - num_vars // 2                      # rounds of the bullet reduction
        assert int.from_bytes(proof[:8], "little") == lg and len(proof) == 2 * (8 + 32 * lg) + 4 * 32
        z1_at = 2 * (8 + 32 * lg) + 64
        assert rejected(proof=flip(proof, 8 + 3))                   # L_vec[0]
        assert rejected(proof=flip(proof, z1_at))                   # z1
        assert rejected(proof=flip(proof, z1_at + 32))              # z2
        assert rejected(comm=flip(comm, 8 + 32 + 5))                # a row of the commitment
        zr2 = zr.copy(); zr2[0] ^= 1
        assert rejected(zr=zr2)
        r2 = r.copy(); r2[num_vars - 1, 0] ^= 1
        assert rejected(r=r2)
        assert rejected(seed=b"other state")
        assert rejected(seed=None)
        with pytest.raises(LassoError, match="trailing data"):
            _verify(hp, pg, r, zr, proof + b"\0", comm, seed=b"state")
        with pytest.raises(LassoError, match="truncated|implausible"):
            _verify(hp, pg, r, zr, proof[:-1], comm, seed=b"state")
    finally:
        hp.free(poly_gens=pg)


# ---- 6: end to end

E2E = [("and", 1, 0), ("xor", 4, 0), ("lt", 2, 0), ("range", 2, 6), ("spark", 2, 0)]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("route", ["wrapped", "lift"])
@pytest.mark.parametrize("kind,c,log_r", E2E)
def test_end_to_end_a_verifier_that_holds_only_bytes(hosts, curve, route, kind, c, log_r):
    hp = hosts(curve, route)
    P.end_to_end(hp, curve, kind, c, 4, log_r, lookups=50, expect_u64=(kind != "spark"))


# ---- 7: refusals

def test_every_refusal_has_its_message(hosts):
    hp = hosts()
    for nv in (0, 31):
        with pytest.raises(LassoError, match="num_vars must be 1 .. 30"):
            hp.poly_gens(nv)
    orc = GU.load_oracle("curve25519")
    mont, _ = P.oracle_points(orc, 7)
    with pytest.raises(LassoError, match="needs 6 points"):
        hp.poly_gens(4, points=mont[:5])
    with pytest.raises(LassoError, match="needs 6 points"):
        hp.poly_gens(4, points=mont)
    pg = hp.poly_gens(4)
    r = hp.gen_random_point(4)
    try:
        v = _ints(16, seed=1)
        with pytest.raises(LassoError, match="must be a power of two"):
            hp.poly_commit(pg, v[:12])
        with pytest.raises(LassoError, match="made for 2\\^4 values, got 8"):
            hp.poly_commit(pg, v[:8])
        with pytest.raises(LassoError, match="made for 2\\^4 values, got 32"):
            _open(hp, pg, _ints(32, seed=2), hp.gen_random_point(5))
        with pytest.raises(LassoError, match="the point must have num_vars coordinates"):
            _open(hp, pg, v, hp.gen_random_point(3))
        lib = hp._poly_fns()
        buf = np.zeros(18, dtype=np.uint64)
        out = (C.c_uint8 * 4096)(); n = C.c_size_t()
        for form in (_abi.VALUES_U64, _abi.VALUES_FR):          # refused on the pointer's value, before anything is read: 4 mod 8 in host memory, 8 mod 16 in device memory
            for ptr, on_device in ((buf.ctypes.data + 4, 0), (buf.ctypes.data - buf.ctypes.data % 16 + 8, 1)):
                assert lib.lasso_host_poly_commit(hp.h, pg, C.c_void_p(ptr), form, on_device, 16, out, 4096, C.byref(n)) == -1
                assert "misaligned for its form (host memory: 8 bytes, device memory: 16 bytes)" in hp.lib.lasso_host_last_error().decode()
        assert lib.lasso_host_poly_commit(hp.h, pg, buf.ctypes.data_as(C.c_void_p), 7, 0, 16, out, 4096, C.byref(n)) == -1
        assert "form is neither" in hp.lib.lasso_host_last_error().decode()
        assert lib.lasso_host_poly_commit(hp.h, pg, buf.ctypes.data_as(C.c_void_p), _abi.VALUES_U64, 0, 16, out, 8, C.byref(n)) == -2 and n.value == 8 + 32 * 4
        with pytest.raises(LassoError, match="an array has shape"):
            hp.poly_commit(pg, np.zeros((16, 3), dtype=np.uint64))
        comm = hp.poly_commit(pg, v)
        t = Transcript(hp.lib, b"example")
        try:
            with pytest.raises(LassoError, match="trailing data|truncated|implausible"):
                hp.poly_commitment_append(t.pair(), b"label", comm[:-1])
            with pytest.raises(LassoError, match="wrong number of rows"):
                hp.poly_verify(pg, r, np.zeros(4, dtype=np.uint64), _open(hp, pg, v, r)[0], (2).to_bytes(8, "little") + comm[8:8 + 64], t.pair())
        finally:
            t.close()
    finally:
        hp.free(poly_gens=pg)
    # a two-rank slab host
    slab = HostProver(C.CDLL(P.build_mock_prover_poly("curve25519")))
    try:
        from lasso_amd.prover import ALLGATHER_FN
        cb = ALLGATHER_FN(lambda user, send, recv, nbytes: 1)
        slab._allgather = cb
        slab._chk(slab.lib.lasso_host_set_comm(slab.h, 0, 2, cb, None))
        with pytest.raises(LassoError, match="slab-mode host \\(world > 1\\)"):
            slab.poly_gens(4)
    finally:
        slab.close()


def test_the_append_is_begin_rows_end(hosts):
    """PolyCommitment::append_to_transcript (dense_mlpoly.rs:281-289) restated with the transcript's own append_message"""
    hp = hosts()
    pg = hp.poly_gens(4)
    try:
        comm = hp.poly_commit(pg, _ints(16, seed=3))
        a, b = Transcript(hp.lib, b"t"), Transcript(hp.lib, b"t")
        try:
            hp.poly_commitment_append(a.pair(), b"comm_values", comm)
            b.append_message(b"comm_values", b"poly_commitment_begin")
            for row in P.split_commitment(comm):
                b.append_message(b"poly_commitment_share", row)
            b.append_message(b"comm_values", b"poly_commitment_end")
            assert a.challenge_bytes(b"x", 32) == b.challenge_bytes(b"x", 32)
        finally:
            a.close(); b.close()
    finally:
        hp.free(poly_gens=pg)


# ---- 8: the launch plan

@pytest.mark.parametrize("flags", [[], ["-DLASSO_BN254"]], ids=CURVES)
def test_eight_byte_scalars_take_the_bucket_kernel(flags):
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_poly_plan_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", *flags, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_poly_plan_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
