"""-m gpu: the MSM over caller points (include/lasso_hip_msm.h: lasso_msm_points, lasso_msm_points_dev) on the device.  The reference is the mock Device — bases_create
on the same points plus msm, the oracle's literal loop — compared through gpuutil.compress_points, which also checks curve membership.  Points are the generators of
gpuutil.gens and their negations (computed on the Montgomery words).  Runs on the build LASSO_TEST_CURVE selects.
Sizes: the kernels work in waves of 64 lanes, workgroups of 256 threads and chunks of 1024 points per workgroup (msm_points_kernels.cuh MSMP_CHUNK): each boundary +-1,
one point, and several chunks."""
import ctypes as C

import numpy as np
import pytest

import msmutil as M
from fieldref import CURVE, L as FR_P, limbs
from gpuutil import compress_points, gens, ints, lift, load_mock, rand_fr, words
from lasso_amd import _abi
from proverutil import OracleSession

pytestmark = pytest.mark.gpu

FQ_P = 21888242871839275222246405745257275088696311157297823662689037894645226208583 if CURVE == "bn254" else 2**255 - 19
SIZES = [1, 2, 3, 63, 64, 65, 255, 256, 257, 1000, 1023, 1024, 1025, 2049, 4099]
NMAX = 1 << 13


@pytest.fixture(scope="module")
def devs():
    from lasso_amd import Device
    real = Device(0, curve=CURVE)
    mock = Device(0, lib=load_mock())
    yield real, mock
    real.close(); mock.close()


@pytest.fixture(scope="module")
def points(devs):
    """NMAX generators; odd rows negated: -(x, y) = (-x, y) on the Edwards build, (x, -y) on BN254 — Montgomery words are linear, so q - word is the word of the negation"""
    g = gens(devs[1].lib, b"gens_sparse_poly", NMAX)[:NMAX].copy()
    col = slice(4, 8) if CURVE == "bn254" else slice(0, 4)
    neg = words([(FQ_P - v) % FQ_P for v in ints(g[1::2, col])])
    g[1::2, col] = neg
    return g


def negate(pts):
    out = pts.copy()
    col = slice(4, 8) if CURVE == "bn254" else slice(0, 4)
    out[:, col] = words([(FQ_P - v) % FQ_P for v in ints(pts[:, col])])
    return out


def reference(mock, pts, sc):
    """the oracle's MSM over the rows of pts that are not all-zero (an all-zero row is the identity: it contributes nothing)"""
    keep = np.any(pts != 0, axis=1)
    if not keep.any():
        b = mock.bases_create(points_any(mock))
        out = mock.msm(b, np.zeros((1, 4), dtype=np.uint64))      # 0 * G: the identity
        mock.bases_destroy(b)
        return compress_points(mock.lib, out)[0]
    b = mock.bases_create(pts[keep])
    out = mock.msm(b, np.ascontiguousarray(sc[keep]))
    mock.bases_destroy(b)
    return compress_points(mock.lib, out)[0]


def points_any(mock):
    return gens(mock.lib, b"gens_sparse_poly", 1)[:1]


def check(devs, pts, sc):
    real, mock = devs
    got = compress_points(mock.lib, real.msm_points(pts, sc))[0]
    assert got == reference(mock, pts, sc)
    return got


@pytest.mark.parametrize("n", SIZES)
def test_sizes_random_and_edge_scalars(devs, points, n):
    rng = np.random.default_rng(1000 + n)
    sc = rand_fr(rng, n)          # n >= 8: rows 0 .. 4 are 0, p - 1, 1, p - 2 and the largest 252-bit word
    check(devs, points[:n], sc)
    sc[n // 2] = 0                # one zero scalar in the middle
    check(devs, points[:n], sc)


@pytest.mark.parametrize("n", [257, 1000])
def test_degenerate_inputs(devs, points, n):
    real, mock = devs
    rng = np.random.default_rng(n)
    P = points[:n]
    one = rand_fr(rng, 1, edge=False)
    equal = np.repeat(one, n, axis=0)
    check(devs, P, equal)                                             # all scalars equal: one bucket per window
    same_point = np.repeat(P[:1], n, axis=0)
    check(devs, same_point, rand_fr(rng, n))                          # all points the same point
    check(devs, same_point, equal)                                    # ... under equal scalars: n additions of one point to itself
    pairs = P.copy(); pairs[1::2] = negate(P[0::2])[: n // 2]         # P, -P pairs under equal scalars
    m = n - n % 2
    ident = check(devs, pairs[:m], equal[:m])
    assert ident == reference(mock, np.zeros((1, 8), dtype=np.uint64), one)      # ... sum to the identity
    half = P.copy(); half[::2] = 0                                    # half of the entries all-zero
    check(devs, half, rand_fr(rng, n))
    assert check(devs, np.zeros_like(P), rand_fr(rng, n)) == ident    # all entries all-zero
    assert check(devs, P, np.zeros((n, 4), dtype=np.uint64)) == ident  # all scalars zero
    check(devs, P, np.repeat(words([FR_P - 1]), n, axis=0))           # r - 1 everywhere (the word p - 1 as a Montgomery representative)
    from gpuutil import mont
    check(devs, P, np.repeat(words([mont(FR_P - 1)]), n, axis=0))     # ... and the scalar whose VALUE is r - 1
    sc = rand_fr(rng, n)
    lazy = lift(sc)                                                   # the largest representative below the header's bound, per element
    assert compress_points(mock.lib, real.msm_points(P, lazy))[0] == check(devs, P, sc)
    lazy2 = lift(sc, rng=rng)
    assert compress_points(mock.lib, real.msm_points(P, lazy2))[0] == reference(mock, P, sc)


def test_empty_input_is_the_identity(devs):
    real, mock = devs
    got = compress_points(mock.lib, real.msm_points(np.zeros((0, 8), dtype=np.uint64), np.zeros((0, 4), dtype=np.uint64)))[0]
    assert got == reference(mock, np.zeros((1, 8), dtype=np.uint64), np.zeros((1, 4), dtype=np.uint64))


@pytest.mark.parametrize("n", [65, 1025, 4099])
def test_agrees_with_prepared_bases_and_with_the_device_resident_form(devs, points, n):
    real, mock = devs
    rng = np.random.default_rng(7 * n)
    sc = rand_fr(rng, n)
    P = points[:n]
    want = compress_points(mock.lib, real.msm_points(P, sc))[0]
    b = real.bases_create(P)
    assert compress_points(mock.lib, real.msm(b, sc))[0] == want          # lasso_bases_create + lasso_msm on the real device
    real.bases_destroy(b)
    dp, ds = real.upload(P), real.upload(sc)
    assert compress_points(mock.lib, real.msm_points_dev(dp, ds, n))[0] == want
    real.free(dp); real.free(ds)


def test_2p17_points_scratch_is_counted_and_bounded(devs, points):
    """2^17 points (the 2^13 generators sixteen times over): equal to the MSM over the generators with sixteen-fold scalars; the scratch comes from the context
    (lasso_mem_stats) and is O(n) — 257 bytes per point plus the chunk sums, no table of 64 windows per point (8 KB), let alone the byte multiples (459 KB)"""
    real, mock = devs
    n = 16 * NMAX
    sc = rand_fr(np.random.default_rng(1), NMAX)
    live, peak = C.c_uint64(), C.c_uint64()
    real._chk(real.lib.lasso_trim(real.ctx))
    real._chk(real.lib.lasso_mem_stats(real.ctx, C.byref(live), C.byref(peak), 1))
    before = live.value
    big = real.msm_points(np.tile(points, (16, 1)), np.tile(sc, (16, 1)))
    real._chk(real.lib.lasso_mem_stats(real.ctx, C.byref(live), C.byref(peak), 0))
    assert peak.value - before <= 512 * n
    sc16 = words([16 * x % FR_P for x in ints(sc)])
    assert compress_points(mock.lib, big) == compress_points(mock.lib, real.msm_points(points, sc16))


def test_linearity_at_2p13(devs, points, oracle):
    """msm(a) + msm(b) == msm(a + b) over 2^13 points; only the three resulting points go through the oracle"""
    real, mock = devs
    n = NMAX
    rng = np.random.default_rng(99)
    a = rand_fr(rng, n, edge=False); b2 = rand_fr(rng, n, edge=False)
    s = words([(x + y) % FR_P for x, y in zip(ints(a), ints(b2))])      # Montgomery form is linear
    ca, cb, cs = (compress_points(mock.lib, real.msm_points(points, v))[0] for v in (a, b2, s))
    U8 = C.c_uint64 * 8
    xa, xb, xo = U8(), U8(), U8()
    assert oracle.orc_pt_decompress(ca, xa) == 0 and oracle.orc_pt_decompress(cb, xb) == 0
    oracle.orc_pt_add(xa, xb, xo)
    buf = (C.c_uint8 * 32)()
    oracle.orc_pt_compress(xo, buf)
    assert bytes(buf) == cs


@pytest.mark.parametrize("case", [("and", 1, 16, 0, 1 << 10), ("and", 4, 16, 0, 1 << 16)], ids=["and-c1-2p10", "and-c4-2p16"])
def test_verifier_paths(case, oracle):
    """fresh child processes (the switch is read once per process; the parent never replaces its own program): the table-free default and LASSO_VERIFY_MSM_POINTS=0 give
    the same verdicts and the same error behaviour, msm_stats proves which path ran, and the oracle's verifier agrees"""
    on = M.verify_in_child(None, CURVE, case, {"LASSO_VERIFY_MSM_POINTS": "1"})
    assert on["honest"] is True and on["tampered"] is not True
    assert on["stats_honest"] == {"points_calls": 4, "available": True}      # one MSM over commitment rows per opening, four openings per proof
    off = M.verify_in_child(None, CURVE, case, {"LASSO_VERIFY_MSM_POINTS": "0"})
    assert off["honest"] is True and off["tampered"] == on["tampered"]
    assert off["stats_honest"] == {"points_calls": 0, "available": True} and off["stats_both"]["points_calls"] == 0
    assert on["proof"] == off["proof"] and on["comm"] == off["comm"]
    r = np.array(on["r"], dtype=np.uint64).reshape(-1, 4)
    o = OracleSession(oracle, _abi.KINDS[case[0]], case[1], case[2], case[3], M.child_indices(case), r)
    try:
        assert o.verify(bytes.fromhex(on["proof"]), bytes.fromhex(on["comm"])) == 1
        try:
            want = o.verify(bytes.fromhex(on["proof"]), bytes.fromhex(on["bad_comm"]))
        except Exception:
            want = None
        assert want != 1
    finally:
        o.close()
