"""-m gpu: label-derived generators with the candidates' arithmetic on the MI355X (k_points_from_candidates behind lasso_points_from_candidates,
include/lasso_hip_gens.h).
  * the kernel through Device.points_from_candidates on the label's stream candidates with every crafted candidate of tests/gensutil.py scattered in (limbs not below
    the modulus, coordinates without a point, the small-order starts of edwards25519, both roots over one coordinate), at batch sizes around the wave and workgroup
    boundaries and at the headline's first batch: status and affine limbs equal the host's (lasso_host_points_from_candidates, where = 0) — a candidate without a point
    is data, not a fault;
  * HostProver.gens at the headline shape in a default process against a LASSO_GENS_DEVICE=0 process (the switches are read once): the three sets byte for byte, the
    first 66 points equal to the oracle's, the counter showing which route ran, and one 2^10 proof in each with equal commitment and proof bytes."""
import ctypes as C

import numpy as np
import pytest

import gensutil as G

pytestmark = pytest.mark.gpu
CURVES = ["curve25519", "bn254"]


@pytest.fixture(scope="module", params=CURVES)
def pair(request):
    from lasso_amd import Device, HostProver
    curve = request.param
    dev, hp = Device(curve=curve), HostProver(curve=curve)      # product libraries; raise if the extension or the GPU is missing
    yield curve, dev, hp
    hp.close(); dev.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 16500])
def test_kernel_equals_host_arithmetic(pair, n):
    curve, dev, hp = pair
    limbs, greatest = G.batch(curve, n, seed=n)
    if n == 1:
        cl, cg = G.crafted_arrays(curve)
        k = [name for name, _, _, _ in G.crafted(curve)].index("p-g1")      # a lone rejected candidate
        limbs, greatest = cl[k:k + 1], cg[k:k + 1]
    a0, s0 = hp.points_from_candidates(limbs, greatest, where=0)
    a1, s1 = dev.points_from_candidates(limbs, greatest)
    assert np.array_equal(s1, s0), [(int(i), int(s1[i]), int(s0[i])) for i in np.nonzero(s1 != s0)[0][:8]]
    assert np.array_equal(a1, a0), [int(i) for i in np.nonzero((a1 != a0).any(axis=1))[0][:8]]
    if n >= len(G.crafted(curve)):
        assert set(int(x) for x in s0) == {G.OK, G.NONCANONICAL, G.NO_POINT}      # every status value is in the batch
    if n in (65, 16500):      # the same through the host library's device route, and the counter moves by n
        before = hp.gens_stats()["device_candidates"]
        a2, s2 = hp.points_from_candidates(limbs, greatest, where=1)
        assert np.array_equal(s2, s0) and np.array_equal(a2, a0)
        assert hp.gens_stats() == {"device_candidates": before + n, "available": True}


def test_crafted_statuses_on_the_device(pair):
    """each crafted candidate gets the status it was crafted for and the big-integer statement's point"""
    curve, dev, hp = pair
    cl, cg = G.crafted_arrays(curve)
    aff, status = dev.points_from_candidates(cl, cg)
    for i, (name, v, g, st) in enumerate(G.crafted(curve)):
        assert int(status[i]) == st, name
        assert aff[i].tobytes() == G.from_candidate(curve, v, g)[1], name


def test_null_out_and_empty_batch(pair):
    curve, dev, hp = pair
    limbs, greatest = G.batch(curve, 70, seed=70)
    _, want = hp.points_from_candidates(limbs, greatest, where=0)
    dev.points_from_candidates(limbs[:1], greatest[:1])      # declares the entry
    st = np.zeros(70, dtype=np.uint8)
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    dev._chk(dev.lib.lasso_points_from_candidates(dev.ctx, vp(limbs), vp(greatest), 70, None, vp(st)))
    assert np.array_equal(st, want)
    assert dev.points_from_candidates(np.zeros((0, 4), dtype=np.uint64), np.zeros(0, dtype=np.uint8))[1].shape == (0,)
    dev._chk(dev.lib.lasso_points_from_candidates(dev.ctx, None, None, 0, None, vp(st)))


HEADLINE = [1, 1 << 24, 1, 16]      # (c, s, memories, log_m): 8194 points; only the generator object is built, nothing is proved
SMALL = [1, 1 << 10, 1, 16]         # the 2^10 proof (258 points: below the default threshold, so a third process forces the device route for it)


@pytest.mark.parametrize("curve", CURVES)
def test_generators_and_proof_do_not_depend_on_the_route(curve):
    jobs = [{"shape": HEADLINE, "head": 66, "prove": None}, {"shape": SMALL, "head": 0, "prove": ["and", 1, 16, 0, 1 << 10]}]
    on = G.gens_in_child("", curve, jobs, {})
    off = G.gens_in_child("", curve, jobs, {"LASSO_GENS_DEVICE": "0"})
    forced = G.gens_in_child("", curve, jobs[1:], {"LASSO_GENS_DEVICE_MIN": "1"})
    assert on[0]["count"] == off[0]["count"] and max(on[0]["count"]) == 8194
    assert on[0]["sha256"] == off[0]["sha256"] and on[1]["sha256"] == off[1]["sha256"]
    want = G.oracle_gens(G.load_oracle(curve), 66)
    for w in range(3):
        head = np.frombuffer(bytes.fromhex(on[0]["head"][w]), dtype=np.uint64).reshape(-1, 8)
        assert np.array_equal(head, want[: head.shape[0]]) and on[0]["head"][w] == off[0]["head"][w], f"set {w}"
    assert max(len(h) for h in on[0]["head"]) == 66 * 64 * 2      # the widest set did hand over 66 points
    assert on[0]["stats"]["device_candidates"] >= 2 * 8194 and on[0]["stats"]["available"] is True
    assert off[0]["stats"] == {"device_candidates": 0, "available": True} and off[1]["stats"]["device_candidates"] == 0
    assert (on[1]["comm"], on[1]["proof"]) == (off[1]["comm"], off[1]["proof"]) == (forced[0]["comm"], forced[0]["proof"]) and len(on[1]["proof"]) > 0
    assert forced[0]["sha256"] == off[1]["sha256"] and forced[0]["stats"]["device_candidates"] >= 2 * 258
