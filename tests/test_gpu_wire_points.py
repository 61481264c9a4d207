"""-m gpu: compressed points decoded on the MI355X (k_points_decompress behind lasso_points_decompress, include/lasso_hip_wire.h).
  * the kernel through Device.points_decompress on the crafted encodings of tests/wireutil.py (non-canonical coordinates, illegal flags, non-residues, the torsion points
    of edwards25519 and subgroup + torsion sums, the malleable encodings) mixed with valid points, at batch sizes around the wave and workgroup boundaries and at the
    verifier's size: status, affine limbs and canonical bytes equal the host decoder's (lasso_host_points_decompress, where = 0) — invalid encodings are data, not faults;
  * HostProver.verify with the device decoder (LASSO_WIRE_DEVICE_MIN=1) against LASSO_VERIFY_DEVICE_POINTS=0, each in a fresh process (the switches are read once):
    the same outcomes on honest and tampered proofs at 2^10, 2^16 and 2^20 lookups on both curves; the per-host counter shows which path ran."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import wireutil as W

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CURVES = ["curve25519", "bn254"]


@pytest.fixture(scope="module", params=CURVES)
def pair(request):
    from lasso_amd import Device, HostProver
    curve = request.param
    dev, hp = Device(curve=curve), HostProver(curve=curve)      # product libraries; raise if the extension or the GPU is missing
    crafted = [b for _, b, _ in W.crafted(curve)]
    valid = W.random_valid(curve, 300, seed=11)
    yield curve, dev, hp, crafted, valid
    hp.close(); dev.close()


def _batch(crafted, valid, n, seed):
    """n encodings: every crafted one (as far as n allows) scattered among valid points"""
    rng = np.random.default_rng(seed)
    enc = [valid[int(i)] for i in rng.integers(0, len(valid), size=n)]
    for b, at in zip(crafted, rng.permutation(n)[: len(crafted)]):
        enc[int(at)] = b
    return enc


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 8449])
def test_kernel_equals_host_decoder(pair, n):
    curve, dev, hp, crafted, valid = pair
    enc = _batch(crafted, valid, n, seed=n)
    if n == 1:
        enc = [crafted[-2]]      # a lone rejected encoding
    blob = b"".join(enc)
    a0, c0, s0 = hp.points_decompress(blob, where=0)
    a1, c1, s1 = dev.points_decompress(blob)
    assert np.array_equal(s1, s0), [(i, int(s1[i]), int(s0[i])) for i in np.nonzero(s1 != s0)[0][:8]]
    assert np.array_equal(a1, a0) and np.array_equal(c1, c0)
    if n >= len(crafted):
        assert set(int(x) for x in s0) >= ({0, 1, 2, 3, 4} if curve == "bn254" else {0, 2, 4, 5})      # every status the curve has is in the batch
    if n in (65, 8449):      # the same through the host library's device route, and the counter moves by n
        before = hp.wire_stats()["device_points"]
        a2, c2, s2 = hp.points_decompress(blob, where=1)
        assert np.array_equal(s2, s0) and np.array_equal(a2, a0) and np.array_equal(c2, c0)
        assert hp.wire_stats() == {"device_points": before + n, "device_available": True}


def test_crafted_statuses_on_the_device(pair):
    """each crafted encoding alone in a batch of valid points gets the status it was crafted for (the big-integer decoder's, tests/test_wire_points_cpu.py)"""
    curve, dev, hp, crafted, valid = pair
    cases = W.crafted(curve)
    blob = b"".join(valid[i % len(valid)] + b for i, (_, b, _) in enumerate(cases))
    aff, canon, status = dev.points_decompress(blob)
    for i, (name, b, st) in enumerate(cases):
        assert int(status[2 * i]) == W.OK, name
        assert int(status[2 * i + 1]) == st, name
        ref = W.decode(curve, b)
        assert (aff[2 * i + 1].tobytes(), canon[2 * i + 1].tobytes()) == (ref[1], ref[2]), name


def test_null_outputs_and_empty_batch(pair):
    import ctypes as C
    curve, dev, hp, crafted, valid = pair
    blob = b"".join(valid[:70])
    st = np.zeros(70, dtype=np.uint8)
    dev._chk(dev.lib.lasso_points_decompress(dev.ctx, blob, 70, None, None, st.ctypes.data_as(C.c_void_p)))
    assert not st.any()
    assert dev.points_decompress(b"")[2].shape == (0,)


_CHILD = r'''
import json, os, sys
sys.path.insert(0, os.path.join(os.getcwd(), "tests"))
import numpy as np
import wireutil as W
from lasso_amd import HostProver, _abi
from lasso_amd.device import LassoError
out = {}
for curve in ("curve25519", "bn254"):
    hp = HostProver(curve=curve)
    for log_s in (10, 16, 20):
        c, log_m, s = 1, 16, 1 << log_s
        idx = hp.gen_indices(s, 1 << log_m, c); r = hp.gen_random_point(log_s)
        S = _abi.Strategy(_abi.KINDS["and"], c, log_m, 0)
        gens = hp.gens(c, s, c, log_m); dense = hp.densify(idx, log_m)
        comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, S, r)
        hp.free(dense)
        pts, scs = W.walk_proof(proof, c, c); cpts = W.commitment_points(comm)
        def outcome(p, cm):
            try:
                return hp.verify(gens, S, s, r, p, cm)
            except LassoError as e:
                return str(e)
        hp.wire_stats(reset=True)
        res = {"honest": outcome(proof, comm), "device_points_after_honest": hp.wire_stats()["device_points"], "wire_points": len(pts) + len(cpts)}
        tampered = {}
        for name, o, bit in (("first-point", pts[0], 3), ("middle-point-flag", pts[len(pts) // 2], 255), ("last-point", pts[-1], 100), ("scalar", scs[len(scs) // 2], 9)):
            bad = bytearray(proof); bad[o + bit // 8] ^= 1 << (bit % 8)
            tampered[name] = outcome(bytes(bad), comm)
        badc = bytearray(comm); o = cpts[len(cpts) // 2]; badc[o + 2] ^= 4
        tampered["commitment-row"] = outcome(proof, bytes(badc))
        a, b = cpts[0], cpts[1]
        badc = bytearray(comm); badc[a:a + 32], badc[b:b + 32] = comm[b:b + 32], comm[a:a + 32]
        tampered["swapped-rows"] = outcome(proof, bytes(badc))
        tampered["truncated"] = outcome(proof[:-1], comm)
        tampered["trailing"] = outcome(proof + b"\0", comm)
        res["tampered"] = tampered
        res["device_points_total"] = hp.wire_stats()["device_points"]
        out[f"{curve}-2p{log_s}"] = res
        hp.free(None, gens)
    hp.close()
print("WIRE_RESULT " + json.dumps(out))
'''


def _child(env_extra):
    env = dict(os.environ)
    env.pop("LASSO_VERIFY_DEVICE_POINTS", None); env.pop("LASSO_WIRE_DEVICE_MIN", None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, "-c", _CHILD], env=env, cwd=ROOT, capture_output=True, text=True, timeout=900)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-4000:]
    line = [ln for ln in res.stdout.split("\n") if ln.startswith("WIRE_RESULT ")][-1]
    return json.loads(line[len("WIRE_RESULT "):])


def test_verifier_outcomes_do_not_depend_on_where_points_are_decoded():
    on = _child({"LASSO_WIRE_DEVICE_MIN": "1"})
    off = _child({"LASSO_VERIFY_DEVICE_POINTS": "0"})
    assert sorted(on) == sorted(off) == sorted(f"{c}-2p{k}" for c in CURVES for k in (10, 16, 20))
    for key in on:
        a, b = on[key], off[key]
        assert a["honest"] is True and b["honest"] is True, key
        assert a["tampered"] == b["tampered"], key
        assert all(v is not True for v in a["tampered"].values()), (key, a["tampered"])
        assert a["wire_points"] == b["wire_points"] > 0
        assert a["device_points_after_honest"] == a["wire_points"], key      # ONE call decoded every point of proof and commitment
        assert b["device_points_after_honest"] == 0 and b["device_points_total"] == 0, key
