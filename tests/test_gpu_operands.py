"""GPU: densify from operand columns (include/lasso_hip_operands.h) on the build LASSO_TEST_CURVE selects.
  1. k_densify_extract_operands + the shared sort / run / timestamp kernels against the mock's serial loop (densified.rs:32-57) on lasso_host_operand_indices' indices:
     dim_u32, dim, read and final bit-exact for every dimension.  Sizes: one lane, a ragged pair, the 256-thread workgroup and the 4096-element RADIX_TILE boundaries +-1,
     and several tiles; one layout per shape of the index (two operands, most significant chunk first over all 64 bits, one operand whose last dimension shifts by 64,
     a one-bit chunk); slab mode at every rank;
  2. an operand that does not fit is LASSO_ERR_INVALID and leaves the context usable (its key is clamped before anything indexes by it);
  3. densify_operands -> commit -> prove gives the index path's and the oracle prover's bytes, through the device entry (lasso_host_densify_stats) and, in a fresh process
     with LASSO_DENSIFY_OPERANDS=0, without it;
  4. operand columns that are already on the GPU (device pointers; torch tensors where torch sees the device) are used where they are, and no index array is hidden
     behind the call."""
import ctypes as C

import numpy as np
import pytest

import operandutil as U
from fieldref import CURVE
from gpuutil import load_mock
from lasso_amd import _abi
from lasso_amd.device import LassoError

pytestmark = pytest.mark.gpu
Layout = _abi.OperandLayout


@pytest.fixture(scope="module")
def devs():
    from lasso_amd import Device
    real = Device(0, curve=CURVE)
    mock = Device(0, lib=load_mock())
    yield real, mock
    real.close(); mock.close()


@pytest.fixture(scope="module")
def prover_lib():
    from lasso_amd.prover import declare_prover, load_prover_library
    return declare_prover(load_prover_library(curve=CURVE))


def _indices(prover_lib, lay, x, y, c, log_m):
    """lasso_host_operand_indices (needs no host object), held to the Python statement"""
    out = np.zeros((len(x), c), dtype=np.uint64)
    vpt = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
    assert prover_lib.lasso_host_operand_indices(C.byref(Layout(*lay)), vpt(x), vpt(y), len(x), c, log_m, vpt(out)) == 0, prover_lib.lasso_host_last_error().decode()
    return out


def _mock_densify(mock, idx, s, log_m, world=1, rank=0):
    """the mock's serial loop per dimension: [(dim_u32, dim, read, final)]"""
    n, c = idx.shape
    m = 1 << log_m
    res = []
    p_idx = mock.upload(idx)
    for dim in range(c):
        p = [mock.alloc(4 * s // world), mock.alloc(32 * s // world), mock.alloc(32 * s // world), mock.alloc(32 * m // world)]
        mock._chk(mock.lib.lasso_densify_dim_slab(mock.ctx, C.c_void_p(p_idx), n, c, dim, s, log_m, world, rank, *[C.c_void_p(q) for q in p]))
        res.append((mock.download(p[0], (s // world,), dtype=np.uint32), mock.download(p[1], (s // world, 4)), mock.download(p[2], (s // world, 4)), mock.download(p[3], (m // world, 4))))
        for q in p:
            mock.free(q)
    mock.free(p_idx)
    return res


def _real_densify(real, lay, x, y, c, s, log_m, world=1, rank=0):
    m = 1 << log_m
    res = []
    p_x = real.upload(x); p_y = real.upload(y) if y is not None else None
    try:
        for dim in range(c):
            p = [real.alloc(4 * s // world), real.alloc(32 * s // world), real.alloc(32 * s // world), real.alloc(32 * m // world)]
            try:
                real.densify_dim_operands(p_x, p_y, len(x), Layout(*lay), c, dim, s, log_m, *p, world=world, rank=rank)
                res.append((real.download(p[0], (s // world,), dtype=np.uint32), real.download(p[1], (s // world, 4)), real.download(p[2], (s // world, 4)), real.download(p[3], (m // world, 4))))
            finally:
                for q in p:
                    real.free(q)
    finally:
        real.free(p_x)
        if p_y is not None:
            real.free(p_y)
    return res


def _same(a, b):
    assert len(a) == len(b)
    for dim, (u, v) in enumerate(zip(a, b)):
        for name, p, q in zip(("dim_u32", "dim", "read", "final"), u, v):
            assert np.array_equal(p, q), (dim, name)


# (layout, C, log_m): two operands; most significant chunk first over all 64 bits (no range limit); one operand, the last dimension shifts by 64 and reads 0; a one-bit chunk
LAYOUTS = [((2, 4, 0), 3, 8), ((2, 8, 1), 8, 16), ((1, 16, 0), 5, 16), ((2, 1, 0), 1, 2)]
SIZES = [1, 2, 3, 255, 256, 257, 4095, 4096, 4097, 70000]


@pytest.mark.parametrize("n_lookups", SIZES)
@pytest.mark.parametrize("lay,c,log_m", LAYOUTS, ids=["2x4-lsb-C3", "2x8-msb-C8", "1x16-lsb-C5", "2x1-lsb-C1"])
def test_kernel_against_the_serial_loop(devs, prover_lib, lay, c, log_m, n_lookups):
    real, mock = devs
    x, y = U.operands_for(lay, c, n_lookups, np.random.default_rng(n_lookups * 13 + c))
    idx = _indices(prover_lib, lay, x, y, c, log_m)
    if n_lookups <= 5000:                                                              # the Python statement itself, where it is quick
        assert np.array_equal(idx, U.py_indices(lay, x, y, c))
    s = 1 << max((n_lookups - 1).bit_length(), 0)
    _same(_real_densify(real, lay, x, y, c, s, log_m), _mock_densify(mock, idx, s, log_m))


@pytest.mark.parametrize("mode", ["same", "sorted"])
@pytest.mark.parametrize("lay,c,log_m", LAYOUTS, ids=["2x4-lsb-C3", "2x8-msb-C8", "1x16-lsb-C5", "2x1-lsb-C1"])
def test_kernel_one_hot_address_and_sorted_operands(devs, prover_lib, lay, c, log_m, mode):
    real, mock = devs
    n_lookups = 4097
    x, y = U.operands_for(lay, c, n_lookups, np.random.default_rng(3 + c), mode=mode)
    idx = _indices(prover_lib, lay, x, y, c, log_m)
    _same(_real_densify(real, lay, x, y, c, 8192, log_m), _mock_densify(mock, idx, 8192, log_m))


@pytest.mark.parametrize("rank", [0, 1, 2, 3])
@pytest.mark.parametrize("lay,c,log_m", LAYOUTS, ids=["2x4-lsb-C3", "2x8-msb-C8", "1x16-lsb-C5", "2x1-lsb-C1"])
def test_kernel_slab_mode_every_rank(devs, prover_lib, lay, c, log_m, rank):
    real, mock = devs
    n_lookups = 4097
    x, y = U.operands_for(lay, c, n_lookups, np.random.default_rng(5 + c))
    idx = _indices(prover_lib, lay, x, y, c, log_m)
    _same(_real_densify(real, lay, x, y, c, 8192, log_m, world=4, rank=rank), _mock_densify(mock, idx, 8192, log_m, world=4, rank=rank))


def test_an_operand_that_does_not_fit(devs, prover_lib):
    """The shape of test_densify_far_out_of_range_stays_in_bounds: the call fails with its own message and the same context then densifies a valid sequence bit-exactly.
    Nothing is provoked: the key of an operand that does not fit is clamped to 0 before the sort / run kernels index by it."""
    real, mock = devs
    lay, c, log_m, n = (2, 4, 0), 3, 8, 4096
    x, y = U.operands_for(lay, c, n, np.random.default_rng(17))
    for pos, col, val in ((17, 0, (1 << 40) + 3), (n - 1, 1, 1 << 63), (n - 1, 0, 1 << 12)):
        bad = [x.copy(), y.copy()]; bad[col][pos] = val
        with pytest.raises(LassoError, match="does not fit"):
            _real_densify(real, lay, bad[0], bad[1], c, n, log_m)
        _same(_real_densify(real, lay, x, y, c, n, log_m), _mock_densify(mock, _indices(prover_lib, lay, x, y, c, log_m), n, log_m))
    with pytest.raises(LassoError, match="operands \\* chunk_bits at most log_m"):
        _real_densify(real, (2, 5, 0), x, y, c, n, log_m)
    with pytest.raises(LassoError, match="second operand column"):
        _real_densify(real, lay, x, None, c, n, log_m)


# ---------------------------------------------------------------- the whole path

# (kind, C, log_m, log_r, lookups, seed): the log_m of each is the smallest its strategy allows at that C with a chunk of a byte or a nibble per operand
WHOLE = [["and", 4, 8, 0, 1 << 10, 31], ["lt", 2, 8, 0, 1 << 8, 32], ["range", 3, 16, 40, 1 << 8, 33], ["xor", 8, 8, 0, 1 << 12, 34]]


@pytest.fixture(scope="module")
def host():
    from lasso_amd.prover import HostProver
    hp = HostProver(curve=CURVE)
    yield hp
    hp.close()


@pytest.fixture(scope="module")
def whole_reference(host, oracle):
    """per case of WHOLE: (operands, the index path's commitment and proof on this device, sha256 of both) — computed once, after checking them against the oracle prover"""
    import hashlib
    from proverutil import OracleSession
    out = []
    for kind, c, log_m, log_r, lookups, seed in WHOLE:
        S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
        lay, x, y = U.case_operands(host, kind, c, log_m, log_r, lookups, seed)
        idx = host.operand_indices(x, y, layout=lay, c=c, log_m=log_m)
        r = host.gen_random_point(lookups.bit_length() - 1)
        gens = host.gens(c, lookups, 2 * c if kind == "lt" else c, log_m)
        dense = host.densify(idx, log_m)
        comm, proof = host.commit(dense, gens), host.prove(dense, gens, S, r)
        host.free(dense)
        orc = OracleSession(oracle, _abi.KINDS[kind], c, log_m, log_r, idx, r)
        try:
            assert comm == orc.commit() and proof == orc.prove()
        finally:
            orc.close()
        out.append({"S": S, "lay": lay, "x": x, "y": y, "r": r, "gens": gens, "comm": comm, "proof": proof, "digest": hashlib.sha256(comm + proof).hexdigest()})
    yield out
    for o in out:
        host.free(gens=o["gens"])


@pytest.mark.parametrize("i", range(len(WHOLE)), ids=[f"{k}-C{c}-2p{n.bit_length() - 1}" for k, c, _, _, n, _ in WHOLE])
def test_whole_path_bytes(host, whole_reference, i):
    kind, c, log_m, log_r, lookups, _ = WHOLE[i]
    ref = whole_reference[i]
    host.densify_stats(reset=True)
    dense = host.densify_operands(ref["x"], ref["y"], layout=ref["lay"], c=c, log_m=log_m)
    try:
        assert host.densify_stats() == {"operand_dims_on_device": c, "available": True}
        comm, proof = host.commit(dense, ref["gens"]), host.prove(dense, ref["gens"], ref["S"], ref["r"])
    finally:
        host.free(dense)
    assert comm == ref["comm"] and proof == ref["proof"]
    assert host.verify(ref["gens"], ref["S"], lookups, ref["r"], proof, comm) is True


def test_whole_path_with_the_switch_off(whole_reference):
    """LASSO_DENSIFY_OPERANDS=0 in a fresh child process: the device entry exists and did not run; the same bytes"""
    got = U.run_child("", CURVE, WHOLE, {"LASSO_DENSIFY_OPERANDS": "0"})
    assert [g["stats"] for g in got] == [{"operand_dims_on_device": 0, "available": True}] * len(WHOLE)
    assert [g["digest"] for g in got] == [ref["digest"] for ref in whole_reference] and all(g["verify"] is True for g in got)


def _dev_lib():
    from lasso_amd.device import load_device_library
    return load_device_library(curve=CURVE)      # the same shared object the host library is linked against


def test_device_resident_columns(whole_reference):
    """x, y already on the device (where = 1; here put there through the host's own context, so that both runs below start from the same bytes): the same commitment and
    proof, and lasso_host_mem_stats' peak during densify_operands strictly below the peak during densify of the same instance on an equally fresh host — the index path
    holds 8 C n = 256 KiB of indices, the operand path holds nothing in their place (the 64 KiB of operands are the caller's), and nothing else differs: a condition on
    the implementation (no hidden index array), not a measurement."""
    from lasso_amd.prover import HostProver
    kind, c, log_m, log_r, lookups, _ = WHOLE[3]
    ref = whole_reference[3]
    lib = _dev_lib()
    peaks = {}
    for path in ("operands", "indices"):
        hp = HostProver(curve=CURVE)
        try:
            ctx = C.c_void_p(hp.ctx())
            cols = []
            for a in (ref["x"], ref["y"]):
                p = C.c_void_p()
                assert lib.lasso_alloc(ctx, a.nbytes, C.byref(p)) == 0 and lib.lasso_upload(ctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
                cols.append(p)
            gens = hp.gens(c, lookups, c, log_m)
            idx = hp.operand_indices(ref["x"], ref["y"], layout=ref["lay"], c=c, log_m=log_m)
            hp.mem_stats(reset=True)
            if path == "operands":
                dense = C.c_void_p()
                hp._chk(hp.lib.lasso_host_densify_operands(hp.h, C.byref(ref["lay"]), cols[0], cols[1], lookups, c, log_m, 1, C.byref(dense)))
            else:
                dense = hp.densify(idx, log_m)
            peaks[path] = hp.mem_stats()["peak_bytes"]
            if path == "operands":
                assert hp.densify_stats() == {"operand_dims_on_device": c, "available": True}
            comm, proof = hp.commit(dense, gens), hp.prove(dense, gens, ref["S"], ref["r"])
            hp.free(dense, gens)
            assert comm == ref["comm"] and proof == ref["proof"], path
            for p in cols:
                assert lib.lasso_free(ctx, p) == 0
        finally:
            hp.close()
    print(f"\npeak device bytes during densify: {peaks}")
    assert peaks["operands"] < peaks["indices"]
    assert peaks["indices"] - peaks["operands"] >= 8 * c * lookups        # the whole index array, not part of it


def test_torch_tensors_on_the_gpu(host, whole_reference):
    """HostProver.densify_operands on torch tensors that live on the GPU: used where they are (where = 1), the same bytes; what is not a contiguous int64 tensor on the
    host's device is refused before anything runs"""
    torch = pytest.importorskip("torch")
    if not torch.cuda.is_available():
        pytest.skip("torch sees no device")
    kind, c, log_m, log_r, lookups, _ = WHOLE[3]
    ref = whole_reference[3]
    tx = torch.from_numpy(ref["x"].view(np.int64)).cuda(); ty = torch.from_numpy(ref["y"].view(np.int64)).cuda()
    host.densify_stats(reset=True)
    dense = host.densify_operands(tx, ty, layout=ref["lay"], c=c, log_m=log_m)
    try:
        assert host.densify_stats() == {"operand_dims_on_device": c, "available": True}
        assert host.commit(dense, ref["gens"]) == ref["comm"] and host.prove(dense, ref["gens"], ref["S"], ref["r"]) == ref["proof"]
    finally:
        host.free(dense)
    with pytest.raises(LassoError, match="int64"):
        host.densify_operands(tx.to(torch.int32), ty.to(torch.int32), layout=ref["lay"], c=c, log_m=log_m)
    with pytest.raises(LassoError, match="int64"):
        host.densify_operands(tx[::2], ty[::2], layout=ref["lay"], c=c, log_m=log_m)
    with pytest.raises(LassoError, match="both"):
        host.densify_operands(tx, ref["y"], layout=ref["lay"], c=c, log_m=log_m)


def test_gpu_bn254_operands():
    """this module again on the BN254 build, in a child process (tests/fieldref.py reads LASSO_TEST_CURVE at import)"""
    import os
    import subprocess
    import sys
    if CURVE == "bn254":
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LASSO_TEST_CURVE="bn254")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider", "-k", "not test_gpu_bn254_operands"],
                         cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout
