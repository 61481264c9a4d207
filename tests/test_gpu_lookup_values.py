"""-m gpu: lasso_lookup_values (include/lasso_hip_values.h) on the real libraries of both curves, and the identity

      MLE(values)(r)  ==  the claimed_evaluation inside the proof bytes

end to end on the product libraries.  All comparisons are exact (Python integers mod p).

  kernel      per kind a child process (tests/valuesutil.py KERNEL_CHILD) under LASSO_VALUES_NX=3, LASSO_POISON=1 and LASSO_SCRATCH_GUARD=1: n in valuesutil.GPU_NS and
              an n of at least three passes per lane (tests/test_lookup_values_cpu.py derives both from the launch plan), C in 1 / 2 / 4 / 8 (16 for LT and Spark),
              log_m in 2 / 4 / 8 / 16, addresses 0 and M - 1 at the first, last and a middle lookup, every offered form; u32 tables with entries 2^32 - 1, field tables
              of lazily reduced words (canonical output); d_out is followed by 64 KiB of a pattern that must survive; lasso_sync returns 0 at the end
  refusals    the 64-bit form where it is not offered, a shape whose weights leave 64 bits, bad arguments: a message, nothing written
  end to end  1000 and 2^12 lookups, every built-in kind and a non-linear caller-defined one: values from the device, evaluated on the device, equal the claim
              in the proof; the proof's bytes do not depend on the call; capacity mode with a compact representation (child process); the 64-bit form of AND from
              operand columns that live in GPU tensors into a GPU tensor; values_stats counts what the device wrote
After a child that did not end normally nothing more is started on the GPU by this module."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import valuesutil as V
from lasso_amd import _abi
from lasso_amd.device import LassoError

pytestmark = pytest.mark.gpu
ROOT = V.ROOT
CURVES = V.CURVES
_dead = []          # why nothing more may be started


def _child(script, args, env_extra, timeout):
    if _dead:
        pytest.fail("not started: an earlier child of this module did not end normally (" + _dead[0] + ")")
    env = dict(os.environ)
    for k in ("LASSO_VALUES_NX", "LASSO_POISON", "LASSO_SCRATCH_GUARD", "LASSO_LEAFLESS_MIN", "LASSO_CAPACITY_COMPACT"):
        env.pop(k, None)
    env.update(env_extra)
    try:
        res = subprocess.run([sys.executable, "-c", script, ROOT] + args, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired:
        _dead.append("time limit: " + " ".join(args))
        raise
    if res.returncode < 0 or res.returncode in (124, 134, 137, 139) or "illegal memory access" in res.stderr:
        _dead.append(f"exit status {res.returncode}: " + " ".join(args))
    assert res.returncode == 0, res.stdout[-1000:] + res.stderr[-3000:]
    return json.loads(res.stdout.strip().split("\n")[-1])


@pytest.fixture(scope="module")
def hosts():
    from lasso_amd.prover import HostProver
    made = {}

    def get(curve):
        if _dead:
            pytest.fail("not started: an earlier child of this module did not end normally (" + _dead[0] + ")")
        if curve not in made:
            made[curve] = HostProver(curve=curve)
        return made[curve]
    yield get
    for hp in made.values():
        hp.close()


# ---- the kernel against Python integers

@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("kind", V.GPU_KINDS)
def test_kernel_against_python_integers(kind, curve):
    out = _child(V.KERNEL_CHILD, [curve, kind], {"LASSO_VALUES_NX": str(V.GPU_NX), "LASSO_POISON": "1", "LASSO_SCRATCH_GUARD": "1"}, timeout=240)
    print(kind, curve, out["cases"], "cases;", out["refusals"])
    assert out["failures"] == []
    assert out["cases"] >= 30
    offered_everywhere = kind in ("and", "or", "xor", "lt", "range")          # at these shapes the weighted sums end below 2^(C * chunk bits) <= 2^64; a shape past the bound: the next test
    assert offered_everywhere != any(V.U64_TEXT in t for t in out["refusals"])
    if kind in ("range", "and", "or", "xor"):
        assert (kind == "range") == any("(C - 1) * inc below 64" in t for t in out["refusals"])       # RangeCheck C = 8 at log_m = 16: refused, not wrapped


# ---- refusals

@pytest.mark.parametrize("curve", CURVES)
def test_bad_arguments_are_messages_and_write_nothing(curve):
    from lasso_amd import Device
    from lasso_amd.custom import strategy_ptr
    if _dead:
        pytest.fail("not started: " + _dead[0])
    dev = Device(0, curve=curve)
    try:
        n = 10
        d_dim = [dev.upload(np.zeros(n, dtype=np.uint32)) for _ in range(2)]
        d_tab = dev.upload(np.arange(16, dtype=np.uint32))
        buf = np.full(n * 32 + 64, V.PATTERN, dtype=np.uint8)
        d_out = dev.upload(buf)
        st = strategy_ptr(V.builtin("xor", 2, 4))
        cases = [
            (lambda: dev.lookup_values(st, d_dim, [d_tab], False, n, 7, d_out), "form is neither"),
            (lambda: dev.lookup_values(st, d_dim, [d_tab], True, n, _abi.VALUES_FR, d_out), "subtables hold integers"),
            (lambda: dev.lookup_values(st, d_dim, [d_tab], False, n, _abi.VALUES_FR, d_out + 8), "16-byte aligned"),
            (lambda: dev.lookup_values(st, [d_dim[0] + 4, d_dim[1]], [d_tab], False, n, _abi.VALUES_FR, d_out), "8-byte aligned"),
            (lambda: dev.lookup_values(st, [d_dim[0], 0], [d_tab], False, n, _abi.VALUES_FR, d_out), "null"),
            (lambda: dev.lookup_values(st, d_dim, [0], False, n, _abi.VALUES_FR, d_out), "table pointer is null"),
            (lambda: dev.lookup_values(strategy_ptr(V.builtin("spark", 2, 4)), d_dim, [d_tab, d_tab], False, n, _abi.VALUES_FR, d_out), "Spark's subtables hold field elements"),
            (lambda: dev.lookup_values(strategy_ptr(_abi.Strategy(9, 2, 4, 0)), d_dim, [d_tab], False, n, _abi.VALUES_FR, d_out), "unknown strategy kind"),
            (lambda: dev.lookup_values(strategy_ptr(V.builtin("range", 5, 13, 60)), d_dim * 3, [d_tab] * 3, False, n, _abi.VALUES_U64, d_out), V.U64_TEXT),
        ]
        for call, text in cases:
            with pytest.raises(LassoError, match=text):
                call()
        dev.lookup_values(st, d_dim, [d_tab], False, 0, _abi.VALUES_FR, d_out)          # no lookups: nothing to do
        dev.sync()
        assert (dev.download(d_out, buf.shape, dtype=np.uint8) == V.PATTERN).all()
        dev.lookup_values(st, d_dim, [d_tab], False, n, _abi.VALUES_U64, d_out)          # the context is usable: address 0 everywhere -> 0 ^ 0
        dev.sync()
        got = dev.download(d_out, buf.shape, dtype=np.uint8)
        assert (got[:8 * n] == 0).all() and (got[8 * n:] == V.PATTERN).all()
        for q in d_dim + [d_tab, d_out]:
            dev.free(q)
    finally:
        dev.close()


# ---- end to end on the product libraries

E2E_KINDS = ["and", "or", "xor", "lt", "range", "spark", "lte"]


@pytest.mark.parametrize("curve", CURVES)
@pytest.mark.parametrize("lookups", [1000, 1 << 12])
@pytest.mark.parametrize("kind", E2E_KINDS)
def test_values_evaluate_to_the_claim_inside_the_proof(hosts, kind, lookups, curve):
    hp = hosts(curve)
    c, log_m = 2, 8
    st, desc = V.gpu_strategy(kind, c, log_m, curve, hp)
    base = hp.values_stats()
    assert base["available"] is True
    V.check_identity(hp, curve, kind, st, desc, V.random_indices(c, log_m, lookups, seed=lookups), log_m)
    s = 1 << (lookups - 1).bit_length()
    assert hp.values_stats()["device_lookups"] == base["device_lookups"] + s * (2 if V.u64_offered(kind, c, log_m) else 1)      # the device route ran, once per form


@pytest.mark.parametrize("curve", CURVES)
def test_the_same_in_capacity_mode_with_a_compact_representation(curve):
    out = _child(V.CAPACITY_CHILD, ["", curve, "1000"], {"LASSO_LEAFLESS_MIN": "64"}, timeout=300)
    assert out == {"compact": True, "kinds": ["and", "lt", "spark", "field_square"]}


def _and_instance():
    c, log_m, n = 4, 16, 3001
    rng = np.random.default_rng(17)
    x = rng.integers(0, 1 << 32, size=n, dtype=np.uint64); y = rng.integers(0, 1 << 32, size=n, dtype=np.uint64)
    x[:4] = [0, 2**32 - 1, 0, 2**32 - 1]; y[:4] = [0, 2**32 - 1, 2**32 - 1, 0]
    return c, log_m, n, 1 << (n - 1).bit_length(), x, y


@pytest.mark.parametrize("curve", CURVES)
def test_u64_values_of_and_from_device_resident_operands_into_device_memory(hosts, curve):
    """operand columns that live on the device (where = 1) -> densify_operands -> the 64-bit values written into device memory of the host's context (out_on_device = 1)
    -> x & y; the field form of the same vector is evaluated where it lies (values_on_device = 1).  Through the C ABI with plain device pointers, so that the check does
    not depend on torch seeing the device; the tensor form of the same flow is the next test."""
    import ctypes as C
    from lasso_amd.custom import strategy_ptr
    from lasso_amd.device import load_device_library
    hp = hosts(curve)
    lib = hp._values_fns()
    dlib = load_device_library(curve=curve)          # the same shared object the prover library is linked against: its contexts are this library's
    c, log_m, n, s, x, y = _and_instance()
    st = V.builtin("and", c, log_m)
    ctx = C.c_void_p(hp.ctx())

    def alloc(nbytes, fill=None):
        p = C.c_void_p()
        assert dlib.lasso_alloc(ctx, nbytes, C.byref(p)) == 0
        if fill is not None:
            assert dlib.lasso_upload(ctx, p, fill.ctypes.data_as(C.c_void_p), fill.nbytes) == 0
        return p

    def fetch(p, shape, dtype):
        out = np.empty(shape, dtype=dtype)
        assert dlib.lasso_download(ctx, out.ctypes.data_as(C.c_void_p), p, out.nbytes) == 0
        return out
    dx, dy = alloc(x.nbytes, x), alloc(y.nbytes, y)
    d_u64 = alloc(8 * s + V.TAIL, np.full(8 * s + V.TAIL, V.PATTERN, dtype=np.uint8))
    d_fr = alloc(32 * s + V.TAIL, np.full(32 * s + V.TAIL, V.PATTERN, dtype=np.uint8))
    dense = C.c_void_p()
    hp._chk(hp.lib.lasso_host_densify_operands(hp.h, C.byref(hp.operand_layout(st)), dx, dy, n, c, log_m, 1, C.byref(dense)))
    try:
        base = hp.values_stats()["device_lookups"]
        hp._chk(lib.lasso_host_lookup_values(hp.h, dense, strategy_ptr(st), _abi.VALUES_U64, 1, d_u64))
        hp._chk(lib.lasso_host_lookup_values(hp.h, dense, strategy_ptr(st), _abi.VALUES_FR, 1, d_fr))
        assert hp.values_stats()["device_lookups"] == base + 2 * s
        raw = fetch(d_u64, 8 * s + V.TAIL, np.uint8)
        got = raw[:8 * s].view(np.uint64)
        assert (got[:n] == (x & y)).all() and (got[n:] == 0).all() and (raw[8 * s:] == V.PATTERN).all()
        assert (fetch(d_fr, 32 * s + V.TAIL, np.uint8)[32 * s:] == V.PATTERN).all()
        r = hp.gen_random_point(s.bit_length() - 1)
        out = np.zeros(4, dtype=np.uint64)
        hp._chk(lib.lasso_host_values_evaluate(hp.h, d_fr, 1, s, r.ctypes.data_as(C.c_void_p), r.shape[0], out.ctypes.data_as(C.c_void_p)))
        ints = [int(v) for v in (x & y)] + [0] * (s - n)
        assert V.claim_int(out, curve) == V.mle_int(ints, r, curve)
        assert np.array_equal(out, hp.values_evaluate(hp.lookup_values(dense, st), r))          # the host-memory route of both calls agrees
    finally:
        hp.free(dense)
        for p in (dx, dy, d_u64, d_fr):
            assert dlib.lasso_free(ctx, p) == 0


@pytest.mark.parametrize("curve", CURVES)
def test_tensors_are_checked_and_used_where_torch_sees_the_device(hosts, curve):
    """HostProver.lookup_values(out=tensor) / values_evaluate(tensor): what is not a contiguous int64 tensor of the right shape on this host's GPU is refused with a message;
    where torch sees the device, the flow of the test above on tensors"""
    import torch
    hp = hosts(curve)
    c, log_m, n, s, x, y = _and_instance()
    st = V.builtin("and", c, log_m)
    dense = hp.densify_operands(x, y, layout=hp.operand_layout(st), c=c, log_m=log_m)
    try:
        for bad in (torch.zeros(s, dtype=torch.int64), torch.zeros(s, dtype=torch.int32)):
            with pytest.raises(LassoError, match="`out` must be a contiguous int64 tensor"):
                hp.lookup_values(dense, st, form="u64", out=bad)
        with pytest.raises(LassoError, match="a tensor must be contiguous int64 of shape"):
            hp.values_evaluate(torch.zeros((s, 4), dtype=torch.int64), hp.gen_random_point(s.bit_length() - 1))
        if not torch.cuda.is_available():
            return          # torch does not see the device here: the device-resident route itself is the test above
        dev = torch.device("cuda", hp.device)
        tx = torch.from_numpy(x.astype(np.int64)).to(dev); ty = torch.from_numpy(y.astype(np.int64)).to(dev)
        dense_t = hp.densify_operands(tx, ty, layout=hp.operand_layout(st), c=c, log_m=log_m)
        try:
            out = torch.full((s + 8,), -1, dtype=torch.int64, device=dev)
            got = hp.lookup_values(dense_t, st, form="u64", out=out[:s])
            torch.cuda.synchronize(dev)
            host = out.cpu().numpy().view(np.uint64)
            assert got.data_ptr() == out.data_ptr()
            assert (host[:n] == (x & y)).all() and (host[n:s] == 0).all() and (host[s:] == np.uint64(2**64 - 1)).all()
            field = torch.zeros((s, 4), dtype=torch.int64, device=dev)
            hp.lookup_values(dense_t, st, out=field)
            r = hp.gen_random_point(s.bit_length() - 1)
            ints = [int(v) for v in (x & y)] + [0] * (s - n)
            assert V.claim_int(hp.values_evaluate(field, r), curve) == V.mle_int(ints, r, curve)
            with pytest.raises(LassoError, match="`out` must be a contiguous int64 tensor"):
                hp.lookup_values(dense_t, st, form="u64", out=out[:s - 1])
        finally:
            hp.free(dense_t)
    finally:
        hp.free(dense)
