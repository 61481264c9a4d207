"""-m gpu: the memory-form contract of include/lasso_hip.h — every entry point accepts LAZILY REDUCED field arrays (any representative below
2^254 + 2^130) — and the field's edge values, on the real library next to the oracle's mock.

a. representation independence: each entry point that reads device field arrays runs on canonical full-field inputs (== the mock) and again with
   every field array replaced by its largest representative (gpuutil.lift); the outputs are byte-identical (canonically equal where the output is
   itself lazily reduced or a copy of the input).  d_E is also lifted on its own: the eq-weighted kernels load it in s-form.
b. edge scalars: challenges, eq points, gamma / tau, u / u^-1, scale and blinds drawn from gpuutil.EDGE, against the mock.
c. the inputs of a. and b. are uniform over the whole field (gpuutil.full_fr) with every EDGE word in front: on BN254 that reaches [2^252, p).
d. the operations that are a line of algebra against Python integers (tests/bigref.py), independent of the mock."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigref
from fieldref import L as FR_P
from gpuutil import EDGE, LAZY_BOUND, canon, compress_points, edge_fr, full_fr, gens, ints, lift, load_mock, mont, small_fr, words
from lasso_amd import _abi

pytestmark = pytest.mark.gpu

NE = len(EDGE)
I_ZERO, I_ONE, I_TWO, I_M1, I_HALF_UP = 0, 1, 2, 3, 6      # EDGE rows: Montgomery 0, 1, 2, p - 1, (p + 1) / 2 (the inverse of 2)


@pytest.fixture(scope="module")
def devs():
    from lasso_amd import Device
    from fieldref import CURVE
    real = Device(0, curve=CURVE)
    mock = Device(0, lib=load_mock())
    yield real, mock
    real.close(); mock.close()


@pytest.fixture(scope="module")
def gens_300(devs):
    return gens(devs[1].lib, b"gens_sparse_poly", 300)


def mixed(rng, n):
    """full-field rows with every EDGE word in front (as many as fit)"""
    x = full_fr(rng, n)
    k = min(n, NE)
    x[:k] = edge_fr(range(k))
    return x


def lifted(inp, keys=None):
    return {k: (lift(v) if (keys is None or k in keys) and isinstance(v, np.ndarray) and v.dtype == np.uint64 and v.shape[-1] == 4 else v)
            for k, v in inp.items()}


def same(x, y, kind, mock_lib):
    if kind == "p":
        return compress_points(mock_lib, np.asarray(x).reshape(-1, 16)) == compress_points(mock_lib, np.asarray(y).reshape(-1, 16))
    if kind == "c":
        return np.array_equal(canon(x), canon(y))
    return np.array_equal(x, y)


def check(devs, run, inp, kinds, keys=None):
    """run(d, inputs) -> list of outputs; kinds[i]: "b" bytes, "c" canonical value, "p" point.  canonical real == mock, lifted real == canonical real"""
    real, mock = devs
    want = run(mock, inp)
    got = run(real, inp)
    assert len(got) == len(want) == len(kinds)
    for i, (x, y, k) in enumerate(zip(got, want, kinds)):
        assert same(x, y, k, mock.lib), f"output {i}: device != mock on canonical inputs"
    again = run(real, lifted(inp, keys))
    for i, (x, y, k) in enumerate(zip(again, got, kinds)):
        assert same(x, y, k, mock.lib), f"output {i}: lifted inputs ({'all' if keys is None else ', '.join(keys)}) changed the result"
    for out in (got, again):     # what the device leaves lazily reduced stays within the header's bound
        for x, k in zip(out, kinds):
            if k == "c":
                assert max(ints(x)) < LAZY_BOUND
    return got


def free_all(d, ptrs):
    for p in ptrs:
        d.free(p)


# ---------------------------------------------------------------- a + c: representation independence on full-field inputs

@pytest.mark.parametrize("n", [64, 1 << 13])
def test_lazy_bind_top(devs, n):
    rng = np.random.default_rng(n)
    inp = {"Z0": mixed(rng, n), "Z1": full_fr(rng, n)}
    r = full_fr(rng, 1)[0]

    def run(d, x):
        ps = [d.upload(x["Z0"]), d.upload(x["Z1"])]
        d.bind_top(ps, n, r)
        out = [d.download(p, (n // 2, 4)) for p in ps]
        free_all(d, ps)
        return out
    check(devs, run, inp, "bb")


@pytest.mark.parametrize("n", [128, 1 << 13])     # n <= 128: latency-shaped kernel
@pytest.mark.parametrize("keys", [None, ("C",)])
def test_lazy_sumcheck_cubic_round(devs, n, keys):
    rng = np.random.default_rng(n + 1)
    inp = {"A0": mixed(rng, n), "A1": full_fr(rng, n), "B0": full_fr(rng, n), "B1": mixed(rng, n), "C": mixed(rng, n)}

    def run(d, x):
        pa = [d.upload(x["A0"]), d.upload(x["A1"])]; pb = [d.upload(x["B0"]), d.upload(x["B1"])]; pc = d.upload(x["C"])
        out = d.sumcheck_cubic_round(pa, pb, pc, n)
        free_all(d, pa + pb + [pc])
        return [out]
    check(devs, run, inp, "b", keys)


@pytest.mark.parametrize("n", [128, 1 << 13])
@pytest.mark.parametrize("keys", [None, ("E",)])
def test_lazy_cubic_eqw_rounds(devs, n, keys):
    """lasso_sumcheck_cubic_eqw_round, _fused and lasso_sumcheck_cubic_eqw2_begin (with and without the bind: its bound arrays are lazily reduced)"""
    rng = np.random.default_rng(n + 2)
    inp = {"A0": mixed(rng, n), "A1": full_fr(rng, n), "B0": full_fr(rng, n), "B1": mixed(rng, n), "E": mixed(rng, n // 2)}
    r = full_fr(rng, 1)[0]

    def run(d, x):
        out = []
        pa = [d.upload(x["A0"]), d.upload(x["A1"])]; pb = [d.upload(x["B0"]), d.upload(x["B1"])]; pe = d.upload(x["E"])
        out.append(d.sumcheck_cubic_eqw_round(pa, pb, pe, n))
        out.append(d.sumcheck_cubic_eqw2(pa, pb, pe, n))
        out.append(d.sumcheck_cubic_eqw2(pa, pb, pe, n, r))
        out.append(np.stack([d.download(p, (n // 2, 4)) for p in pa + pb]))
        free_all(d, pa + pb)
        pa = [d.upload(x["A0"]), d.upload(x["A1"])]; pb = [d.upload(x["B0"]), d.upload(x["B1"])]
        out.append(d.sumcheck_cubic_eqw_round_fused(pa, pb, pe, n, r))
        out.append(np.stack([d.download(p, (n // 2, 4)) for p in pa + pb]))
        free_all(d, pa + pb + [pe])
        return out
    got = check(devs, run, inp, "bbbcbb", keys)
    assert np.array_equal(bigref.cubic_eqw_round([inp["A0"], inp["A1"]], [inp["B0"], inp["B1"]], inp["E"], n), got[0])


@pytest.mark.parametrize("n", [256, 1 << 14])       # the table built in LDS / by the separate eq kernels
def test_lazy_cubic_eqw2_begin_eq(devs, n):
    rng = np.random.default_rng(n + 3)
    ell = (n // 2).bit_length() - 1
    inp = {"A0": mixed(rng, n), "B0": full_fr(rng, n)}
    point = mixed(rng, ell); scale = full_fr(rng, 1)[0]

    def run(d, x):
        pa = [d.upload(x["A0"])]; pb = [d.upload(x["B0"])]; pe = d.alloc(32 * (n // 2))
        out = [d.sumcheck_cubic_eqw2_eq(pa, pb, pe, n, point, scale), d.download(pe, (n // 2, 4))]
        free_all(d, pa + pb + [pe])
        return out
    check(devs, run, inp, "bb")


@pytest.mark.parametrize("n,bind", [(64, False), (1024, False), (2048, True)])    # q = 512 = lasso_sumcheck_tail_capacity(): 2048 binds down to it
@pytest.mark.parametrize("keys", [None, ("E",)])
def test_lazy_cubic_tail(devs, n, bind, keys):
    rng = np.random.default_rng(n + 4 + bind)
    q = n // 4 if bind else n // 2
    turns = (2 * q).bit_length() - 1
    inp = {"A0": mixed(rng, n), "A1": full_fr(rng, n), "B0": full_fr(rng, n), "B1": mixed(rng, n), "E": mixed(rng, q)}
    r0 = full_fr(rng, 1)[0] if bind else None
    chal = full_fr(rng, turns)

    def run(d, x):
        pa = [d.upload(x["A0"]), d.upload(x["A1"])]; pb = [d.upload(x["B0"]), d.upload(x["B1"])]; pe = d.upload(x["E"])
        out = d.sumcheck_cubic_tail(pa, pb, pe, n, r0, chal)
        free_all(d, pa + pb + [pe])
        return out
    check(devs, run, inp, "b" * (turns + 1), keys)


@pytest.mark.parametrize("n", [64, 1024])
def test_lazy_cubic_tail_begin_eq(devs, n):
    rng = np.random.default_rng(n + 5)
    q = n // 2; ell = q.bit_length() - 1
    turns = (2 * q).bit_length() - 1
    inp = {"A0": mixed(rng, n), "B0": full_fr(rng, n)}
    point = mixed(rng, ell); scale = full_fr(rng, 1)[0]; chal = full_fr(rng, turns)

    def run(d, x):
        pa = [d.upload(x["A0"])]; pb = [d.upload(x["B0"])]
        out = d.sumcheck_cubic_tail_eq(pa, pb, n, point, scale, chal)
        free_all(d, pa + pb)
        return out
    check(devs, run, inp, "b" * (turns + 1))


@pytest.mark.parametrize("n", [64, 1 << 14])
@pytest.mark.parametrize("keys", [None, ("E",)])
def test_lazy_linear_eqw_rounds(devs, n, keys):
    """lasso_sumcheck_linear_eqw_round, _fused, _fused_from"""
    rng = np.random.default_rng(n + 6)
    inp = {"P0": mixed(rng, n), "P1": full_fr(rng, n), "E": mixed(rng, n // 2)}
    r = full_fr(rng, 1)[0]

    def run(d, x):
        pp = [d.upload(x["P0"]), d.upload(x["P1"])]; pe = d.upload(x["E"])
        out = [d.sumcheck_linear_eqw_round(pp, pe, n)]
        pd = [d.alloc(32 * (n // 2)) for _ in pp]
        out.append(d.sumcheck_linear_eqw_round_fused_from(pp, pd, pe, n, r))
        out.append(np.stack([d.download(p, (n // 2, 4)) for p in pd]))
        out.append(d.sumcheck_linear_eqw_round_fused(pp, pe, n, r))
        out.append(np.stack([d.download(p, (n // 2, 4)) for p in pp]))
        free_all(d, pp + pd + [pe])
        return out
    check(devs, run, inp, "bbcbc", keys)


@pytest.mark.parametrize("n,bind", [(64, False), (2048, True)])
@pytest.mark.parametrize("keys", [None, ("E",)])
def test_lazy_linear_tail(devs, n, bind, keys):
    rng = np.random.default_rng(n + 7)
    q = n // 4 if bind else n // 2
    turns = (2 * q).bit_length() - 1
    inp = {"P0": mixed(rng, n), "P1": full_fr(rng, n), "E": mixed(rng, q)}
    r0 = full_fr(rng, 1)[0] if bind else None
    chal = full_fr(rng, turns)

    def run(d, x):
        pp = [d.upload(x["P0"]), d.upload(x["P1"])]; pe = d.upload(x["E"])
        out = d.sumcheck_linear_tail(pp, pe, n, r0, chal)
        free_all(d, pp + [pe])
        return out
    check(devs, run, inp, "b" * (turns + 1), keys)


@pytest.mark.parametrize("kind,c,log_m,log_r", [("and", 2, 4, 0), ("lt", 2, 4, 0), ("range", 3, 8, 40), ("spark", 3, 4, 0)])
@pytest.mark.parametrize("n", [2, 1 << 11])
@pytest.mark.parametrize("keys", [None, ("eq",)])
def test_lazy_combine_round_and_claim(devs, kind, c, log_m, log_r, n, keys):
    rng = np.random.default_rng(n + c)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, log_r)
    alpha = 2 * c if kind == "lt" else c
    degree = c + 1 if kind in ("lt", "spark") else 2
    inp = {f"P{i}": mixed(rng, n) if i % 2 == 0 else full_fr(rng, n) for i in range(alpha)}
    inp["eq"] = mixed(rng, n)

    def run(d, x):
        pp = [d.upload(x[f"P{i}"]) for i in range(alpha)]; pe = d.upload(x["eq"])
        out = [d.sumcheck_combine_round(S, pp, pe, n, degree), d.combine_claim(S, pp, pe, n)]
        if kind == "lt":
            qq = [d.alloc(32 * n) for _ in pp]
            d.lt_prescale(S, qq, n, src=pp)
            out.append(d.sumcheck_combine_round_lt_scaled(S, qq, pe, n, degree))
            out.append(np.stack([d.download(p, (n, 4)) for p in qq]))
            free_all(d, qq)
        free_all(d, pp + [pe])
        return out
    check(devs, run, inp, "bbbc" if kind == "lt" else "bb", keys)


@pytest.mark.parametrize("n", [7, 1 << 12])
def test_lazy_multi_dot_and_heads(devs, n):
    rng = np.random.default_rng(n + 8)
    inp = {"P0": mixed(rng, n), "P1": full_fr(rng, n), "W": mixed(rng, n)[::-1].copy()}

    def run(d, x):
        pp = [d.upload(x["P0"]), d.upload(x["P1"])]; pw = d.upload(x["W"])
        out = [d.multi_dot(pp, pw, n), d.read_heads(pp + [pw])]
        free_all(d, pp + [pw])
        return out
    got = check(devs, run, inp, "bc")
    assert np.array_equal(got[0], bigref.multi_dot([inp["P0"], inp["P1"]], inp["W"]))


@pytest.mark.parametrize("n", [8, 1 << 13])
def test_lazy_gp_build(devs, n):
    rng = np.random.default_rng(n + 9)
    inp = {"L": mixed(rng, n)}

    def run(d, x):
        tree = np.zeros((2 * n, 4), dtype=np.uint64); tree[:n] = x["L"]
        p = d.upload(tree)
        d.gp_build(p, n)
        out = [d.download(p, (2 * n - 2, 4))[n:]]
        d.free(p)
        return out
    check(devs, run, inp, "b")


@pytest.mark.parametrize("s,log_m", [(64, 4), (1 << 13, 8)])
def test_lazy_fingerprints(devs, s, log_m):
    """lasso_fingerprint_ops / _gp / _gp_upper / _strips and lasso_fingerprint_mem, table, read, final and lookup arrays lifted; plus lasso_gather"""
    rng = np.random.default_rng(s + log_m)
    m = 1 << log_m
    dim = rng.integers(0, m, size=s, dtype=np.uint32); dim[0] = m - 1; dim[1] = 0
    inp = {"T": mixed(rng, m), "R": mixed(rng, s), "F": full_fr(rng, m)}
    gamma, tau = full_fr(rng, 2)
    cs = s // 8

    def run(d, x):
        pt = d.upload(x["T"]); pd = d.upload(dim); pr = d.upload(x["R"]); pf = d.upload(x["F"])
        ro = d.alloc(32 * s); wo = d.alloc(32 * s); io = d.alloc(32 * m); fo = d.alloc(32 * m)
        tr = d.alloc(64 * s); tw = d.alloc(64 * s); ur = d.alloc(32 * s); uw = d.alloc(32 * s); sr = d.alloc(32 * 4 * cs); sw = d.alloc(32 * 4 * cs)
        ge = d.alloc(32 * s)
        d.fingerprint_ops(pt, pd, pr, s, gamma, tau, ro, wo)
        d.fingerprint_mem(pt, pf, m, gamma, tau, io, fo)
        d.fingerprint_ops_gp(pt, pd, pr, s, gamma, tau, tr, tw)
        d.fingerprint_ops_gp_upper(pt, pd, pr, s, gamma, tau, ur, uw)
        d.fingerprint_ops_strips(pt, pd, pr, s, gamma, tau, 2, 0, cs, sr, sw)
        d.gather(pt, pd, s, ge)
        out = [d.download(ro, (s, 4)), d.download(wo, (s, 4)), d.download(io, (m, 4)), d.download(fo, (m, 4)),
               d.download(tr, (2 * s - 2, 4)), d.download(tw, (2 * s - 2, 4)), d.download(ur, (s - 2, 4)), d.download(uw, (s - 2, 4)),
               d.download(sr, (4 * cs, 4)), d.download(sw, (4 * cs, 4)), d.download(ge, (s, 4))]
        free_all(d, (pt, pd, pr, pf, ro, wo, io, fo, tr, tw, ur, uw, sr, sw, ge))
        return out
    got = check(devs, run, inp, "bbbbbbbbbbc")
    g, t = gamma.reshape(1, 4), tau.reshape(1, 4)
    want = bigref.fingerprint_ops(inp["T"], dim, inp["R"], g, t) + bigref.fingerprint_mem(inp["T"], inp["F"], g, t)
    for x, y in zip(got[:4], want):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("ls,rs", [(2, 4), (64, 300)])
def test_lazy_matvec_left(devs, ls, rs):
    rng = np.random.default_rng(ls + rs)
    inp = {"Z": mixed(rng, ls * rs), "L": mixed(rng, ls)}

    def run(d, x):
        pz = d.upload(x["Z"]); pl = d.upload(x["L"]); po = d.alloc(32 * rs)
        d.matvec_left_dev(pz, pl, ls, rs, po)
        out = [d.matvec_left(pz, canon(x["L"]), ls, rs), d.download(po, (rs, 4)), d.fr_to_bytes(po, rs), d.fr_to_bytes(pz, ls * rs)]
        free_all(d, (pz, pl, po))
        return out
    got = check(devs, run, inp, "bbbb")
    assert np.array_equal(got[0], bigref.matvec_left(inp["Z"], inp["L"], ls, rs))


@pytest.mark.parametrize("n", [1 << 12, 1 << 17])    # fr_to_bytes: through the mapped buffer / through scratch
def test_lazy_fr_to_u32_and_bytes(devs, n):
    rng = np.random.default_rng(n + 10)
    vals = rng.integers(0, 2**32, size=n, dtype=np.uint64); vals[:4] = [0, 1, 2**32 - 1, 2**31]
    inp = {"X": small_fr(vals)}

    def run(d, x):
        p = d.upload(x["X"]); p32 = d.alloc(4 * n)
        mx = d.fr_to_u32(p, n, p32)
        out = [np.array([mx], dtype=np.uint32), d.download(p32, (n,), dtype=np.uint32), d.fr_to_bytes(p, n)]
        free_all(d, (p, p32))
        return out
    check(devs, run, inp, "bbb")


@pytest.mark.parametrize("ls,rs,maxv", [(4, 8, 256), (64, 256, 1 << 16), (3, 100, 1 << 32), (8, 64, None)])
def test_lazy_hyrax_commit(devs, gens_300, ls, rs, maxv):
    """a lifted small-integer Z still commits to the same bytes (the small-scalar kernels are chosen from the canonical values)"""
    rng = np.random.default_rng(ls * rs)
    if maxv is None:
        Z = mixed(rng, ls * rs)
    else:
        v = rng.integers(0, maxv, size=ls * rs, dtype=np.uint64); v[0] = 0; v[-1] = maxv - 1
        Z = small_fr(v)

    def run(d, x):
        b = d.bases_create(gens_300); p = d.upload(x["Z"])
        out = [d.hyrax_commit(p, ls, rs, b), d.hyrax_commit_compressed(p, ls, rs, b)]
        free_all(d, [p]); d.bases_destroy(b)
        return out
    check(devs, run, {"Z": Z}, "pb")


@pytest.mark.parametrize("n", [2, 64, 298])
def test_lazy_msm(devs, gens_300, n):
    """lasso_msm (host scalars), lasso_msm_dev, lasso_msm_dev_scaled"""
    rng = np.random.default_rng(n + 11)
    inp = {"S": mixed(rng, n)}
    scale = full_fr(rng, 1)[0]; tail = mixed(rng, 2)

    def run(d, x):
        b = d.bases_create(gens_300[: n + 2]); p = d.upload(x["S"])
        out = [d.msm(b, canon(x["S"])), d.msm_dev(b, p, n), d.msm_dev_scaled(b, p, n, scale, tail)]
        free_all(d, [p]); d.bases_destroy(b)
        return out
    check(devs, run, inp, "ppp")


@pytest.mark.parametrize("n,nk", [(8, 8), (256, 4), (1 << 12, 1 << 11)])
def test_lazy_bullet(devs, n, nk):
    """lasso_inner_products_lr, lasso_bullet_lr, lasso_bullet_fold, lasso_bullet_round (with and without the fold)"""
    rng = np.random.default_rng(n * 3 + nk)
    mock_lib = devs[1].lib
    g = gens(mock_lib, b"gens_sparse_poly", n + 1)
    nw = n // nk
    inp = {"a": mixed(rng, nk), "b": full_fr(rng, nk), "w": mixed(rng, nw)}
    tail = mixed(rng, 4); blinds = full_fr(rng, 2)
    u, ui = words([mont(3)]), words([mont(pow(3, -1, FR_P))])
    half, nw2 = nk // 2, 2 * nw

    def run(d, x):
        bases = d.bases_create(g)
        pa = d.upload(x["a"]); pb = d.upload(x["b"]); pw = d.upload(x["w"]); pw2 = d.alloc(32 * nw2)
        out = [d.inner_products_lr(pa, pb, nk), d.bullet_lr(bases, n, pa, nk, pw, tail)]
        out.append(d.bullet_round(bases, n, pa, pb, pw, 0, 0, 0, nk, None, None, blinds))
        if nk >= 4:
            a2 = d.alloc(32 * half); b2 = d.alloc(32 * half); w3 = d.alloc(32 * nw2)
            out.append(d.bullet_round(bases, n, pa, pb, pw, a2, b2, w3, half, u[0], ui[0], blinds))
            out += [d.download(a2, (half, 4)), d.download(b2, (half, 4)), d.download(w3, (nw2, 4))]
            free_all(d, (a2, b2, w3))
        d.bullet_fold(pa, pb, nk, pw, nw, pw2, u[0], ui[0])
        out += [d.download(pa, (half, 4)), d.download(pb, (half, 4)), d.download(pw2, (nw2, 4))]
        free_all(d, (pa, pb, pw, pw2)); d.bases_destroy(bases)
        return out
    got = check(devs, run, inp, "bppp" + "bbb" + "bbb" if nk >= 4 else "bpp" + "bbb")
    assert np.array_equal(got[0], bigref.inner_products_lr(inp["a"], inp["b"]))
    for x, y in zip(got[-3:], bigref.bullet_fold(inp["a"], inp["b"], inp["w"], u, ui)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("n", [8, 256])
def test_lazy_bullet_tail_ahead(devs, n):
    """lasso_bullet_tail_ahead + lasso_bullet_post: the last fold, the heads and the delta MSM in one chain"""
    import ctypes as C
    import time
    rng = np.random.default_rng(n + 12)
    mock_lib = devs[1].lib
    g = gens(mock_lib, b"gens_sparse_poly", n + 1)
    nw = n // 2
    inp = {"a": mixed(rng, 2), "b": full_fr(rng, 2), "w": mixed(rng, nw)}
    scale = full_fr(rng, 1); tail = mixed(rng, 2)
    u, ui = edge_fr([I_TWO]), edge_fr([I_HALF_UP])
    vp = lambda x: np.ascontiguousarray(x, dtype=np.uint64).ctypes.data_as(C.c_void_p)

    def run(d, x):
        bases = d.bases_create(g)
        if d.lib.lasso_bullet_tail_ahead_ok(d.ctx, bases) != 1:
            d.bases_destroy(bases)
            pytest.skip("lasso_bullet_tail_ahead not available in this configuration")
        pa = d.upload(x["a"]); pb = d.upload(x["b"]); pw = d.upload(x["w"]); pw2 = d.alloc(32 * n)
        d._chk(d.lib.lasso_bullet_tail_ahead(d.ctx, bases, n, C.c_void_p(pa), C.c_void_p(pb), C.c_void_p(pw), nw, C.c_void_p(pw2), vp(scale), vp(tail)))
        time.sleep(0.002)
        d._chk(d.lib.lasso_bullet_post(d.ctx, vp(u), vp(ui)))
        res = np.empty((6, 4), dtype=np.uint64)
        d._chk(d.lib.lasso_result_wait(d.ctx, res.ctypes.data_as(C.c_void_p), 6))
        out = [res[:4].reshape(1, 16), res[4:6], d.download(pw2, (n, 4))]
        free_all(d, (pa, pb, pw, pw2)); d.bases_destroy(bases)
        return out
    check(devs, run, inp, "pbb")


# ---------------------------------------------------------------- b: edge scalars against the mock and the big-integer reference

CHALLENGES = {"all_m1": [I_M1], "zero_one_m1": [I_ZERO, I_ONE, I_M1], "all_zero": [I_ZERO], "all_one": [I_ONE], "edges": list(range(NE))}


@pytest.mark.parametrize("pattern", list(CHALLENGES))
@pytest.mark.parametrize("n", [64, 1 << 13])
def test_edge_bind_chain_to_scalar(devs, pattern, n):
    """lasso_bind_top bound down to one element with challenges from EDGE (every r = p - 1, 0 / 1 / p - 1 alternating, ...) == mock == big integers"""
    rng = np.random.default_rng(n)
    z = mixed(rng, n)
    seq = CHALLENGES[pattern]
    rs = edge_fr([seq[i % len(seq)] for i in range(n.bit_length() - 1)])

    def run(d):
        p = d.upload(z); m = n; steps = []
        for r in rs:
            d.bind_top([p], m, r); m //= 2
            steps.append(d.download(p, (m, 4)))
        d.free(p)
        return steps
    a, b = run(devs[0]), run(devs[1])
    want = z
    for x, y, r in zip(a, b, rs):
        want = bigref.bind(want, r.reshape(1, 4))
        assert np.array_equal(x, y) and np.array_equal(x, want)


@pytest.mark.parametrize("pattern", ["all_zero", "all_one", "all_m1", "zero_one_m1", "edges"])
@pytest.mark.parametrize("ell", [7, 13])     # lasso_sumcheck_cubic_eqw2_begin_eq takes tables of 2^7 entries and more
@pytest.mark.parametrize("si", [None, I_ZERO, I_M1, NE - 1])
def test_edge_eq_points(devs, pattern, ell, si):
    """eq tables over points of 0, 1, p - 1 (most of the table zero) and scales from EDGE: lasso_eq_evals(_scaled) and the round that builds the table inline"""
    seq = CHALLENGES[pattern]
    point = edge_fr([seq[i % len(seq)] for i in range(ell)])
    scale = None if si is None else edge_fr([si])[0]
    rng = np.random.default_rng(ell)
    n = 2 << ell
    A = [mixed(rng, n)]; B = [full_fr(rng, n)]

    def run(d):
        p = d.alloc(32 << ell); e1 = d.alloc(32 << ell)
        d.eq_evals_scaled(point, scale, p)
        pa = [d.upload(A[0])]; pb = [d.upload(B[0])]
        inline = d.sumcheck_cubic_eqw2_eq(pa, pb, e1, n, point, scale)
        out = [d.download(p, (1 << ell, 4)), inline, d.download(e1, (1 << ell, 4))]
        free_all(d, [p, e1] + pa + pb)
        return out
    a, b = run(devs[0]), run(devs[1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[0], bigref.eq_evals(point, None if scale is None else scale.reshape(1, 4)))
    assert np.array_equal(a[2], a[0])


@pytest.mark.parametrize("pattern", ["all_m1", "zero_one_m1", "edges"])
@pytest.mark.parametrize("n,bind", [(64, False), (2048, True)])
def test_edge_tail_challenges(devs, pattern, n, bind):
    """the resident cubic and linear tails (and the inline-eq tail) with challenge sequences from EDGE"""
    rng = np.random.default_rng(n)
    q = n // 4 if bind else n // 2
    turns = (2 * q).bit_length() - 1
    seq = CHALLENGES[pattern]
    chal = edge_fr([seq[i % len(seq)] for i in range(turns)])
    r0 = edge_fr([I_M1])[0] if bind else None
    A = [mixed(rng, n), full_fr(rng, n)]; B = [full_fr(rng, n), mixed(rng, n)]; E = mixed(rng, q)
    ell = q.bit_length() - 1
    point = edge_fr([seq[i % len(seq)] for i in range(ell)])

    def run(d):
        pa = [d.upload(x) for x in A]; pb = [d.upload(x) for x in B]; pe = d.upload(E)
        out = d.sumcheck_cubic_tail(pa, pb, pe, n, r0, chal)
        free_all(d, pa + pb)
        pa = [d.upload(x) for x in A]
        out += d.sumcheck_linear_tail(pa, pe, n, r0, chal)
        free_all(d, pa)
        if not bind:
            pa = [d.upload(x) for x in A]; pb = [d.upload(x) for x in B]
            out += d.sumcheck_cubic_tail_eq(pa, pb, n, point, edge_fr([I_M1])[0], chal)
            free_all(d, pa + pb)
        d.free(pe)
        return out
    a, b = run(devs[0]), run(devs[1])
    assert len(a) == len(b)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("ei", [I_ZERO, I_ONE, I_M1, NE - 1])
@pytest.mark.parametrize("n", [128, 1 << 13])
def test_edge_eq_tables_in_rounds(devs, ei, n):
    """constant eq tables and challenges of 0 / 1 / p - 1 through the eq-weighted cubic rounds: mock and big integers"""
    rng = np.random.default_rng(n + ei)
    A = [mixed(rng, n)]; B = [full_fr(rng, n)]; E = edge_fr([ei] * (n // 2))

    def run(d):
        pa = [d.upload(A[0])]; pb = [d.upload(B[0])]; pe = d.upload(E)
        out = [d.sumcheck_cubic_eqw_round(pa, pb, pe, n)]
        m = n
        for r in edge_fr([I_M1, I_ZERO, I_ONE]):
            out.append(d.sumcheck_cubic_eqw2(pa, pb, pe, m, r)); m //= 2
            out.append(canon(np.stack([d.download(p, (m, 4)) for p in pa + pb])))
        free_all(d, pa + pb + [pe])
        return out
    a, b = run(devs[0]), run(devs[1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert np.array_equal(a[0], bigref.cubic_eqw_round(A, B, E, n))


@pytest.mark.parametrize("gi,ti", [(I_ZERO, I_ZERO), (I_ONE, I_M1), (I_M1, I_ONE), (NE - 1, I_TWO), (I_M1, "collide")])
def test_edge_gamma_tau(devs, gi, ti):
    """fingerprints with gamma / tau from EDGE, including tau = the fingerprint of an entry (that fingerprint is 0, and every tree product above it)"""
    rng = np.random.default_rng(7)
    m, s = 16, 64
    table = mixed(rng, m); final = full_fr(rng, m); read = mixed(rng, s)
    dim = rng.integers(0, m, size=s, dtype=np.uint32); dim[0] = 3
    gamma = edge_fr([gi])
    if ti == "collide":      # a + v gamma + t gamma^2 == tau for read entry 0
        g = bigref.val(gamma)[0]
        t = (bigref.val(read[:1])[0] * g * g + bigref.val(table[3:4])[0] * g + 3) % FR_P
        tau = words([mont(t)])
    else:
        tau = edge_fr([ti])

    def run(d):
        pt = d.upload(table); pd = d.upload(dim); pr = d.upload(read); pf = d.upload(final)
        ro = d.alloc(32 * s); wo = d.alloc(32 * s); io = d.alloc(32 * m); fo = d.alloc(32 * m); tr = d.alloc(64 * s); tw = d.alloc(64 * s)
        d.fingerprint_ops(pt, pd, pr, s, gamma[0], tau[0], ro, wo)
        d.fingerprint_mem(pt, pf, m, gamma[0], tau[0], io, fo)
        d.fingerprint_ops_gp(pt, pd, pr, s, gamma[0], tau[0], tr, tw)
        out = [d.download(ro, (s, 4)), d.download(wo, (s, 4)), d.download(io, (m, 4)), d.download(fo, (m, 4)), d.download(tr, (2 * s - 2, 4)), d.download(tw, (2 * s - 2, 4))]
        free_all(d, (pt, pd, pr, pf, ro, wo, io, fo, tr, tw))
        return out
    a, b = run(devs[0]), run(devs[1])
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    want = bigref.fingerprint_ops(table, dim, read, gamma, tau) + bigref.fingerprint_mem(table, final, gamma, tau)
    for x, y in zip(a[:4], want):
        assert np.array_equal(x, y)
    if ti == "collide":
        assert not a[0][0].any() and not a[4][-2].any()        # the zero leaf propagates up to the last layer


@pytest.mark.parametrize("u_i,ui_i", [(I_ONE, I_ONE), (I_M1, I_M1), (I_TWO, I_HALF_UP), (I_HALF_UP, I_TWO)])
@pytest.mark.parametrize("n,nk", [(8, 8), (1 << 12, 1 << 11)])
def test_edge_bullet_scalars(devs, gens_300, u_i, ui_i, n, nk):
    """u / u^-1 pairs u in {1, p - 1, 2, (p + 1) / 2}, blinds, scale and tails from EDGE: fold, round, MSMs"""
    rng = np.random.default_rng(n + u_i)
    mock_lib = devs[1].lib
    g = gens(mock_lib, b"gens_sparse_poly", n + 1)
    nw = n // nk
    a = mixed(rng, nk); b = full_fr(rng, nk); w = mixed(rng, nw)
    u, ui = edge_fr([u_i]), edge_fr([ui_i])
    blinds = edge_fr([I_M1, NE - 1]); tail = edge_fr([I_ZERO, I_M1, I_ONE, NE - 1]); scale = edge_fr([I_M1])[0]
    half = nk // 2

    def run(d):
        bases = d.bases_create(g)
        pa = d.upload(a); pb = d.upload(b); pw = d.upload(w)
        a2 = d.alloc(32 * half); b2 = d.alloc(32 * half); w2 = d.alloc(32 * 2 * nw)
        out = [d.bullet_round(bases, n, pa, pb, pw, a2, b2, w2, half, u[0], ui[0], blinds),
               d.download(a2, (half, 4)), d.download(b2, (half, 4)), d.download(w2, (2 * nw, 4)),
               d.bullet_lr(bases, n, pa, nk, pw, tail)]
        d.bullet_fold(pa, pb, nk, pw, nw, w2, u[0], ui[0])
        out += [d.download(pa, (half, 4)), d.download(pb, (half, 4)), d.download(w2, (2 * nw, 4))]
        b300 = d.bases_create(gens_300)
        out.append(d.msm_dev_scaled(b300, w2, min(2 * nw, 298), scale, tail[:2]))
        d.bases_destroy(b300)
        free_all(d, (pa, pb, pw, a2, b2, w2)); d.bases_destroy(bases)
        return out
    x, y = run(devs[0]), run(devs[1])
    for i, (p, q) in enumerate(zip(x, y)):
        assert same(p, q, "p" if i in (0, 4, 8) else "b", mock_lib)
    for p, q in zip(x[5:8], bigref.bullet_fold(a, b, w, u, ui)):
        assert np.array_equal(p, q)


# ---------------------------------------------------------------- BN254

def test_gpu_bn254_field_edges():
    """this module again on the BN254 build, in a child process (tests/fieldref.py reads LASSO_TEST_CURVE at import)"""
    from fieldref import CURVE
    if CURVE == "bn254":
        return
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LASSO_TEST_CURVE="bn254")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "gpu", "-x", "-q", "-p", "no:cacheprovider",
                          "-k", "not test_gpu_bn254_field_edges"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout
