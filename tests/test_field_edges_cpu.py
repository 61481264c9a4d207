"""The big-integer statements of tests/bigref.py against the oracle's mock of the same C ABI, on the inputs the GPU edge tests use (tests/gpuutil.py EDGE /
full_fr): the expected values of tests/test_gpu_field_edges.py section d are checked here without a GPU, for both curves (BN254 in a child process)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import bigref
from fieldref import L as FR_P
from gpuutil import EDGE, edge_fr, full_fr, load_mock, mont, words

NE = len(EDGE)
SCALARS = [0, 1, 3, 5, 6, NE - 1]        # EDGE rows: Montgomery 0, 1, p - 1, (p - 1) / 2, (p + 1) / 2, the top limb-space word


@pytest.fixture(scope="module")
def mock():
    from lasso_amd import Device
    d = Device(0, lib=load_mock())
    yield d
    d.close()


def mixed(rng, n):
    """full-field rows with every EDGE word in front"""
    x = full_fr(rng, n)
    k = min(n, NE)
    x[:k] = edge_fr(range(k))
    return x


def test_edge_words_cover_both_spaces():
    p = FR_P
    assert EDGE[:7] == [mont(v) for v in (0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2)]
    assert all(2**(29 * k) - 1 in EDGE and 2**(29 * k) in EDGE for k in range(1, 9))
    assert p - 1 in EDGE and 1 in EDGE
    top = EDGE[-1]
    assert top < p and top + 2**232 >= p and top % 2**232 == 2**232 - 1


@pytest.mark.parametrize("si", SCALARS)
@pytest.mark.parametrize("n", [2, 64])
def test_bind_matches_mock(mock, si, n):
    rng = np.random.default_rng(n + si)
    z = mixed(rng, n); r = edge_fr([si])
    p = mock.upload(z)
    mock.bind_top([p], n, r[0])
    got = mock.download(p, (n // 2, 4)); mock.free(p)
    assert np.array_equal(got, bigref.bind(z, r))


def test_bind_chain_all_minus_one_matches_mock(mock):
    rng = np.random.default_rng(3)
    n = 64
    z = mixed(rng, n); r = words([mont(FR_P - 1)])
    p = mock.upload(z); want = z
    m = n
    while m > 1:
        mock.bind_top([p], m, r[0]); want = bigref.bind(want, r); m //= 2
    got = mock.download(p, (1, 4)); mock.free(p)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("pattern", ["zeros", "ones", "minus_one", "alternating", "mixed"])
@pytest.mark.parametrize("scaled", [False, True])
def test_eq_evals_match_mock(mock, pattern, scaled):
    rng = np.random.default_rng(len(pattern))
    ell = 6
    r = {"zeros": edge_fr([0] * ell), "ones": edge_fr([1] * ell), "minus_one": edge_fr([3] * ell),
         "alternating": edge_fr([0, 1, 3, 0, 1, 3]), "mixed": mixed(rng, ell)}[pattern]
    scale = edge_fr([3])[0] if scaled else None
    p = mock.alloc(32 << ell)
    mock.eq_evals_scaled(r, scale, p)
    got = mock.download(p, (1 << ell, 4)); mock.free(p)
    assert np.array_equal(got, bigref.eq_evals(r, None if scale is None else scale.reshape(1, 4)))


def test_multi_dot_and_matvec_match_mock(mock):
    rng = np.random.default_rng(11)
    n = 64
    polys = [mixed(rng, n) for _ in range(3)]; w = mixed(rng, n)[::-1].copy()
    pp = [mock.upload(x) for x in polys]; pw = mock.upload(w)
    assert np.array_equal(mock.multi_dot(pp, pw, n), bigref.multi_dot(polys, w))
    ls, rs = 8, 8
    lv = edge_fr(range(ls))
    assert np.array_equal(mock.matvec_left(pp[0], lv, ls, rs), bigref.matvec_left(polys[0], lv, ls, rs))
    for p in pp + [pw]:
        mock.free(p)


def test_inner_products_and_fold_match_mock(mock):
    rng = np.random.default_rng(12)
    nk, nw = 32, 4
    a = mixed(rng, nk); b = mixed(rng, nk)[::-1].copy(); w = edge_fr([3, 0, 1, NE - 1])
    pa = mock.upload(a); pb = mock.upload(b)
    assert np.array_equal(mock.inner_products_lr(pa, pb, nk), bigref.inner_products_lr(a, b))
    for ui_, i_ in ((1, 1), (3, 3), (2, 6)):     # u = 1, p - 1 (self-inverse) and 2 with u^-1 = (p + 1) / 2
        u, ui = edge_fr([ui_]), edge_fr([i_])
        qa = mock.upload(a); qb = mock.upload(b); pw = mock.upload(w); pw2 = mock.alloc(32 * 2 * nw)
        mock.bullet_fold(qa, qb, nk, pw, nw, pw2, u[0], ui[0])
        fa, fb, fw = bigref.bullet_fold(a, b, w, u, ui)
        assert np.array_equal(mock.download(qa, (nk // 2, 4)), fa) and np.array_equal(mock.download(qb, (nk // 2, 4)), fb)
        assert np.array_equal(mock.download(pw2, (2 * nw, 4)), fw)
        for p in (qa, qb, pw, pw2):
            mock.free(p)
    mock.free(pa); mock.free(pb)


@pytest.mark.parametrize("gi,ti", [(0, 0), (1, 3), (3, 1), (5, NE - 1), (NE - 1, 2)])
def test_fingerprints_match_mock(mock, gi, ti):
    rng = np.random.default_rng(gi * 31 + ti)
    m, s = 32, 64
    table = mixed(rng, m); final = mixed(rng, m)[::-1].copy(); read = mixed(rng, s)
    dim = rng.integers(0, m, size=s, dtype=np.uint32); dim[0] = m - 1; dim[1] = 0
    gamma, tau = edge_fr([gi]), edge_fr([ti])
    pt = mock.upload(table); pd = mock.upload(dim); pr = mock.upload(read); pf = mock.upload(final)
    outs = [mock.alloc(32 * s), mock.alloc(32 * s), mock.alloc(32 * m), mock.alloc(32 * m)]
    mock.fingerprint_ops(pt, pd, pr, s, gamma[0], tau[0], outs[0], outs[1])
    mock.fingerprint_mem(pt, pf, m, gamma[0], tau[0], outs[2], outs[3])
    got = [mock.download(outs[0], (s, 4)), mock.download(outs[1], (s, 4)), mock.download(outs[2], (m, 4)), mock.download(outs[3], (m, 4))]
    want = list(bigref.fingerprint_ops(table, dim, read, gamma, tau)) + list(bigref.fingerprint_mem(table, final, gamma, tau))
    for x, y in zip(got, want):
        assert np.array_equal(x, y)
    for p in [pt, pd, pr, pf] + outs:
        mock.free(p)


@pytest.mark.parametrize("ei", [None, 0, 1, 3])
def test_cubic_eqw_sums_match_mock(mock, ei):
    rng = np.random.default_rng(7 if ei is None else ei)
    n, nc = 64, 2
    A = [mixed(rng, n) for _ in range(nc)]; B = [mixed(rng, n)[::-1].copy() for _ in range(nc)]
    E = mixed(rng, n // 2) if ei is None else edge_fr([ei] * (n // 2))
    pa = [mock.upload(x) for x in A]; pb = [mock.upload(x) for x in B]; pe = mock.upload(E)
    got = mock.sumcheck_cubic_eqw_round(pa, pb, pe, n)
    for p in pa + pb + [pe]:
        mock.free(p)
    assert np.array_equal(got, bigref.cubic_eqw_round(A, B, E, n))


def test_bn254_references_match_bn254_mock():
    """this module again over BN254 (fieldref reads the curve at import: a child process)"""
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, LASSO_TEST_CURVE="bn254")
    res = subprocess.run([sys.executable, "-m", "pytest", os.path.abspath(__file__), "-m", "not gpu", "-x", "-q", "-p", "no:cacheprovider",
                          "-k", "not test_bn254_references_match_bn254_mock"], cwd=root, env=env, capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-3000:] + res.stderr[-2000:]
    assert " passed" in res.stdout and "failed" not in res.stdout
