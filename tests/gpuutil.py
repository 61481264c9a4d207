"""Helpers shared by the GPU parity tests: the real device library next to the oracle's mock of the same C ABI."""
import ctypes
import os
import subprocess

import numpy as np

from fieldref import CURVE, L as FR_P, limbs, to_mont

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def load_mock():
    from lasso_amd import _abi
    name = "libmock_hip_bn254.so" if CURVE == "bn254" else "libmock_hip.so"
    so = os.path.join(ROOT, "oracle", name)
    srcs = [os.path.join(ROOT, "oracle", f) for f in ("mock_hip.cpp", "lasso_oracle.hpp", "ff.hpp", "ed25519.hpp", "bn254.hpp", "hashes.hpp")] + [os.path.join(ROOT, "include", "lasso_hip.h"), os.path.join(ROOT, "lasso_amd", "csrc", "device_switches.cuh")]
    if not os.path.exists(so) or any(os.path.getmtime(s) > os.path.getmtime(so) for s in srcs):
        subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), name])
    lib = ctypes.CDLL(so)
    _abi.declare(lib)
    lib.mock_point_compress.argtypes = [ctypes.c_void_p, ctypes.c_void_p]
    lib.mock_point_on_curve.argtypes = [ctypes.c_void_p]
    lib.mock_point_on_curve.restype = ctypes.c_int
    lib.mock_gens.argtypes = [ctypes.c_char_p, ctypes.c_size_t, ctypes.c_void_p]
    return lib


def rand_fr(rng, n, edge=True):
    """(n,4) uint64 Montgomery-form field elements (any value < p is a valid Montgomery representation)."""
    a = rng.integers(0, 2**64, size=(n, 4), dtype=np.uint64)
    a[:, 3] &= np.uint64(2**60 - 1)   # < 2^252 < p
    if edge and n >= 8:
        a[0] = 0
        a[1] = limbs(FR_P - 1)
        a[2] = limbs(1)
        a[3] = limbs(FR_P - 2)
        a[4] = [2**64 - 1, 2**64 - 1, 2**64 - 1, 2**60 - 1]
    return a


def small_fr(vals):
    """small non-negative ints -> (n,4) Montgomery limbs via Python big ints"""
    return np.array([limbs(to_mont(int(v), FR_P)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def compress_points(mock, pts):
    """(k,16) uint64 projective points -> list of 32-byte compressed encodings (via the oracle); also checks curve membership."""
    out = []
    buf = (ctypes.c_uint8 * 32)()
    for i in range(pts.shape[0]):
        p = np.ascontiguousarray(pts[i])
        assert mock.mock_point_on_curve(p.ctypes.data_as(ctypes.c_void_p)) == 1, "point not on curve / T inconsistent"
        mock.mock_point_compress(p.ctypes.data_as(ctypes.c_void_p), buf)
        out.append(bytes(buf))
    return out


def gens(mock, label, n):
    out = np.empty((n + 1, 8), dtype=np.uint64)
    mock.mock_gens(label, n, out.ctypes.data_as(ctypes.c_void_p))
    return out


# ---- inputs at the edges of the field and of its memory form (tests/test_gpu_field_edges.py, tests/test_field_edges_cpu.py)

# include/lasso_hip.h: lazily reduced arrays hold representatives below this bound, and every entry point accepts them
LAZY_BOUND = 2**254 + 2**130


def words(vals):
    """Python ints (each < 2^256) -> (n,4) uint64 memory words, no conversion"""
    return np.array([limbs(int(v)) for v in vals], dtype=np.uint64).reshape(-1, 4)


def ints(rows):
    """(..., 4) uint64 memory words -> flat list of Python ints"""
    flat = np.asarray(rows, dtype=np.uint64).reshape(-1, 4)
    return [int(r[0]) | int(r[1]) << 64 | int(r[2]) << 128 | int(r[3]) << 192 for r in flat]


def full_fr(rng, n):
    """(n,4) uniform Montgomery words in [0, p) for the active curve: rejection sampling over 254 bits"""
    out = []
    while len(out) < n:
        a = rng.integers(0, 2**64, size=(2 * (n - len(out)) + 8, 4), dtype=np.uint64)
        a[:, 3] &= np.uint64(2**62 - 1)
        out += [v for v in ints(a) if v < FR_P]
    return words(out[:n])


def _edge_words():
    p = FR_P
    top = p.bit_length() - 1                       # 2^top < p < 2^(top+1)
    values = [0, 1, 2, p - 1, p - 2, (p - 1) // 2, (p + 1) // 2, 2**top - 1, 2**top, 2**(top - 1) - 1, 2**(top - 1)]
    mem = [to_mont(v, p) for v in values]          # edges in value space, as Montgomery words
    for k in range(1, 9):                          # edges in limb space (the 29-bit limbs the kernels compute in)
        mem += [2**(29 * k) - 1, 2**(29 * k)]
    low = 2**232 - 1                               # limbs 0..7 all 2^29 - 1, limb 8 as large as p allows
    mem += [p - 1, 1, low + ((p - 1 - low) >> 232 << 232)]
    seen = []
    for w in mem:
        if w not in seen:
            seen.append(w)
    assert all(0 <= w < p for w in seen)
    return seen


EDGE = _edge_words()


def edge_fr(idx):
    """rows of EDGE picked by index (cycled)"""
    return words([EDGE[i % len(EDGE)] for i in idx])


def mont(v):
    """the Montgomery memory word of the field element v"""
    return to_mont(int(v) % FR_P, FR_P)


def lift(rows, k=None, rng=None):
    """every word x -> x + k*p, another representative of the same residue below LAZY_BOUND.  k=None: the largest such k for each element;
    rng: a uniform per-element k in [0, that largest k]; an int k: that k, clipped to the largest"""
    out = []
    for x in ints(rows):
        kmax = (LAZY_BOUND - 1 - x) // FR_P
        kk = kmax if k is None and rng is None else (int(rng.integers(0, kmax + 1)) if rng is not None else min(int(k), kmax))
        out.append(x + kk * FR_P)
    return words(out).reshape(np.asarray(rows).shape)


def canon(rows):
    """canonical representatives of Montgomery-form rows (any 256-bit value of the same residue -> the value in [0, p))"""
    shape = np.asarray(rows).shape
    return words([x % FR_P for x in ints(rows)]).reshape(shape)
