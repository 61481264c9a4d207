"""Python big-integer statements of the entry points that are a line of algebra, on Montgomery memory words of the active curve (fieldref.CURVE).

Independent of the oracle's mock: tests/test_field_edges_cpu.py checks them against the mock, tests/test_gpu_field_edges.py against the device.
Inputs are (n,4) uint64 rows of any representative; outputs are canonical Montgomery rows."""
from fieldref import L as P, R
from gpuutil import ints, words

RINV = pow(R, -1, P)


def val(rows):
    """memory words -> field values (Python ints in [0, p))"""
    return [x * RINV % P for x in ints(rows)]


def mem(vals):
    """field values -> canonical memory words"""
    return words([v * R % P for v in vals])


def bind(z, r):
    """dense_mlpoly.rs:209-216: the lower half after Z[i] <- Z[i] + r (Z[i + n/2] - Z[i])"""
    z = val(z); r = val(r)[0]; h = len(z) // 2
    return mem([(z[i] + r * (z[h + i] - z[i])) % P for i in range(h)])


def eq_evals(r, scale=None):
    """eq_poly.rs:22-38: out[x] = prod_j (x_j ? r_j : 1 - r_j), r[0] <-> the top bit of x; times scale"""
    r = val(r) if len(r) else []
    out = [1 if scale is None else val(scale)[0]]
    for rj in r:
        out = [v * f % P for v in out for f in (1 - rj, rj)]
    return mem(out)


def multi_dot(polys, w):
    w = val(w)
    return mem([sum(a * b for a, b in zip(val(p), w)) % P for p in polys])


def matvec_left(z, lv, ls, rs):
    z = val(z); lv = val(lv)
    return mem([sum(lv[j] * z[j * rs + i] for j in range(ls)) % P for i in range(rs)])


def inner_products_lr(a, b):
    a = val(a); b = val(b); h = len(a) // 2
    return mem([sum(a[i] * b[h + i] for i in range(h)) % P, sum(a[h + i] * b[i] for i in range(h)) % P])


def fingerprint_ops(table, dim, read, gamma, tau):
    """memory_checking.rs:284-301: (read, write) fingerprints a + v gamma + t gamma^2 - tau"""
    t = val(table); rd = val(read); g = val(gamma)[0]; ta = val(tau)[0]
    ro = [(rd[i] * g * g + t[dim[i]] * g + int(dim[i]) - ta) % P for i in range(len(dim))]
    wo = [((rd[i] + 1) * g * g + t[dim[i]] * g + int(dim[i]) - ta) % P for i in range(len(dim))]
    return mem(ro), mem(wo)


def fingerprint_mem(table, final, gamma, tau):
    """memory_checking.rs:257-273: (init, final) fingerprints"""
    t = val(table); f = val(final); g = val(gamma)[0]; ta = val(tau)[0]
    io = [(t[i] * g + i - ta) % P for i in range(len(t))]
    fo = [(f[i] * g * g + t[i] * g + i - ta) % P for i in range(len(t))]
    return mem(io), mem(fo)


def cubic_eqw_round(A, B, E, n):
    """the three sums of lasso_sumcheck_cubic_eqw_round: sum_i A(x)[i] B(x)[i] E[i] at x = 0, 2, 3, per circuit"""
    e = val(E); h = n // 2
    out = []
    for a, b in zip(A, B):
        a = val(a); b = val(b)
        for x in (0, 2, 3):
            out.append(sum((a[i] + x * (a[h + i] - a[i])) * (b[i] + x * (b[h + i] - b[i])) * e[i] for i in range(h)) % P)
    return mem(out)


def bullet_fold(a, b, w, u, u_inv):
    """bullet.rs:127-131: a' = a_lo u + a_hi u^-1, b' = b_lo u^-1 + b_hi u, weights w -> (w u^-1, w u) interleaved"""
    a = val(a); b = val(b); w = val(w); u = val(u)[0]; ui = val(u_inv)[0]; h = len(a) // 2
    fa = [(a[i] * u + ui * a[h + i]) % P for i in range(h)]
    fb = [(b[i] * ui + u * b[h + i]) % P for i in range(h)]
    fw = []
    for x in w:
        fw += [x * ui % P, x * u % P]
    return mem(fa), mem(fb), mem(fw)

