"""Helpers of the compressed-point tests (tests/test_wire_points_cpu.py, tests/test_gpu_wire_points.py): a big-integer decoder of ark-serialize compressed points written
from ark-ec's rules (NOT from the product's C++), crafted encodings for both curves, a walker of the proof's wire format that finds every point and scalar, and the CPU
build of the host prover against the mock with the device decoder added (tests/cpp/mock_wire_wrap.cpp)."""
import os

import numpy as np
from mockbuild import build_mock_prover

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

OK, OK_IDENTITY, NONCANONICAL, BAD_FLAGS, NOT_ON_CURVE, NOT_IN_SUBGROUP = range(6)

# ---------------------------------------------------------------- edwards25519 as ark-curve25519 states it: -x^2 + y^2 = 1 + d x^2 y^2, cofactor 8
P25 = 2**255 - 19
D25 = (-121665 * pow(121666, -1, P25)) % P25
L25 = 2**252 + 27742317777372353535851937790883648493
BASE25 = (15112221349535400772501151409588531511454012693041857206046113283949847762202, 46316835694926478169428394003475163141307993866256225615783033603165251855960)


def ed_add(a, b):
    (x1, y1), (x2, y2) = a, b
    k = D25 * x1 * x2 * y1 * y2 % P25
    return ((x1 * y2 + x2 * y1) * pow(1 + k, -1, P25) % P25, (y1 * y2 + x1 * x2) * pow(1 - k, -1, P25) % P25)      # a = -1: y3 = (y1 y2 - a x1 x2) / (1 - k)


def ed_mul(k, pt):
    # extended coordinates without inversions (add-2008-hwcd-3 is complete on this curve), one inversion at the end
    def add(p, q):
        X1, Y1, Z1, T1 = p; X2, Y2, Z2, T2 = q
        A = (Y1 - X1) * (Y2 - X2) % P25; B = (Y1 + X1) * (Y2 + X2) % P25; C = 2 * D25 * T1 * T2 % P25; Dd = 2 * Z1 * Z2 % P25
        E, F, G, H = B - A, Dd - C, Dd + C, B + A
        return (E * F % P25, G * H % P25, F * G % P25, E * H % P25)
    acc = (0, 1, 1, 0); q = (pt[0], pt[1], 1, pt[0] * pt[1] % P25)
    while k:
        if k & 1:
            acc = add(acc, q)
        q = add(q, q); k >>= 1
    zi = pow(acc[2], -1, P25)
    return (acc[0] * zi % P25, acc[1] * zi % P25)


def sqrt25(a):
    """a square root of a mod 2^255 - 19 (p = 5 mod 8), or None"""
    a %= P25
    r = pow(a, (P25 + 3) // 8, P25)
    if r * r % P25 != a:
        r = r * pow(2, (P25 - 1) // 4, P25) % P25
    return r if r * r % P25 == a else None


def ed_on_curve(x, y):
    return (-x * x + y * y - 1 - D25 * x * x * y * y) % P25 == 0


def mont_words(v, p):
    return ((v << 256) % p).to_bytes(32, "little")


def decode25(b):
    """ark-ec twisted_edwards Affine::deserialize_with_mode(Compress::Yes, Validate::Yes): (status, affine 64 bytes, canonical 32 bytes)"""
    zero = (bytes(64), bytes(32))
    v = int.from_bytes(b, "little")
    flag, y = v >> 255, v & (2**255 - 1)
    if y >= P25:                                   # Fq::deserialize_with_flags: the masked integer must be a field element
        return (NONCANONICAL, *zero)
    # get_xs_from_y_unchecked: x^2 = (1 - y^2) / (a - d y^2), a = -1; (smaller, larger) root; TEFlags::XIsNegative picks the larger
    den = (-1 - D25 * y * y) % P25
    if den == 0:
        return (NOT_ON_CURVE, *zero)
    x = sqrt25((1 - y * y) * pow(den, -1, P25))
    if x is None:
        return (NOT_ON_CURVE, *zero)
    small, large = min(x, P25 - x if x else 0), max(x, P25 - x if x else 0)
    x = large if flag else small
    assert ed_on_curve(x, y)
    if ed_mul(L25, (x, y)) != (0, 1):              # is_in_correct_subgroup_assuming_on_curve
        return (NOT_IN_SUBGROUP, *zero)
    canon = y | ((1 << 255) if x > (P25 - x) % P25 else 0)
    return (OK, mont_words(x, P25) + mont_words(y, P25), canon.to_bytes(32, "little"))


def enc25(pt, flip=False):
    x, y = pt
    neg = x > (P25 - x) % P25
    return (y | ((1 << 255) if neg != flip else 0)).to_bytes(32, "little")


def torsion25():
    """the eight points of order dividing 8, from cofactor clearing the other way: [l]Q for curve points Q until one has order 8"""
    y = 2
    while True:
        y += 1
        den = (-1 - D25 * y * y) % P25
        x = sqrt25((1 - y * y) * pow(den, -1, P25))
        if x is None:
            continue
        t = ed_mul(L25, (x, y))
        if ed_mul(4, t) != (0, 1):
            break
    pts, cur = [], (0, 1)
    for _ in range(8):
        pts.append(cur); cur = ed_add(cur, t)
    assert cur == (0, 1) and len(set(pts)) == 8
    return pts


def crafted25():
    """(label, 32 bytes, expected status) — the cases the host and device decoders must agree on"""
    out = []
    subgroup = [ed_mul(k, BASE25) for k in (1, 2, 3, 7, L25 - 1, 2**200 + 12345, 987654321987654321)]
    for i, pt in enumerate(subgroup):
        out.append((f"subgroup{i}", enc25(pt), OK)); out.append((f"subgroup{i}-other-root", enc25(pt, flip=True), OK))
    out.append(("identity", (1).to_bytes(32, "little"), OK)); out.append(("identity-flag", (1 | 1 << 255).to_bytes(32, "little"), OK))      # x = 0: both flag values are the same point
    out.append(("order2", (P25 - 1).to_bytes(32, "little"), NOT_IN_SUBGROUP)); out.append(("order2-flag", (P25 - 1 | 1 << 255).to_bytes(32, "little"), NOT_IN_SUBGROUP))
    for v in (P25, P25 + 1, 2**255 - 1, P25 + 18):
        out.append((f"y={v - P25}+p", v.to_bytes(32, "little"), NONCANONICAL)); out.append((f"y={v - P25}+p-flag", (v | 1 << 255).to_bytes(32, "little"), NONCANONICAL))
    y, found = 1, 0
    while found < 6:                               # y with (1 - y^2) / (-1 - d y^2) a non-residue
        y += 1
        if sqrt25((1 - y * y) * pow((-1 - D25 * y * y) % P25, -1, P25)) is None:
            out.append((f"nonresidue-y={y}", (y | (found & 1) << 255).to_bytes(32, "little"), NOT_ON_CURVE)); found += 1
    tors = torsion25()
    for i, t in enumerate(tors):
        out.append((f"torsion{i}", enc25(t), OK if t == (0, 1) else NOT_IN_SUBGROUP))
    for i, t in enumerate(tors[1:]):
        s = ed_add(subgroup[i % len(subgroup)], t)
        assert ed_on_curve(*s)
        out.append((f"subgroup+torsion{i + 1}", enc25(s), NOT_IN_SUBGROUP)); out.append((f"subgroup+torsion{i + 1}-other-root", enc25(s, flip=True), NOT_IN_SUBGROUP))
    out.append(("zero", bytes(32), None))      # y = 0: x^2 = -1, a square (p = 1 mod 4) — a point of order 4; the status is the reference decoder's
    return [(n, b, st if st is not None else decode25(b)[0]) for n, b, st in out]


# ---------------------------------------------------------------- ark-bn254 G1: y^2 = x^3 + 3 over Fq, cofactor 1
Q254 = 21888242871839275222246405745257275088696311157297823662689037894645226208583


def sw_add(a, b):
    if a is None:
        return b
    if b is None:
        return a
    (x1, y1), (x2, y2) = a, b
    if x1 == x2 and (y1 + y2) % Q254 == 0:
        return None
    lam = (3 * x1 * x1 * pow(2 * y1, -1, Q254) if a == b else (y2 - y1) * pow(x2 - x1, -1, Q254)) % Q254
    x3 = (lam * lam - x1 - x2) % Q254
    return (x3, (lam * (x1 - x3) - y1) % Q254)


def sw_mul(k, pt):
    acc = None
    while k:
        if k & 1:
            acc = sw_add(acc, pt)
        pt = sw_add(pt, pt); k >>= 1
    return acc


def decode254(b):
    """ark-ec short_weierstrass Affine::deserialize_with_mode(Compress::Yes, Validate::Yes)"""
    zero = (bytes(64), bytes(32))
    v = int.from_bytes(b, "little")
    neg, inf, x = v >> 255 & 1, v >> 254 & 1, v & (2**254 - 1)
    if neg and inf:                                # SWFlags::from_u8: no such value
        return (BAD_FLAGS, *zero)
    if x >= Q254:                                  # read before the flags are acted on
        return (NONCANONICAL, *zero)
    if inf:
        return (OK_IDENTITY, bytes(64), bytes(31) + b"\x40")
    rhs = (x * x * x + 3) % Q254
    y = pow(rhs, (Q254 + 1) // 4, Q254)
    if y * y % Q254 != rhs:
        return (NOT_ON_CURVE, *zero)
    small, large = min(y, (Q254 - y) % Q254), max(y, (Q254 - y) % Q254)
    y = large if neg else small
    canon = x | ((1 << 255) if y > (Q254 - y) % Q254 else 0)
    return (OK, mont_words(x, Q254) + mont_words(y, Q254), canon.to_bytes(32, "little"))


def enc254(pt, flip=False):
    x, y = pt
    neg = y > (Q254 - y) % Q254
    return (x | ((1 << 255) if neg != flip else 0)).to_bytes(32, "little")


def crafted254():
    out = []
    for i, k in enumerate((1, 2, 3, 5, 2**100 + 7, 31337, 2**253 + 99)):
        pt = sw_mul(k, (1, 2))
        out.append((f"point{i}", enc254(pt), OK)); out.append((f"point{i}-other-root", enc254(pt, flip=True), OK))
    out.append(("identity", bytes(31) + b"\x40", OK_IDENTITY))
    out.append(("infinity-x=1", (1 | 1 << 254).to_bytes(32, "little"), OK_IDENTITY)); out.append(("infinity-x=q-1", (Q254 - 1 | 1 << 254).to_bytes(32, "little"), OK_IDENTITY))
    out.append(("infinity-x=q", (Q254 | 1 << 254).to_bytes(32, "little"), NONCANONICAL)); out.append(("infinity-x=2^254-1", (2**254 - 1 | 1 << 254).to_bytes(32, "little"), NONCANONICAL))
    out.append(("both-flags", (1 | 3 << 254).to_bytes(32, "little"), BAD_FLAGS)); out.append(("both-flags-noncanonical", (Q254 | 3 << 254).to_bytes(32, "little"), BAD_FLAGS))
    for v in (Q254, Q254 + 1, 2**254 - 1):
        out.append((f"x={v - Q254}+q", v.to_bytes(32, "little"), NONCANONICAL)); out.append((f"x={v - Q254}+q-flag", (v | 1 << 255).to_bytes(32, "little"), NONCANONICAL))
    x, found = 0, 0
    while found < 6:
        x += 1
        rhs = (x * x * x + 3) % Q254
        if pow(rhs, (Q254 - 1) // 2, Q254) != 1:
            out.append((f"nonresidue-x={x}", (x | (found & 1) << 255).to_bytes(32, "little"), NOT_ON_CURVE)); found += 1
    out.append(("zero", bytes(32), decode254(bytes(32))[0]))
    return out


def crafted(curve):
    return crafted254() if curve == "bn254" else crafted25()


def decode(curve, b):
    return decode254(b) if curve == "bn254" else decode25(b)


def random_valid(curve, n, seed):
    """n encodings of valid points: small multiples chain of a random multiple of the generator (cheap to make in Python), both roots mixed"""
    rng = np.random.default_rng(seed)
    k0 = int.from_bytes(rng.bytes(31), "little") + 1
    out = []
    if curve == "bn254":
        step = sw_mul(k0, (1, 2)); cur = step
        for i in range(n):
            out.append(enc254(cur, flip=bool(i & 1))); cur = sw_add(cur, step)
    else:
        step = ed_mul(k0, BASE25); cur = step
        for i in range(n):
            out.append(enc25(cur, flip=bool(i & 1))); cur = ed_add(cur, step)
    return out


# ---------------------------------------------------------------- the proof's wire format (ark-serialize, compressed): where the points and the scalars are

def walk_proof(proof, alpha, c):
    """offsets of every 32-byte point and scalar of a SparsePolynomialEvaluationProof in stream order: (points, scalars).  Vec<T> = u64 length + items."""
    pos, pts, scs = 0, [], []

    def u64():
        nonlocal pos
        v = int.from_bytes(proof[pos:pos + 8], "little"); pos += 8
        return v

    def pt():
        nonlocal pos
        pts.append(pos); pos += 32

    def sc():
        nonlocal pos
        scs.append(pos); pos += 32

    def vec(item):
        for _ in range(u64()):
            item()

    def sumcheck():
        vec(lambda: vec(sc))

    def dpl():
        vec(pt); vec(pt); pt(); pt(); sc(); sc()

    def bgpa():
        def layer():
            sumcheck(); vec(sc); vec(sc)
        vec(layer)

    vec(pt); sumcheck(); sc()
    for _ in range(alpha):
        sc()
    dpl()
    for _ in range(4 * alpha):
        sc()
    bgpa(); bgpa()
    for _ in range(3 * c + alpha):
        sc()
    dpl(); dpl(); dpl()
    assert pos == len(proof), (pos, len(proof))
    return pts, scs


def commitment_points(comm):
    """offsets of the rows of a commitment ([u64 n][n x 32] twice)"""
    pos, pts = 0, []
    for _ in range(2):
        n = int.from_bytes(comm[pos:pos + 8], "little"); pos += 8
        pts += [pos + 32 * i for i in range(n)]; pos += 32 * n
    assert pos == len(comm)
    return pts


def build_mock_prover_wire(curve="curve25519"):
    """the host prover over the mock with the device decoder (tests/cpp/mock_wire_wrap.cpp: the product's pt_decompress on the host)"""
    return build_mock_prover(curve, ext=("wire",))
