// BN254 build (-DLASSO_BN254) of fq.cuh: Fq = the base field of ark-bn254's G1,
// q = 21888242871839275222246405745257275088696311157297823662689037894645226208583, and the group y^2 = x^3 + 3 over it.
// Unlike the curve25519 header (plain lazy limbs around 2^255 - 19), fq_t here IS ark-ff's in-memory Montgomery form (R = 2^256), always
// canonical, an instance of mont32.cuh; fq_from_mont / fq_to_mont are the identity and stay only so that shared code reads the same.  Points are homogeneous projective
// (X : Y : Z), x = X/Z, y = Y/Z, identity (0 : 1 : 0), under the COMPLETE formulas of Renes-Costello-Batina 2016 (a = 0: algorithms 7-9) — no
// exceptional cases, so bucket sums and trees need no branches.  ed_point keeps the four-coordinate layout of the ABI's lasso_point (t unused,
// zero): ark-ec's `short_weierstrass::Projective` is Jacobian, but the transcript only ever sees the compressed affine point
// (utils/transcript.rs:47-51), so any projective representative is equivalent downstream.
#pragma once
#include <stdint.h>
#include "fr.cuh"

struct alignas(16) fq_t {
  uint32_t v[8];
};

struct Bn254FqM32 : m32_defaults<Bn254FqM32> {
  typedef fq_t T;
  static LHD uint32_t p(int i) {
    const uint32_t P[8] = {0xd87cfd47u, 0x3c208c16u, 0x6871ca8du, 0x97816a91u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    return P[i];
  }
  static constexpr uint32_t INV32 = 0xe4866389u;             // -q^{-1} mod 2^32
  static constexpr uint64_t INV64 = 0x87d20782e4866389ull;   // -q^{-1} mod 2^64
  static constexpr int WRAPS = 8;                            // 2^256 < 6q
  static LHD fq_t one() { return m32_from_limbs<fq_t>(0xc58f0d9du, 0xd35d438du, 0xf5c70b3du, 0x0a78eb28u, 0x7879462cu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u); }  // R mod q
  static LHD fq_t r2() { return m32_from_limbs<fq_t>(0x538afa89u, 0xf32cfc5bu, 0xd44501fbu, 0xb5e71911u, 0x0a417ff6u, 0x47ab1effu, 0xcab8351fu, 0x06d89f71u); }   // R^2 mod q
};
M32_INSTANCE(fq, Bn254FqM32)

static constexpr auto& fq_from_limbs = m32_from_limbs<fq_t>;
LHD fq_t fq_from_mont(const fq_t& a) { return a; }
LHD fq_t fq_to_mont(const fq_t& a) { return a; }
LHD fq_t fq_canonical(const fq_t& a) { return a; }   // values are kept canonical
LHD fq_t fq_inv_chain(const fq_t& a) { return fq_inv(a); }
LHD fq_t fq_mul3(const fq_t& a) { return fq_add(fq_dbl(a), a); }
LHD fq_t fq_mul9(const fq_t& a) { const fq_t t = fq_dbl(fq_dbl(fq_dbl(a))); return fq_add(t, a); }   // b3 = 3 b = 9

struct ed_point { fq_t X, Y, T, Z; };   // (X : Y : Z), T unused (zero): the lasso_point layout
LHD ed_point ed_identity() { ed_point p; p.X = fq_zero(); p.Y = fq_one(); p.T = fq_zero(); p.Z = fq_zero(); return p; }
LHD ed_point ed_from_affine(const fq_t& x, const fq_t& y) { ed_point p; p.X = x; p.Y = y; p.T = fq_zero(); p.Z = fq_one(); return p; }
LHD ed_point ed_neg(const ed_point& p) { ed_point r = p; r.Y = fq_neg(p.Y); return r; }
LHD bool ed_eq(const ed_point& a, const ed_point& b) {
  return fq_eq(fq_mul(a.X, b.Z), fq_mul(b.X, a.Z)) && fq_eq(fq_mul(a.Y, b.Z), fq_mul(b.Y, a.Z)) && fq_eq(fq_mul(a.X, b.Y), fq_mul(b.X, a.Y));
}
// complete addition (RCB16 algorithm 7, a = 0, b3 = 9): 12 products
LHD ed_point ed_add(const ed_point& p, const ed_point& q) {
  fq_t t0 = fq_mul(p.X, q.X), t1 = fq_mul(p.Y, q.Y), t2 = fq_mul(p.Z, q.Z);
  fq_t t3 = fq_sub(fq_sub(fq_mul(fq_add(p.X, p.Y), fq_add(q.X, q.Y)), t0), t1);   // X1Y2 + X2Y1
  fq_t t4 = fq_sub(fq_sub(fq_mul(fq_add(p.Y, p.Z), fq_add(q.Y, q.Z)), t1), t2);   // Y1Z2 + Y2Z1
  fq_t y3 = fq_sub(fq_sub(fq_mul(fq_add(p.X, p.Z), fq_add(q.X, q.Z)), t0), t2);   // X1Z2 + X2Z1
  t0 = fq_mul3(t0); t2 = fq_mul9(t2);
  fq_t z3 = fq_add(t1, t2); t1 = fq_sub(t1, t2); y3 = fq_mul9(y3);
  ed_point r;
  r.X = fq_sub(fq_mul(t3, t1), fq_mul(t4, y3));
  r.Y = fq_add(fq_mul(t1, z3), fq_mul(y3, t0));
  r.Z = fq_add(fq_mul(z3, t4), fq_mul(t0, t3));
  r.T = fq_zero();
  return r;
}
// complete doubling (RCB16 algorithm 9, a = 0)
LHD ed_point ed_dbl(const ed_point& p) {
  fq_t t0 = fq_sqr(p.Y), z3 = fq_dbl(fq_dbl(fq_dbl(t0))), t1 = fq_mul(p.Y, p.Z), t2 = fq_mul9(fq_sqr(p.Z));
  fq_t x3 = fq_mul(t2, z3), y3 = fq_add(t0, t2);
  z3 = fq_mul(t1, z3);
  t0 = fq_sub(t0, fq_mul3(t2));
  ed_point r;
  r.Y = fq_add(fq_mul(t0, y3), x3);
  r.X = fq_dbl(fq_mul(t0, fq_mul(p.X, p.Y)));
  r.Z = z3; r.T = fq_zero();
  return r;
}
LHD ed_point ed_mul_limbs(const ed_point& p, const uint32_t* e) {   // e: canonical 8-limb scalar
  ed_point r = ed_identity();
  for (int i = 255; i >= 0; i--) { r = ed_dbl(r); if ((e[i / 32] >> (i % 32)) & 1) r = ed_add(r, p); }
  return r;
}
