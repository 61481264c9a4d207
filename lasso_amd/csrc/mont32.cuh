// A prime field below 2^255 as 8 x u32 Montgomery limbs (R = 2^256), once for every modulus: fr.cuh (curve25519 Fr; BN254 Fr, trait in bn254_fr.cuh) and
// bn254_fq.cuh (BN254 Fq) are the instances.  The byte layout equals ark-ff's `Fp256<MontBackend<_,4>>` (4 x u64 little endian), so device buffers are bit-for-bit what
// the Rust host would hand over (SURVEY.md §8b "Data representation at the ABI").  Values are always canonical (< p).
//
// T is the element type, a plain `alignas(16) { uint32_t v[8]; }` struct (fr_t, fq_t: ABI and kernel parameter types, so not templates).
// M supplies: T; p(i) (32-bit limbs of p); INV32, INV64 (-p^-1 mod 2^32, 2^64); one(), r2() (R, R^2 mod p); WRAPS (2^256 < WRAPS * p); and
// inherits m32_defaults<M>, whose members it may hide where its modulus earns a shortcut (geq_p; OWN_ROW32 with row32).  The host's 64-bit
// product may be specialised for a trait.
//
// gfx950 notes: every limb product is written as u64 = u32*u32 + u32 so hipcc emits v_mad_u64_u32.
// This header is __host__ __device__: the host prover uses the same arithmetic for its O(log n) tails.
#pragma once
#include <stdint.h>

#ifndef LHD
#if defined(__HIPCC__)
#define LHD __host__ __device__ __forceinline__
#else
#define LHD inline
#endif
#endif

/* LASSO_HOST_LIMBS32: tests force the device form on the host */
#if !defined(__HIPCC__) && defined(__SIZEOF_INT128__) && !defined(LASSO_HOST_LIMBS32)
#define M32_HOST_LIMBS64 1
#endif

template <class T> LHD T m32_from_limbs(uint32_t a0, uint32_t a1, uint32_t a2, uint32_t a3, uint32_t a4, uint32_t a5, uint32_t a6, uint32_t a7) {
  T r; r.v[0] = a0; r.v[1] = a1; r.v[2] = a2; r.v[3] = a3; r.v[4] = a4; r.v[5] = a5; r.v[6] = a6; r.v[7] = a7; return r;
}

template <class M> struct m32_defaults {
  // a >= p ?
  static LHD bool geq_p(const uint32_t* a) {
    for (int i = 7; i >= 0; i--) { const uint32_t pi = M::p(i); if (a[i] != pi) return a[i] > pi; }
    return true;
  }
  static constexpr bool OWN_ROW32 = false;   // a trait with a row32(t, m) of its own (one reduction row of the 32-bit CIOS over t[0..9]) hides this with true
};

template <class M, class T = typename M::T> LHD T m32_zero() { T r; for (int i = 0; i < 8; i++) r.v[i] = 0; return r; }
template <class T> LHD bool m32_is_zero(const T& a) { uint32_t o = 0; for (int i = 0; i < 8; i++) o |= a.v[i]; return o == 0; }
template <class T> LHD bool m32_eq(const T& a, const T& b) { uint32_t o = 0; for (int i = 0; i < 8; i++) o |= a.v[i] ^ b.v[i]; return o == 0; }

// r = a - p if a >= p (a < 2p), branch-free
template <class M> LHD void m32_cond_sub_p(uint32_t* a) {
  uint32_t t[8]; uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { uint64_t d = (uint64_t)a[i] - M::p(i) - bw; t[i] = (uint32_t)d; bw = (d >> 63); }
  // bw == 1  <=>  a < p  => keep a
  uint32_t keep = (uint32_t)0 - (uint32_t)bw;
#pragma unroll
  for (int i = 0; i < 8; i++) a[i] = (a[i] & keep) | (t[i] & ~keep);
}

template <class M, class T> LHD T m32_add(const T& a, const T& b) {
  T r; uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (uint64_t)a.v[i] + b.v[i]; r.v[i] = (uint32_t)c; c >>= 32; }
  // a,b < p < 2^255 so no carry out of 256 bits
  m32_cond_sub_p<M>(r.v);
  return r;
}
template <class M, class T> LHD T m32_sub(const T& a, const T& b) {
  T r; uint64_t bw = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { uint64_t d = (uint64_t)a.v[i] - b.v[i] - bw; r.v[i] = (uint32_t)d; bw = d >> 63; }
  uint32_t m = (uint32_t)0 - (uint32_t)bw;  // add p back when borrowed
  uint64_t c = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) { c += (uint64_t)r.v[i] + (M::p(i) & m); r.v[i] = (uint32_t)c; c >>= 32; }
  return r;
}
template <class M, class T> LHD T m32_neg(const T& a) { return m32_sub<M>(m32_zero<M>(), a); }
template <class M, class T> LHD T m32_dbl(const T& a) { return m32_add<M>(a, a); }

// Montgomery product a*b*R^-1 mod p.
#ifdef M32_HOST_LIMBS64
// Host build (g++, the O(log n) tails of the prover): CIOS over 64-bit limbs with 128-bit products — same function, ~6x faster on x86-64
// than the 32-bit form.  T's bytes are the 4 x u64 little-endian limbs on a little-endian host.
template <class M, class T> inline T m32_mul(const T& a, const T& b) {
  typedef unsigned __int128 u128;
  const uint64_t P[4] = {M::p(0) | (uint64_t)M::p(1) << 32, M::p(2) | (uint64_t)M::p(3) << 32, M::p(4) | (uint64_t)M::p(5) << 32, M::p(6) | (uint64_t)M::p(7) << 32}, INV = M::INV64;
  uint64_t x[4], y[4]; __builtin_memcpy(x, a.v, 32); __builtin_memcpy(y, b.v, 32);
  uint64_t t[6] = {0, 0, 0, 0, 0, 0};
  for (int i = 0; i < 4; i++) {
    u128 c = 0;
    for (int j = 0; j < 4; j++) { c += (u128)x[j] * y[i] + t[j]; t[j] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[4] = (uint64_t)c; t[5] = (uint64_t)(c >> 64);
    const uint64_t m = t[0] * INV;
    c = (u128)m * P[0] + t[0]; c >>= 64;
    for (int j = 1; j < 4; j++) { c += (u128)m * P[j] + t[j]; t[j - 1] = (uint64_t)c; c >>= 64; }
    c += t[4]; t[3] = (uint64_t)c; t[4] = t[5] + (uint64_t)(c >> 64);
  }
  // result < 2p < 2^255
  uint64_t s[4]; uint64_t bw = 0;
  for (int i = 0; i < 4; i++) { u128 d = (u128)t[i] - P[i] - bw; s[i] = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1; }
  const uint64_t keep = (uint64_t)0 - bw;
  uint64_t r[4]; for (int i = 0; i < 4; i++) r[i] = (t[i] & keep) | (s[i] & ~keep);
  T o; __builtin_memcpy(o.v, r, 32);
  return o;
}
#else
// CIOS over 32-bit limbs (device form; also the host form inside hipcc translation units).
template <class M, class T> LHD T m32_mul(const T& a, const T& b) {
  uint32_t t[10];
#pragma unroll
  for (int i = 0; i < 10; i++) t[i] = 0;
#pragma unroll
  for (int i = 0; i < 8; i++) {
    uint64_t c = 0;
    const uint32_t bi = b.v[i];
#pragma unroll
    for (int j = 0; j < 8; j++) { c += (uint64_t)a.v[j] * bi + t[j]; t[j] = (uint32_t)c; c >>= 32; }
    c += t[8]; t[8] = (uint32_t)c; t[9] = (uint32_t)(c >> 32);
    const uint32_t m = t[0] * M::INV32;
    if constexpr (M::OWN_ROW32) M::row32(t, m);
    else {
      c = (uint64_t)m * M::p(0) + t[0]; c >>= 32;
#pragma unroll
      for (int j = 1; j < 8; j++) { c += (uint64_t)m * M::p(j) + t[j]; t[j - 1] = (uint32_t)c; c >>= 32; }
      c += t[8]; t[7] = (uint32_t)c; c >>= 32;
      t[8] = t[9] + (uint32_t)c;
    }
  }
  // result < 2p and p < 2^255, so t[8] == 0
  T r;
#pragma unroll
  for (int i = 0; i < 8; i++) r.v[i] = t[i];
  m32_cond_sub_p<M>(r.v);
  return r;
}
#endif
template <class M, class T> LHD T m32_sqr(const T& a) { return m32_mul<M>(a, a); }

// small integer -> Montgomery form (dense_mlpoly.rs:263-269 `F::from(Z[i] as u64)`)
template <class M, class T = typename M::T> LHD T m32_from_u64(uint64_t x) {
  T t = m32_zero<M>(); t.v[0] = (uint32_t)x; t.v[1] = (uint32_t)(x >> 32);
  return m32_mul<M>(t, M::r2());
}
// Montgomery -> canonical integer limbs
template <class M, class T> LHD T m32_to_canonical(const T& a) { T o = m32_zero<M>(); o.v[0] = 1; return m32_mul<M>(a, o); }
// canonical integer (< 2^256) -> Montgomery
template <class M, class T> LHD T m32_from_canonical(const T& c) {
  T t = c;
  // c may be >= p (up to 2^256-1 < WRAPS * p): subtract while needed
  for (int k = 0; k < M::WRAPS && M::geq_p(t.v); k++) {
    uint64_t bw = 0;
    for (int i = 0; i < 8; i++) { uint64_t d = (uint64_t)t.v[i] - M::p(i) - bw; t.v[i] = (uint32_t)d; bw = d >> 63; }
  }
  return m32_mul<M>(t, M::r2());
}
// a^e, e canonical 8-limb exponent (host-side tails only)
template <class M, class T> LHD T m32_pow(const T& a, const uint32_t* e) {
  T r = M::one();
  for (int i = 255; i >= 0; i--) { r = m32_sqr<M>(r); if ((e[i / 32] >> (i % 32)) & 1) r = m32_mul<M>(r, a); }
  return r;
}
template <class M, class T> LHD T m32_inv(const T& a) {  // Fermat; inverse(0) = 0
  uint32_t e[8]; for (int i = 0; i < 8; i++) e[i] = M::p(i);
  e[0] -= 2u;
  return m32_pow<M>(a, e);
}
// number of significant bits of the canonical value
template <class T> LHD int m32_canonical_bits(const T& c) {
  for (int i = 7; i >= 0; i--) if (c.v[i]) { uint32_t x = c.v[i]; int n = 0; while (x) { n++; x >>= 1; } return 32 * i + n; }
  return 0;
}

// The pre##_* names of an instance (fr_add, fq_mul, ...), what every caller uses, ARE the instantiations: references, not wrapper functions.
// One more inlining layer would send every body through one more round of the optimiser on its way into a kernel, and the carry chains do not
// come out of that with the same instructions.
#define M32_INSTANCE(pre, M)                                                     \
  static constexpr auto& pre##_zero = m32_zero<M, pre##_t>;                      \
  static constexpr auto& pre##_one = M::one;                                     \
  static constexpr auto& pre##_r2 = M::r2;                                       \
  static constexpr auto& pre##_p_limb = M::p;                                    \
  static constexpr auto& pre##_is_zero = m32_is_zero<pre##_t>;                   \
  static constexpr auto& pre##_eq = m32_eq<pre##_t>;                             \
  static constexpr auto& pre##_geq_p = M::geq_p;                                 \
  static constexpr auto& pre##_cond_sub_p = m32_cond_sub_p<M>;                   \
  static constexpr auto& pre##_add = m32_add<M, pre##_t>;                        \
  static constexpr auto& pre##_sub = m32_sub<M, pre##_t>;                        \
  static constexpr auto& pre##_neg = m32_neg<M, pre##_t>;                        \
  static constexpr auto& pre##_dbl = m32_dbl<M, pre##_t>;                        \
  static constexpr auto& pre##_mul = m32_mul<M, pre##_t>;                        \
  static constexpr auto& pre##_sqr = m32_sqr<M, pre##_t>;                        \
  static constexpr auto& pre##_from_u64 = m32_from_u64<M, pre##_t>;              \
  static constexpr auto& pre##_to_canonical = m32_to_canonical<M, pre##_t>;      \
  static constexpr auto& pre##_from_canonical = m32_from_canonical<M, pre##_t>;  \
  static constexpr auto& pre##_pow = m32_pow<M, pre##_t>;                        \
  static constexpr auto& pre##_inv = m32_inv<M, pre##_t>;                        \
  static constexpr auto& pre##_canonical_bits = m32_canonical_bits<pre##_t>;
