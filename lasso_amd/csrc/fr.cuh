// Fr, the scalar field of the build's curve, as 8 x u32 Montgomery limbs (R = 2^256): an instance of mont32.cuh.
//   curve25519:            p = 2^252 + 27742317777372353535851937790883648493
//   BN254 (-DLASSO_BN254): the order of ark-bn254's G1 (bn254_fr.cuh) — byte-identical to ark-ff's `Fp256<MontBackend<FrConfig, 4>>`; the modulus
//                          has no structure to exploit, so the reduction rows are full.
//
// gfx950 notes: the curve25519 modulus limbs 4..6 are zero and limb 7 is 2^28, which the unrolled reduction folds into
// carries and a shift (4 mads + 1 mul per reduction row instead of 8).
#pragma once
#include "mont32.cuh"

struct alignas(16) fr_t {
  uint32_t v[8];
};

#ifdef LASSO_BN254
#include "bn254_fr.cuh"   // the trait of ark-bn254's Fr
#else
struct Curve25519FrM32 : m32_defaults<Curve25519FrM32> {
  typedef fr_t T;
  static constexpr uint32_t FR_P0 = 0x5cf5d3edu, FR_P1 = 0x5812631au, FR_P2 = 0xa2f79cd6u, FR_P3 = 0x14def9deu, FR_P7 = 0x10000000u;   // limbs 4..6 are zero
  static LHD uint32_t p(int i) { return i == 0 ? FR_P0 : i == 1 ? FR_P1 : i == 2 ? FR_P2 : i == 3 ? FR_P3 : i == 7 ? FR_P7 : 0u; }
  static constexpr uint32_t INV32 = 0x12547e1bu;             // -p^{-1} mod 2^32
  static constexpr uint64_t INV64 = 0xd2b51da312547e1bull;   // -p^{-1} mod 2^64
  static constexpr int WRAPS = 16;                           // 2^256 < 16p
  static LHD fr_t one() { return m32_from_limbs<fr_t>(0x8d98951du, 0xd6ec3174u, 0x737dcf70u, 0xc6ef5bf4u, 0xfffffffeu, 0xffffffffu, 0xffffffffu, 0x0fffffffu); }  // R mod p
  static LHD fr_t r2() { return m32_from_limbs<fr_t>(0x449c0f01u, 0xa40611e3u, 0x68859347u, 0xd00e1ba7u, 0x17f5be65u, 0xceec73d2u, 0x7c309a3du, 0x0399411bu); }   // R^2 mod p
  static LHD bool geq_p(const uint32_t* a) {
    // compare from the top; limbs 4..6 of p are zero
    if (a[7] != FR_P7) return a[7] > FR_P7;
    if (a[6] | a[5] | a[4]) return true;
    if (a[3] != FR_P3) return a[3] > FR_P3;
    if (a[2] != FR_P2) return a[2] > FR_P2;
    if (a[1] != FR_P1) return a[1] > FR_P1;
    return a[0] >= FR_P0;
  }
  static constexpr bool OWN_ROW32 = true;
  static LHD void row32(uint32_t* t, uint32_t m) {
    uint64_t c = (uint64_t)m * FR_P0 + t[0]; c >>= 32;
    c += (uint64_t)m * FR_P1 + t[1]; t[0] = (uint32_t)c; c >>= 32;
    c += (uint64_t)m * FR_P2 + t[2]; t[1] = (uint32_t)c; c >>= 32;
    c += (uint64_t)m * FR_P3 + t[3]; t[2] = (uint32_t)c; c >>= 32;
    c += t[4]; t[3] = (uint32_t)c; c >>= 32;
    c += t[5]; t[4] = (uint32_t)c; c >>= 32;
    c += t[6]; t[5] = (uint32_t)c; c >>= 32;
    c += ((uint64_t)m << 28) + t[7]; t[6] = (uint32_t)c; c >>= 32;
    c += t[8]; t[7] = (uint32_t)c; c >>= 32;
    t[8] = t[9] + (uint32_t)c;
  }
};
typedef Curve25519FrM32 FrM32;
#ifdef M32_HOST_LIMBS64
// The host's 64-bit product, hand-unrolled over the sparse limbs (P2 = 0): the prover's tails sit on the headline's critical path, and the
// generic loop of mont32.cuh does not compile to the same instructions for this modulus.
template <> inline fr_t m32_mul<Curve25519FrM32, fr_t>(const fr_t& a, const fr_t& b) {
  typedef unsigned __int128 u128;
  const uint64_t P0 = 0x5812631a5cf5d3edull, P1 = 0x14def9dea2f79cd6ull, P3 = 0x1000000000000000ull, INV = Curve25519FrM32::INV64;
  uint64_t x[4], y[4]; __builtin_memcpy(x, a.v, 32); __builtin_memcpy(y, b.v, 32);
  uint64_t t0 = 0, t1 = 0, t2 = 0, t3 = 0, t4 = 0;
#define FR64_ROW(yi)                                                                                   \
  {                                                                                                    \
    u128 c = (u128)x[0] * (yi) + t0; t0 = (uint64_t)c; c >>= 64;                                        \
    c += (u128)x[1] * (yi) + t1; t1 = (uint64_t)c; c >>= 64;                                            \
    c += (u128)x[2] * (yi) + t2; t2 = (uint64_t)c; c >>= 64;                                            \
    c += (u128)x[3] * (yi) + t3; t3 = (uint64_t)c; c >>= 64;                                            \
    c += t4; t4 = (uint64_t)c; const uint64_t t5 = (uint64_t)(c >> 64);                                 \
    const uint64_t m = t0 * INV;                                                                     \
    c = (u128)m * P0 + t0; c >>= 64;                                                                    \
    c += (u128)m * P1 + t1; t0 = (uint64_t)c; c >>= 64;                                                 \
    c += t2; t1 = (uint64_t)c; c >>= 64;                                                                \
    c += (u128)m * P3 + t3; t2 = (uint64_t)c; c >>= 64;                                                 \
    c += t4; t3 = (uint64_t)c; c >>= 64;                                                                \
    t4 = t5 + (uint64_t)c;                                                                            \
  }
  FR64_ROW(y[0]) FR64_ROW(y[1]) FR64_ROW(y[2]) FR64_ROW(y[3])
#undef FR64_ROW
  // result < 2p < 2^254: conditional subtraction of p on 64-bit limbs
  u128 d = (u128)t0 - P0; const uint64_t s0 = (uint64_t)d; uint64_t bw = (uint64_t)(d >> 64) & 1;
  d = (u128)t1 - P1 - bw; const uint64_t s1 = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1;
  d = (u128)t2 - bw; const uint64_t s2 = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1;
  d = (u128)t3 - P3 - bw; const uint64_t s3 = (uint64_t)d; bw = (uint64_t)(d >> 64) & 1;
  const uint64_t keep = (uint64_t)0 - bw;   // borrow: the value was < p
  uint64_t r[4] = {(t0 & keep) | (s0 & ~keep), (t1 & keep) | (s1 & ~keep), (t2 & keep) | (s2 & ~keep), (t3 & keep) | (s3 & ~keep)};
  fr_t o; __builtin_memcpy(o.v, r, 32);
  return o;
}
#endif
#endif

M32_INSTANCE(fr, FrM32)
