// The BN254 build's Fr as a trait of mont32.cuh: the order of ark-bn254's G1,
// p = 21888242871839275222246405745257275088548364400416034343698204186575808495617 (254 bits).  Included by fr.cuh, after fr_t, in place of the
// curve25519 trait; the modulus has no structure to exploit, so every function is mont32.cuh's own.
#pragma once
struct Bn254FrM32 : m32_defaults<Bn254FrM32> {
  typedef fr_t T;
  static LHD uint32_t p(int i) {
    const uint32_t P[8] = {0xf0000001u, 0x43e1f593u, 0x79b97091u, 0x2833e848u, 0x8181585du, 0xb85045b6u, 0xe131a029u, 0x30644e72u};
    return P[i];
  }
  static constexpr uint32_t INV32 = 0xefffffffu;             // -p^{-1} mod 2^32
  static constexpr uint64_t INV64 = 0xc2e1f593efffffffull;   // -p^{-1} mod 2^64
  static constexpr int WRAPS = 8;                            // 2^256 < 6p
  static LHD fr_t one() { return m32_from_limbs<fr_t>(0x4ffffffbu, 0xac96341cu, 0x9f60cd29u, 0x36fc7695u, 0x7879462eu, 0x666ea36fu, 0x9a07df2fu, 0x0e0a77c1u); }  // R mod p
  static LHD fr_t r2() { return m32_from_limbs<fr_t>(0xae216da7u, 0x1bb8e645u, 0xe35c59e3u, 0x53fe3ab1u, 0x53bb8085u, 0x8c49833du, 0x7f4e44a5u, 0x0216d0b1u); }   // R^2 mod p
};
typedef Bn254FrM32 FrM32;
