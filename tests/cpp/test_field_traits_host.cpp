// Prints every constant of every modulus trait of the arithmetic headers (lasso_amd/csrc/fr.cuh, fq.cuh over mont32.cuh; fr29.cuh, fe29.cuh over
// mont29.cuh) as an integer, one `trait.name = 0x...` line each; tests/test_host_arith_cpp.py checks them against Python's big integers.  Built once
// per curve: the traits of the other curve sit behind -DLASSO_BN254.
#include "../../lasso_amd/csrc/fe29.cuh"
#include "../../lasso_amd/csrc/fr29.cuh"
#include <cstdio>

static void hex(const char* trait, const char* name, const uint32_t* w, int n) {
  printf("%s.%s = 0x", trait, name);
  for (int i = n - 1; i >= 0; i--) printf("%08x", w[i]);
  printf("\n");
}
static void small(const char* trait, const char* name, uint64_t x) { printf("%s.%s = 0x%llx\n", trait, name, (unsigned long long)x); }
// nine 29-bit digits (each in [0, 2^29)) -> the integer
static void digits29(const char* trait, const char* name, const int32_t* l) {
  uint32_t w[10] = {0};
  for (int k = 0; k < 9; k++) {
    if (l[k] < 0 || l[k] > M29_MASK) { printf("%s.%s: limb %d out of range\n", trait, name, k); return; }
    const uint64_t x = (uint64_t)(uint32_t)l[k] << ((29 * k) & 31);
    w[(29 * k) >> 5] |= (uint32_t)x; w[((29 * k) >> 5) + 1] |= (uint32_t)(x >> 32);
  }
  hex(trait, name, w, 10);
}

template <class M> static void mont32_trait(const char* trait) {
  uint32_t p[8]; for (int i = 0; i < 8; i++) p[i] = M::p(i);
  hex(trait, "p", p, 8);
  small(trait, "INV32", M::INV32); small(trait, "INV64", M::INV64); small(trait, "WRAPS", (uint64_t)M::WRAPS);
  hex(trait, "ONE", M::one().v, 8); hex(trait, "R2", M::r2().v, 8);
}
#define NINE(M, c) {M::c##_0, M::c##_1, M::c##_2, M::c##_3, M::c##_4, M::c##_5, M::c##_6, M::c##_7, M::c##_8}
template <class M> static void mont29_modulus(const char* trait) {
  int32_t p[9]; for (int k = 0; k < 9; k++) p[k] = M::p(k);
  const int32_t one_s[9] = NINE(M, ONE_S);
  digits29(trait, "p", p); small(trait, "PINV", M::PINV); digits29(trait, "ONE_S", one_s);
}
template <class M> static void mont29_reciprocal(const char* trait) {   // what only the general-modulus reductions use
  const int32_t k522[9] = NINE(M, K522);
  small(trait, "QC", (uint64_t)M::QC); digits29(trait, "K522", k522);
}
template <class M> static void mont29_radix(const char* trait) {
  digits29(trait, "K5", M::k5().v); digits29(trait, "K10", M::k10().v); digits29(trait, "R2S", M::r2s().v);
}

int main() {
#ifdef LASSO_BN254
  mont32_trait<Bn254FrM32>("Bn254FrM32"); mont32_trait<Bn254FqM32>("Bn254FqM32");
  mont29_modulus<Bn254FrM>("Bn254FrM"); mont29_reciprocal<Bn254FrM>("Bn254FrM"); mont29_radix<Bn254FrM>("Bn254FrM");
  mont29_modulus<Bn254FqM>("Bn254FqM"); mont29_reciprocal<Bn254FqM>("Bn254FqM");
#else
  mont32_trait<Curve25519FrM32>("Curve25519FrM32");
  mont29_modulus<Curve25519FrM>("Curve25519FrM"); mont29_radix<Curve25519FrM>("Curve25519FrM");
#endif
  printf("OK\n");
  return 0;
}
