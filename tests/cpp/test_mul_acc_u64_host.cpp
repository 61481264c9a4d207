// CPU check of fr29_mul_acc_u64 / fr29_acc_carry_u64 (lasso_amd/csrc/mont29.cuh, fr29.cuh): the product of a 64-bit INTEGER with a field element in 27 multiply-adds, the
// arithmetic of k_matvec_left_u64 (poly_u64_kernels.cuh), driven the way the kernel's per-thread loop drives it, against fr.cuh's Montgomery arithmetic (which
// tests/cpp/test_arith_host.cpp pins to the oracle).  Operands that are not canonical (a lazily reduced word, the all-ones word) have no fr_mul statement: there the reference
// is fr29_mul on the lifted integer, which tests/cpp/test_fr29_host.cpp pins to fr_mul, and the two all-ones sums are printed for tests/test_poly_commit_cpu.py to check
// against Python integers.  Built plain and with -fsanitize=undefined: the claim that FR29_U64_ACC_PERIOD products fit between two carry passes is a claim about signed
// 64-bit columns.
#include "../../lasso_amd/csrc/fr29.cuh"
#include <random>
#include <cstdio>
#include <cstring>
#include <vector>

#ifdef LASSO_BN254
#define FR_TOP_SHAVE 2
#else
#define FR_TOP_SHAVE 3
#endif
static std::mt19937_64 rng(777);
static fr_t rand_fr() { for (;;) { uint64_t l[4]; for (int i = 0; i < 4; i++) l[i] = rng(); l[3] &= (~0ull) >> FR_TOP_SHAVE; fr_t t; memcpy(t.v, l, 32); if (!fr_geq_p(t.v)) return t; } }
static bool same(const fr_t& a, const fr_t& b) { return memcmp(a.v, b.v, 32) == 0; }
#define CHECK(c) do { if (!(c)) { printf("FAIL %s line %d\n", #c, __LINE__); return 1; } } while (0)

// what the kernel writes for a finished accumulator
static fr_t finish(fr29_acc w) { fr29_acc_carry_u64(w); return fr29_store(fr29_mul(fr29_acc_reduce(w), fr29_r2s())); }
// z * L as the 32-byte route states it: the lifted integer (u-form) times L in s-form
static fr_t lifted_product(uint64_t z, const fr_t& L) { return fr29_store(fr29_mul(fr29_mul(fr29_from_u64_int(z), fr29_r2s()), fr29_unpack_s(L))); }
static void print_word(const char* name, const fr_t& w) { printf("%s = ", name); for (int i = 7; i >= 0; i--) printf("%08x", w.v[i]); printf("\n"); }

int main() {
  std::vector<uint64_t> zs{0, 1, (1ull << 29) - 1, 1ull << 29, 1ull << 58, ~0ull, (1ull << 58) - 1, (1ull << 29) + 1, 0x8000000000000000ull};
  for (int i = 0; i < 300; i++) zs.push_back(rng() >> (i % 64));
  std::vector<fr_t> Ls{fr_zero(), fr_one(), fr_neg(fr_one()), fr_from_u64(~0ull)};
  for (int i = 0; i < 60; i++) Ls.push_back(rand_fr());
  // one product, every z against every L
  for (uint64_t z : zs) for (const fr_t& L : Ls) {
    fr29_acc w = fr29_acc_zero();
    fr29_mul_acc_u64(w, z, fr29_unpack_s(L));
    const fr_t got = finish(w);
    CHECK(same(got, fr_mul(fr_from_u64(z), L)));
    CHECK(same(got, lifted_product(z, L)));
  }
  // Operands at the edge of what a device array may hold and beyond: the largest representative below 2^254 + 2^130 of p - 1, and the all-ones word (every limb of its
  // s-form is 2^29 - 1 except the lowest: the masks admit nothing larger).  FR29_U64_ACC_PERIOD products of 2^64 - 1 between carries, and the same number again after one.
  fr_t lazy, ones;
  {
    for (int i = 0; i < 8; i++) ones.v[i] = 0xffffffffu;
    fr_t pm1; for (int i = 0; i < 8; i++) pm1.v[i] = fr_p_limb(i); pm1.v[0] -= 1u;      // the memory integer p - 1
    lazy = pm1;
    for (;;) {   // + p while the sum stays below 2^254 + 2^130
      uint64_t c = 0; fr_t nx;
      for (int i = 0; i < 8; i++) { const uint64_t t = (uint64_t)lazy.v[i] + fr_p_limb(i) + c; nx.v[i] = (uint32_t)t; c = t >> 32; }
      const bool below = !c && (nx.v[7] < 0x40000000u || (nx.v[7] == 0x40000000u && nx.v[6] == 0 && nx.v[5] == 0 && nx.v[4] < 4));
      if (!below) break;
      lazy = nx;
    }
  }
  for (const fr_t* Lp : {&lazy, &ones}) {
    const fr29 Ls29 = fr29_unpack_s(*Lp);
    for (int k = 0; k < 9; k++) CHECK(Ls29.v[k] >= 0 && Ls29.v[k] < (1 << 29));
    fr29_acc w = fr29_acc_zero(); fr29 ref = fr29_zero();
    const fr29 one_prod = fr29_unpack_u(lifted_product(~0ull, *Lp));
    for (int pass = 0; pass < 2; pass++) {
      for (int i = 0; i < FR29_U64_ACC_PERIOD; i++) { fr29_mul_acc_u64(w, ~0ull, Ls29); ref = fr29_unpack_u(fr29_store(fr29_add(ref, one_prod))); }
      for (int k = 0; k < 17; k++) CHECK(w.h[k] >= 0);                         // no column has wrapped
      fr29_acc_carry_u64(w);
      for (int k = 0; k < 11; k++) CHECK(w.h[k] >= 0 && w.h[k] < (1 << 29));
      for (int k = 12; k < 17; k++) CHECK(w.h[k] == 0);
      const fr_t got = finish(w);
      CHECK(same(got, fr29_store(ref)));
      if (Lp == &ones) print_word(pass ? "ONES30" : "ONES15", got);
    }
  }
  // the full carry pass of the 9 x 9 accumulator serves as well (the two passes agree on what they leave in columns 0..11)
  {
    fr29_acc a = fr29_acc_zero(), b = fr29_acc_zero();
    for (int i = 0; i < FR29_U64_ACC_PERIOD; i++) { fr29_mul_acc_u64(a, zs[5 + i], fr29_unpack_s(Ls[3 + i])); fr29_mul_acc_u64(b, zs[5 + i], fr29_unpack_s(Ls[3 + i])); }
    fr29_acc_carry(a); fr29_acc_carry_u64(b);
    for (int k = 0; k < 17; k++) CHECK(a.h[k] == b.h[k]);
  }
  // column sums as the kernel's loop forms them: T terms, a carry pass every FR29_U64_ACC_PERIOD, vs the running sum of Montgomery products
  for (int T : {1, 2, 14, 15, 16, 29, 30, 31, 4096, 1 << 20}) {
    fr29_acc w = fr29_acc_zero(); fr_t ref = fr_zero(); uint32_t cnt = 0;
    for (int i = 0; i < T; i++) {
      const uint64_t z = T == (1 << 20) && (i & 3) ? ~0ull - (uint64_t)i : zs[(size_t)i % zs.size()];      // the long sum: mostly near 2^64
      const fr_t& L = Ls[((size_t)i * 7 + 1) % Ls.size()];
      fr29_mul_acc_u64(w, z, fr29_unpack_s(L));
      if (++cnt == FR29_U64_ACC_PERIOD) { fr29_acc_carry_u64(w); cnt = 0; }
      ref = fr_add(ref, fr_mul(fr_from_u64(z), L));
    }
    CHECK(same(finish(w), ref));
  }
  printf("OK\n");
  return 0;
}
