// Fr (the scalar field of the build's curve) in nine signed 29-bit limbs — the form the polynomial kernels COMPUTE in: an instance of mont29.cuh.
// curve25519: p = 2^252 + c.  The BN254 build: ark-bn254's Fr, the same interface and the same contracts (u-form / s-form, "reduced" /
// "loose", what the reductions accept), through the general-modulus arithmetic of mont29.cuh.
//
// Memory keeps ark-ff's layout (fr_t: 8 x u32 = 4 x u64, x*2^256 mod p, canonical) because that is the ABI; a kernel unpacks on load,
// works in fr29, and canonicalises + packs on store.  Why another form: on gfx950 v_mad_i64_i32 issues every ~5 cycles and adds into a
// 64-bit column in place, so with 29-bit limbs a schoolbook product is 81 back-to-back multiply-adds with NO carry handling in between
// (nine 2^59 products fit a signed 64-bit column).  The 8 x 32-bit CIOS form (fr.cuh) spends 500 of its 600 instructions per product moving
// carries (v_mov / v_lshl_add_u64); it remains the host form and the reference the tests compare against.
//
// value(a) = sum a.v[k] * 2^(29k), limbs signed, lazily reduced: add/sub are limb-wise with no carries and no modular correction.
//   "reduced": limbs 0..7 in [0, 2^29), limb 8 small and signed  (outputs of fr29_mul, fr29_weak, the unpack functions)
//   "loose":   |limb| <= 2^30                                      (one add/sub of reduced values)
// fr29_mul(a, b) = a*b / 2^261 (mod p), Montgomery with radix 2^29 (curve25519: over the sparse modulus, limbs 5..7 of p are zero, limb 8 = 2^20).
//   requires |a.v[i]| <= 2^30, |b.v[j]| <= 2^29 (a loose, b reduced).  |a*b| < X * 2^261  =>  result in (-X, p + X), reduced.
//   a loose, b reduced -> a*b/2^261 mod p, reduced.  curve25519: 81 + 45 multiply-adds.
//
// The radix is 2^261, memory is 2^256: a product of two "u-form" values (x*2^256) comes out 2^5 short.  Every kernel therefore loads
// ONE operand of each product in "s-form" (x*2^261 = the same bits shifted left by 5, free at unpack time) or corrects a whole sum
// once at the end with a constant (FR29_K5 / FR29_K10).  mul(u, s) = u-form; mul(s, s) = s-form; mul(u, u) = u-form / 2^5.
//
// What changes for BN254 against curve25519:
// every reduction row is full (162 multiply-adds per product instead of 126), the lazy reductions take their quotient from a reciprocal
// (m29_near), and they accept MORE than the curve25519 ones (|value| < 2^258 ~ 21 p against 2^255 ~ 8 p) and return LESS (semi: below
// p (1 + 2^-24) against 4 p), so every kernel whose magnitudes were argued for the curve25519 header in units of p holds here as well:
// products come out in (-X, p + X) with X = |a| |b| / 2^261 — three times larger relative to p (p / 2^261 = 2^-7.4 against 2^-9), still below p
// for every operand pair the kernels form (a < 8 p times an s-form challenge < 32 p gives X < 1.5 p only for the widest sums; binds multiply a
// difference of two semi values, |a| < 1.01 p, X < 0.2 p).
#pragma once
#include <stdint.h>
#include "fr.cuh"
#include "mont29.cuh"

#ifdef LASSO_BN254
struct Bn254FrM {
  static LHD int32_t p(int k) { const int32_t P[9] = {268435457, 521120927, 240919632, 131109107, 361091715, 47923392, 10936641, 240920116, 3171406}; return P[k]; }
  static constexpr uint32_t PINV = 268435455u;   // -p^-1 mod 2^29
  static constexpr int32_t QC = 1420063842;
  static constexpr int32_t ONE_S_0 = 268435287, ONE_S_1 = 514263732, ONE_S_2 = 86771339, ONE_S_3 = 391139145, ONE_S_4 = 178784091, ONE_S_5 = 490881230, ONE_S_6 = 299191303,
                           ONE_S_7 = 86689704, ONE_S_8 = 903222;
  static constexpr int32_t K522_0 = 95853524, K522_1 = 102173274, K522_2 = 34397646, K522_3 = 498479371, K522_4 = 240439551, K522_5 = 486036963, K522_6 = 471195907,
                           K522_7 = 131109217, K522_8 = 656714;
  static LHD m29<Bn254FrM> k5() { return m29_limbs<Bn254FrM>(268430039, 492061940, 71535269, 62181526, 323781850, 244503300, 348886451, 68918589, 360451); }          // 2^266 mod p
  static LHD m29<Bn254FrM> k10() { return m29_limbs<Bn254FrM>(268262109, 223975601, 492627914, 522739689, 150938553, 164142673, 394138283, 408892696, 2020216); }       // 2^271 mod p
  static LHD m29<Bn254FrM> r2s() { return m29_limbs<Bn254FrM>(338539743, 433494286, 343078028, 115075043, 193254777, 284818167, 304038784, 396432094, 1209799); }       // 2^517 mod p
};
typedef Bn254FrM FrM29;
#else
struct Curve25519FrM {
  // limbs 5..7 of p are zero; limb 8 = 2^20
  static LHD int32_t p(int k) { const int32_t P[9] = {485872621, 9640146, 501691798, 502512965, 333, 0, 0, 0, 1 << 20}; return P[k]; }
  static constexpr uint32_t PINV = 307527195u;   // -p^-1 mod 2^29
  static constexpr int32_t ONE_S_0 = 290322925, ONE_S_1 = 442594051, ONE_S_2 = 259787148, ONE_S_3 = 377041255, ONE_S_4 = 536700270, ONE_S_5 = 536870911, ONE_S_6 = 536870911,
                           ONE_S_7 = 536870911, ONE_S_8 = 1048575;
  static LHD m29<Curve25519FrM> k5() { return m29_limbs<Curve25519FrM>(133862381, 442392295, 276935791, 245514615, 531400038, 536870911, 536870911, 536870911, 1048575); }     // 2^266 mod p
  static LHD m29<Curve25519FrM> k10() { return m29_limbs<Curve25519FrM>(495834093, 435936093, 288821455, 331629432, 361792606, 536870911, 536870911, 536870911, 1048575); }    // 2^271 mod p
  static LHD m29<Curve25519FrM> r2s() { return m29_limbs<Curve25519FrM>(147395749, 34354560, 457688582, 356494647, 483104506, 488734555, 518485561, 233882216, 206883); }        // 2^517 mod p
};
typedef Curve25519FrM FrM29;

// The four reductions whose quotient comes from a shift (p = 2^252 + c) instead of mont29.cuh's reciprocal.

// Lazily reduced memory form for arrays that only kernels read (the bound arrays of a sumcheck between two rounds): any limbs with
// |.| < 2^31 and |value| < 2^255 -> digits (limbs in [0, 2^29), limb 8 <= 2^22) of SOME representative in (0, 2^254 + 2^130) of the same
// residue.  One fused pass: floor(value / 2^252) is estimated from the two top limbs (off by at most 1 either way: the carries of the lower
// limbs it ignores), and with f = estimate - 2 the value - f p lies in [2^252, 4 * 2^252) up to |f| c (c = p - 2^252 ~ 2^125).  48 instructions
// against 115 for fr29_canonical; fr29_pack / fr29_unpack_u carry such a value through memory unchanged, and every reader (fr29_mul
// operands, fr29_canonical) accepts it.
template <> LHD m29<FrM29> m29_near<FrM29>(const m29<FrM29>& a) {
  const int32_t f = ((a.v[8] + (a.v[7] >> 29)) >> 20) - 2;
  m29<FrM29> r; int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { int64_t x = (int64_t)a.v[k] - (int64_t)f * FrM29::p(k) + c; if (k < 8) { r.v[k] = (int32_t)x & M29_MASK; c = x >> 29; } else r.v[8] = (int32_t)x; }
  return r;
}

// any limbs with |.| < 2^31 and |value| < 2^255 -> the canonical representative in [0, p), limbs in [0, 2^29)
// (f below is floor(value / 2^252), |f| <= 8: the remainder r stays within 8c of [0, 2^252), which the second stage absorbs)
template <> LHD m29<FrM29> m29_canonical<FrM29>(const m29<FrM29>& a) {
  m29<FrM29> w = m29_weak(a);
  // r = value - f*p with f = floor(value / 2^252): r in (-3c, 2^252 + 3c)
  const int32_t f = w.v[8] >> 20;
  m29<FrM29> r; int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { int64_t x = (int64_t)w.v[k] - (int64_t)f * FrM29::p(k) + c; if (k < 8) { r.v[k] = (int32_t)x & M29_MASK; c = x >> 29; } else r.v[8] = (int32_t)x; }
  // g = -1: r < 0, r + p is canonical.  g = 0: canonical.  g = 1: r in [2^252, 2^252 + 3c): r - p if that is non-negative, else r.
  const int32_t g = r.v[8] >> 20;
  m29<FrM29> s; c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { int64_t x = (int64_t)r.v[k] - (int64_t)g * FrM29::p(k) + c; if (k < 8) { s.v[k] = (int32_t)x & M29_MASK; c = x >> 29; } else s.v[8] = (int32_t)x; }
  const bool keep_r = s.v[8] < 0;
#pragma unroll
  for (int k = 0; k < 9; k++) s.v[k] = keep_r ? r.v[k] : s.v[k];
  return s;
}
// Nine 64-bit column sums, times 2^shift (shift <= 10), -> the canonical limbs of the same residue.  This is how a block / grid sum ends:
// the radix corrections the kernels used to apply as one more Montgomery product with 2^261 (ONE_S), 2^266 (K5) or 2^271 (K10) are the
// shifts 0, 5, 10 of the column values, and the reduction is one exact quotient estimate instead of a product: with l_8 the top column after a
// carry pass (everything above 2^232), f = l_8 >> 20 is floor(value / 2^252) exactly, and value - (f - 1) p lies in (0, 2^253 + 2^152).
// |col[k]| < 2^50 before the shift (sums of up to 2^20 reduced limbs).  ~220 instructions against ~460 for from_columns + product + canonical.
template <> LHD m29<FrM29> m29_reduce_columns<FrM29>(const int64_t* col, int shift) {
  int64_t l[9]; int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { const int64_t x = col[k] * ((int64_t)1 << shift) + c; if (k < 8) { l[k] = x & M29_MASK; c = x >> 29; } else l[8] = x; }
  const int32_t f = (int32_t)(l[8] >> 20) - 1;   // |l_8| < 2^51: fits
  m29<FrM29> r; c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { const int64_t x = l[k] - (int64_t)f * FrM29::p(k) + c; if (k < 8) { r.v[k] = (int32_t)x & M29_MASK; c = x >> 29; } else r.v[8] = (int32_t)x; }
  return m29_canonical(r);
}
// nine 64-bit column sums (e.g. of up to 2^20 reduced values) -> reduced fr29 of the same value mod p, with |value| < 2^262 + 2^29 p
template <> LHD m29<FrM29> m29_from_columns<FrM29>(const int64_t* col) {
  const int32_t ONE_S[9] = {FrM29::ONE_S_0, FrM29::ONE_S_1, FrM29::ONE_S_2, FrM29::ONE_S_3, FrM29::ONE_S_4, FrM29::ONE_S_5, FrM29::ONE_S_6, FrM29::ONE_S_7, FrM29::ONE_S_8};
  int64_t l[9]; int64_t c = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { int64_t x = col[k] + c; c = x >> 29; l[k] = x & M29_MASK; }
  // value = l + c * 2^261 and 2^261 = ONE_S (mod p); |c| < 2^35 in any use here, c * ONE_S[k] < 2^64
  m29<FrM29> r; int64_t d = 0;
#pragma unroll
  for (int k = 0; k < 9; k++) { int64_t x = l[k] + c * ONE_S[k] + d; if (k < 8) { r.v[k] = (int32_t)x & M29_MASK; d = x >> 29; } else r.v[8] = (int32_t)x; }
  return r;
}
#endif

typedef m29<FrM29> fr29;
typedef m29_acc<FrM29> fr29_acc;
#define FR29_MASK M29_MASK

// The fr29_* names over the m29 templates.  The two curves differ in HOW they forward, and only in that.  The instructions a kernel compiles to
// depend on how many inlining layers a body passes on its way in (a wrapper more or less reorders carry chains and schedules), and each curve's
// kernels are tuned and measured at one depth: one wrapper layer for BN254, none (the name IS the instantiation) for curve25519.
// fr29_unpack_u: memory (canonical x*2^256, 8 x u32) -> limbs of the same integer ("u-form").  fr29_unpack_s: memory -> limbs of (integer << 5) = x*2^261
// ("s-form"); the integer is < 2^253 (BN254: 2^254), so limb 8 < 2^26 (2^27).  fr29_pack: canonical limbs -> memory words.
// acc is the 17-column double-width value (29-bit columns, signed 64-bit);
// fr29_mul_acc adds a*b into it with the same 81 multiply-adds fr29_mul starts with and nothing else.  One product adds < 9 * 2^58 to a column
// when |a.v|, |b.v| <= 2^29, so up to THREE products may be added between two fr29_acc_carry passes (which bring columns 0..15 back to
// [0, 2^29) and let column 16 absorb the carries).  fr29_acc_reduce finishes with the Montgomery reduction: the sum / 2^261 (mod p), reduced,
// correct for sums of up to 2^20 products.
static constexpr auto& fr29_from_limbs = m29_limbs<FrM29>;
#ifdef LASSO_BN254
LHD fr29 fr29_zero() { return m29_zero<FrM29>(); }
LHD fr29 fr29_add(const fr29& a, const fr29& b) { return m29_add(a, b); }
LHD fr29 fr29_sub(const fr29& a, const fr29& b) { return m29_sub(a, b); }
LHD fr29 fr29_weak(const fr29& a) { return m29_weak(a); }
LHD fr29 fr29_mul(const fr29& a, const fr29& b) { return m29_mul(a, b); }
LHD fr29_acc fr29_acc_zero() { return m29_acc_zero<FrM29>(); }
LHD void fr29_mul_acc(fr29_acc& acc, const fr29& a, const fr29& b) { m29_mul_acc(acc, a, b); }
LHD void fr29_acc_carry(fr29_acc& acc) { m29_acc_carry(acc); }
LHD fr29 fr29_acc_reduce(const fr29_acc& acc) { return m29_acc_reduce(acc); }
LHD fr29 fr29_semi(const fr29& a) { return m29_near(a); }
LHD fr29 fr29_canonical(const fr29& a) { return m29_canonical(a); }
LHD fr29 fr29_reduce_columns(const int64_t* col, int shift) { return m29_reduce_columns<FrM29>(col, shift); }
LHD fr29 fr29_from_columns(const int64_t* col) { return m29_from_columns<FrM29>(col); }
LHD fr29 fr29_unpack_u(const fr_t& x) { return m29_unpack_words<FrM29>(x.v); }
LHD fr29 fr29_unpack_s(const fr_t& x) { return m29_unpack_words_shl5<FrM29>(x.v); }
LHD fr_t fr29_pack(const fr29& a) { fr_t r; m29_pack_words(a, r.v); return r; }
#else
static constexpr auto& fr29_zero = m29_zero<FrM29>;
static constexpr auto& fr29_add = m29_add<FrM29>;
static constexpr auto& fr29_sub = m29_sub<FrM29>;
static constexpr auto& fr29_weak = m29_weak<FrM29>;
static constexpr auto& fr29_mul = m29_mul<FrM29>;
static constexpr auto& fr29_acc_zero = m29_acc_zero<FrM29>;
static constexpr auto& fr29_mul_acc = m29_mul_acc<FrM29>;
static constexpr auto& fr29_acc_carry = m29_acc_carry<FrM29>;
static constexpr auto& fr29_acc_reduce = m29_acc_reduce<FrM29>;
static constexpr auto& fr29_semi = m29_near<FrM29>;
static constexpr auto& fr29_canonical = m29_canonical<FrM29>;
static constexpr auto& fr29_reduce_columns = m29_reduce_columns<FrM29>;
static constexpr auto& fr29_from_columns = m29_from_columns<FrM29>;
// memory words <-> limbs take and return fr_t itself, where mont29.cuh's go through a pointer to the words: the same loops as m29_unpack_words,
// m29_unpack_words_shl5 and m29_pack_words, but through the pointer forms the curve25519 kernels do not all compile to the same instructions.
LHD fr29 fr29_unpack_u(const fr_t& x) {
  fr29 r;
#pragma unroll
  for (int k = 0; k < 9; k++) {
    const int bit = 29 * k, w = bit >> 5, s = bit & 31;
    uint64_t two = (uint64_t)x.v[w] | ((w + 1 < 8) ? ((uint64_t)x.v[w + 1] << 32) : 0);
    r.v[k] = (int32_t)((uint32_t)(two >> s) & FR29_MASK);
  }
  return r;
}
LHD fr29 fr29_unpack_s(const fr_t& x) {
  fr29 r;
  r.v[0] = (int32_t)((x.v[0] << 5) & FR29_MASK);
#pragma unroll
  for (int k = 1; k < 9; k++) {
    const int bit = 29 * k - 5, w = bit >> 5, s = bit & 31;
    uint64_t two = (uint64_t)x.v[w] | ((w + 1 < 8) ? ((uint64_t)x.v[w + 1] << 32) : 0);
    r.v[k] = (int32_t)((uint32_t)(two >> s) & FR29_MASK);
  }
  return r;
}
LHD fr_t fr29_pack(const fr29& a) {
  fr_t r;
#pragma unroll
  for (int w = 0; w < 8; w++) {
    // word w = bits [32w, 32w+32): limb k0 = floor(32w/29) from bit offset s, plus the next limb(s)
    const int k0 = (32 * w) / 29, s = 32 * w - 29 * k0;
    uint64_t acc = (uint64_t)(uint32_t)a.v[k0] >> s;
    int have = 29 - s;
    if (k0 + 1 < 9) { acc |= (uint64_t)(uint32_t)a.v[k0 + 1] << have; have += 29; }
    if (have < 32 && k0 + 2 < 9) acc |= (uint64_t)(uint32_t)a.v[k0 + 2] << have;
    r.v[w] = (uint32_t)acc;
  }
  return r;
}
#endif

// acc += z * b, z a 64-bit integer, b as an unpack function returns it: 27 multiply-adds; up to FR29_U64_ACC_PERIOD of them between two fr29_acc_carry passes (mont29.cuh
// m29_mul_acc_u64 derives the number).  With b in s-form (x 2^261), fr29_acc_reduce gives the INTEGER residue sum z x, and one product with R2S its memory form.
#define FR29_U64_ACC_PERIOD M29_U64_ACC_PERIOD
LHD void fr29_mul_acc_u64(fr29_acc& acc, uint64_t z, const fr29& b) { m29_mul_acc_u64(acc, z, b); }
// the carry pass for an accumulator that has taken fr29_mul_acc_u64 products ONLY: they reach columns 0..10, and a sum of up to 2^20 of them is below 2^345, so column 11
// (everything from 2^319 up: below 2^26) absorbs the top carry and columns 12..16 stay zero — to the compiler too, which then keeps 12 live columns instead of 17
LHD void fr29_acc_carry_u64(fr29_acc& acc) {
#pragma unroll
  for (int k = 0; k < 11; k++) { acc.h[k + 1] += acc.h[k] >> 29; acc.h[k] &= FR29_MASK; }
}

// 2^261 mod p: fr29_mul(a, ONE_S) = a (mod p) with the magnitude brought back to (-X, p + X)
LHD fr29 fr29_one_s() { return fr29_from_limbs(FrM29::ONE_S_0, FrM29::ONE_S_1, FrM29::ONE_S_2, FrM29::ONE_S_3, FrM29::ONE_S_4, FrM29::ONE_S_5, FrM29::ONE_S_6, FrM29::ONE_S_7, FrM29::ONE_S_8); }
// 2^266 mod p: corrects a sum of mul(mul(u, s), u)-style terms that came out 2^5 short
LHD fr29 fr29_k5() { return FrM29::k5(); }
// 2^271 mod p: corrects a sum of mul(mul(u, u), u) terms (2^10 short)
LHD fr29 fr29_k10() { return FrM29::k10(); }
// 2^517 mod p: fr29_mul(integer x < 2^64 as limbs, R2S) = x * 2^256 = u-form of x
LHD fr29 fr29_r2s() { return FrM29::r2s(); }
// the integer 2^10 as limbs: fr29_mul(fr29_mul(u, u), INT_FROM_UU) = the canonical integer x*y (mod p) of a product of two u-form values
LHD fr29 fr29_int_from_uu() { fr29 r = fr29_zero(); r.v[0] = 1 << 10; return r; }
// small non-negative integer -> limbs (for fr29_mul(x, R2S))
LHD fr29 fr29_from_u64_int(uint64_t x) { return fr29_from_limbs((int32_t)(x & FR29_MASK), (int32_t)((x >> 29) & FR29_MASK), (int32_t)(x >> 58), 0, 0, 0, 0, 0, 0); }
// u-form value with |value| < 4p -> memory
LHD fr_t fr29_store(const fr29& a) { return fr29_pack(fr29_canonical(a)); }
