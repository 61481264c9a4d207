// The lazy sums of the subtable-MLE kernels (mle_kernels.cuh), host and device, so that the CPU tests can hold them against big integers
// (tests/cpp/test_mle_acc_host.cpp, plain and under -fsanitize=undefined).
//
// A lane of k_tables_mle owns one low index i_lo and walks rows i_hi: it forms  A = sum_rows T[i_hi, i_lo] * hi[i_hi]  WITHOUT a reduction per entry, then ONE
// Montgomery reduction and ONE product with lo[i_lo].  Two table forms:
//   u32 entries   t < 2^32 is an integer, e = the limbs of a factor-table entry (reduced: limbs 0..7 in [0, 2^29), limb 8 in [0, 2^23) for any memory word below 2^255).
//                 With t = t0 + 2^29 t1 (t0 < 2^29, t1 < 8) the product is 18 multiply-adds into ten 64-bit columns: h[k] += e[k] t0, h[k + 1] += e[k] t1.
//                 One term adds less than 2^29 * 2^29 + 8 * 2^29 < 2^58 + 2^32 to a column, and a fold leaves columns 0..8 below 2^29, so MLE_FOLD_EVERY = 16 terms keep
//                 every column below 16 * (2^58 + 2^32) + 2^29 < 2^62.01 — inside a signed 64-bit word — and the fold (one carry pass, nothing modular) brings columns
//                 0..8 back to [0, 2^29).  Column 9 only absorbs: it holds floor(A / 2^261), and A < N * 2^32 * 2^255 for N terms, so it stays below N * 2^26 (N <= 2^15
//                 rows: 2^41).
//   Fr entries    both operands are field elements: fr29_mul_acc's 81 multiply-adds into the 17-column fr29_acc, whose own rule (fr29.cuh) is a carry pass every
//                 MLE_FR_FOLD_EVERY = 3 products.
// Either sum ends in mle_*_reduce: A / 2^261 (mod p) as a reduced fr29 with |value| < 2^261 + 2 p, a legal first operand of fr29_mul.
#pragma once
#include <stdint.h>
#include "fr29.cuh"

#define MLE_FOLD_EVERY 16u      // u32 terms between two carry passes of mle_acc (bound above)
#define MLE_FR_FOLD_EVERY 3u    // field products between two fr29_acc_carry passes (fr29.cuh: up to three)

struct mle_acc { int64_t h[10]; };
LHD mle_acc mle_acc_zero() { mle_acc a;
#pragma unroll
  for (int k = 0; k < 10; k++) a.h[k] = 0; return a; }
// a += t * e   (e reduced, limb 8 non-negative; at most MLE_FOLD_EVERY calls between two folds)
LHD void mle_acc_add_u32(mle_acc& a, uint32_t t, const fr29& e) {
  const int32_t t0 = (int32_t)(t & FR29_MASK), t1 = (int32_t)(t >> 29);
#pragma unroll
  for (int k = 0; k < 9; k++) { a.h[k] += (int64_t)e.v[k] * t0; a.h[k + 1] += (int64_t)e.v[k] * t1; }
}
// carry pass: columns 0..8 back to [0, 2^29), column 9 takes what is above 2^261; the value is unchanged
LHD void mle_acc_fold(mle_acc& a) {
#pragma unroll
  for (int k = 0; k < 9; k++) { a.h[k + 1] += a.h[k] >> 29; a.h[k] &= FR29_MASK; }
}
// A / 2^261 (mod p), reduced: the ten columns are the low columns of a double-width value whose upper seven are zero (call after a fold)
LHD fr29 mle_acc_reduce(const mle_acc& a) {
  fr29_acc w = fr29_acc_zero();
#pragma unroll
  for (int k = 0; k < 10; k++) w.h[k] = a.h[k];
  fr29_acc_carry(w);
  return fr29_acc_reduce(w);
}
// the Fr form's step and end, named so that kernel and host test run the same lines
LHD void mle_fr_acc_add(fr29_acc& w, const fr29& t, const fr29& e) { fr29_mul_acc(w, t, e); }
LHD fr29 mle_fr_acc_reduce(fr29_acc& w) { fr29_acc_carry(w); return fr29_acc_reduce(w); }
