/* lasso_hip_mle.h — SubtableStrategy::evaluate_subtable_mle (src/subtables/mod.rs:31-93) for tables the CALLER defines (lasso_strategy_custom, lasso_hip.h): the
 * multilinear extension of up to 32 tables of 2^log_m entries at one point, as one device call.  A table without a closed form has no cheaper MLE than the dot product
 * with EqPolynomial(point).evals(); the verifier used to form that on one CPU thread, 2^log_m products and a 32 * 2^log_m-byte eq table per subtable.  Here the eq table
 * is never materialised: chi_i = hi[i >> lo_bits] * lo[i & mask] over two factor tables of at most 2^15 entries each, and the tables are read once.
 * This header is separate so that a library which implements lasso_hip.h alone stays a complete implementation of that header.  Exported by liblasso_hip.so and
 * liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_MLE_H
#define LASSO_HIP_MLE_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out[k] = sum_i T_k[i] * chi_i(point),  chi = EqPolynomial(point).evals()  (eq_poly.rs:22-38: point[0] <-> the top bit of i),  k < num_tables.
 *   tables_u32 / tables_fr  num_tables HOST pointers to 2^log_m entries each: 32-bit integers, or field elements in memory form (any representative a device array may
 *                           hold: below 2^254 + 2^130); exactly one of the two arguments is non-NULL, and no pointer in it is NULL
 *   num_tables              1 .. 32          log_m  1 .. 30
 *   point                   log_m field elements, host memory, any representative lasso_hip.h allows
 *   out                     num_tables field elements, host memory: fully reduced memory form
 * A broken rule is LASSO_ERR_INVALID with a message, before anything is launched.  Synchronous.
 * Scratch comes from the context (counted by lasso_mem_stats) and does not depend on log_m: the tables are uploaded strip by strip, at most 64 MiB of strips at a time
 * (all tables' strips together), beside at most 2 MiB of factor tables and 2 MiB of block sums — under 69 MiB in all.  LASSO_MLE_STRIP=N makes a strip N entries of every
 * table instead (tests: strip boundaries within small tables); the strips then take num_tables * N * (4 or 32) bytes.
 * LASSO_ERR_UNSUPPORTED, with a message, when that buffer would have to grow while a resident kernel is active. */
int32_t lasso_tables_mle(lasso_ctx* ctx, const uint32_t* const* tables_u32, const lasso_fr* const* tables_fr, uint32_t num_tables, uint32_t log_m, const lasso_fr* point, lasso_fr* out);
/* the same over tables resident on the device: a HOST array of num_tables DEVICE pointers; the tables are only read, nothing is uploaded and one launch walks them whole
 * (scratch: the factor tables and the block sums, at most 4 MiB) */
int32_t lasso_tables_mle_dev(lasso_ctx* ctx, const uint32_t* const* d_tables_u32, const lasso_fr* const* d_tables_fr, uint32_t num_tables, uint32_t log_m, const lasso_fr* point, lasso_fr* out);

#ifdef __cplusplus
}
#endif
#endif
