/* lasso_hip_values.h — the lookup RESULTS as a vector on the device.  SparsePolynomialEvaluationProof::prove proves one scalar, claimed_evaluation =
 * sum_k eq(r, k) * g(T[dim(k)]) (subtables/mod.rs:187-216, surge.rs:119-211): the multilinear extension at r of v[k] = combine_lookups(T_sub(0)[dim_0(k)], ...) — x & y for
 * AND, x < y for LT, x for a range check.  This entry point writes v from the addresses a densified representation already holds on the device: 4 * C bytes read and 8 or 32
 * bytes written per lookup, instead of NUM_MEMORIES gathered arrays of 32 bytes per lookup.
 * This header is separate so that a library which implements lasso_hip.h alone stays a complete implementation of that header.  Exported by liblasso_hip.so and
 * liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_VALUES_H
#define LASSO_HIP_VALUES_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

enum lasso_values_form { LASSO_VALUES_FR = 0 /* n field elements, fully reduced memory form */, LASSO_VALUES_U64 = 1 /* n 64-bit integers */ };

/* out[k] = combine_lookups(vals),  vals[i] = T[memory_to_subtable_index(i)][dim[memory_to_dimension_index(i)][k]],  i < NUM_MEMORIES,  k < n, for every strategy kind:
 *   AND / OR / XOR / RangeCheck   sum_i 2^(i * inc) * vals[i]  (and.rs:45-53, range_check.rs:78-86; (C - 1) * inc < 64 as everywhere)
 *   LT                            lt.rs:62-71; its two tables hold bits (what lasso_materialize_subtable_u32 writes)
 *   Spark                         the product
 *   LASSO_CUSTOM                  the term list of the lasso_strategy_custom `s` points to, packed and kept in the context as lasso_combine_claim keeps it; the memory maps are the
 *                                 descriptor's (or the trait's defaults); the descriptor's HOST table pointers are not read — the tables are the device arrays below
 *   d_dim          HOST array of s->c DEVICE pointers: n addresses below 2^log_m each, 8-byte aligned (DensifiedRepresentation's dim_usize).  An address is masked to log_m
 *                  bits before it is used, so a larger one reads a wrong entry instead of memory outside the table.
 *   d_tables_u32   HOST array of num_subtables DEVICE pointers to 2^log_m 32-bit integers each (AND / OR / XOR: 1 table, LT: 2, RangeCheck: 3, custom: its own), or NULL
 *   d_tables_fr    the same as field elements in memory form (any representative a device array may hold: below 2^254 + 2^130), or NULL.  Exactly one of the two is non-NULL;
 *                  the integer kinds take integers, Spark (C tables) takes field elements, a caller-defined strategy either.
 *   form           LASSO_VALUES_FR: d_out receives n field elements (32 bytes each), canonical.
 *                  LASSO_VALUES_U64: n 64-bit integers.  Offered for LT, and for AND / OR / XOR / RangeCheck when sum_i 2^(i * inc) * max_table_value < 2^64 with the kind's own
 *                  max_table_value (2^(log_m / 2) - 1; RangeCheck: 2^log_m - 1) — which the tables passed must respect.  Every other case — Spark, LASSO_CUSTOM, a
 *                  built-in shape whose bound reaches 2^64 — is LASSO_ERR_UNSUPPORTED with a message.
 *   d_out          device memory, 16-byte aligned; exactly n elements are written and nothing else
 * A descriptor or argument that breaks a rule is LASSO_ERR_INVALID with a message.  Both refusals come before anything is launched.  n = 0 does nothing.
 * One launch, enqueued on the context's stream like lasso_gather (not synchronous); profiling family LASSO_K_MISC.  No scratch; a caller-defined strategy's term list is the
 * context's staged copy (a NEW list cannot be staged while a launch of the context is outstanding, as for lasso_combine_claim).
 * LASSO_VALUES_NX=N caps the grid at N workgroups (tests). */
int32_t lasso_lookup_values(lasso_ctx* ctx, const lasso_strategy* s, const uint32_t* const* d_dim, const uint32_t* const* d_tables_u32, const lasso_fr* const* d_tables_fr,
                            size_t n, int32_t form, void* d_out);

#ifdef __cplusplus
}
#endif
#endif
