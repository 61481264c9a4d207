/* lasso_prover_mle.h — SubtableStrategy::evaluate_subtable_mle (src/subtables/mod.rs:31-93) at the host prover's C ABI, for every strategy kind, and the counter of the
 * caller-defined tables the device evaluated.  Separate from lasso_prover.h for the reason lasso_hip_mle.h is separate from lasso_hip.h: the larger headers stay as their
 * implementations and generated bindings know them.  Exported by liblasso_prover.so and liblasso_prover_bn254.so. */
#ifndef LASSO_PROVER_MLE_H
#define LASSO_PROVER_MLE_H
#include "lasso_prover.h"
#ifdef __cplusplus
extern "C" {
#endif

/* out[k] = the multilinear extension of subtable k of `strategy` at `point` (point_len = log_m field elements, Montgomery form), for EVERY subtable k < num_subtables of the
 * strategy (AND / OR / XOR: 1, LT: 2, RangeCheck: 3, Spark: C, custom: its own): fully reduced field elements.  The built-in kinds and Spark use their closed forms whatever
 * `where` says.  kind = LASSO_CUSTOM: where = 0 is the host loop (2^log_m products per table over EqPolynomial(point).evals()), where = 1 one lasso_tables_mle call over all
 * tables (include/lasso_hip_mle.h) — -1 with a message when the device library this host was linked against has no such entry.
 * lasso_host_verify* evaluates the distinct subtables a caller-defined strategy's memories use in one such device call when the entry exists and
 * num_subtables * 2^log_m is at least LASSO_MLE_DEVICE_MIN; LASSO_VERIFY_DEVICE_MLE=0 keeps the host loop.  Verdicts, return codes and error texts do not depend on the route. */
int32_t lasso_host_tables_mle(lasso_host* h, const lasso_strategy* strategy, const lasso_fr* point, size_t point_len, int32_t where, lasso_fr* out);
/* *device_tables = caller-defined tables this host has evaluated on the device so far (verifier and lasso_host_tables_mle(where = 1) together); *available = 1 when the
 * device library has lasso_tables_mle; either may be NULL; reset != 0 zeroes the counter. */
int32_t lasso_host_mle_stats(lasso_host* h, uint64_t* device_tables, int32_t* available, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
