/* lasso_prover_values.h — the lookup RESULTS at the host prover's C ABI, and the proof's claim about them.  SparsePolynomialEvaluationProof::prove proves
 * claimed_evaluation = sum_k eq(r, k) * g(T[dim(k)]) (subtables/mod.rs:187-216): the multilinear extension at r of the vector v[k] = combine_lookups(T_sub(0)[dim_0(k)], ...).
 * The calls below give a caller that vector (a CPU statement, and the device route over a densified representation), evaluate a vector at r, and read the claim out of the
 * proof bytes, so that   values_evaluate(lookup_values(dense), r) == proof_claimed_evaluation(prove(dense, r))   can be checked by whoever uses the proof.
 * Separate from lasso_prover.h for the reason lasso_hip_values.h is separate from lasso_hip.h: the larger headers stay as their implementations and generated bindings know
 * them.  The device entries (lasso_lookup_values, lasso_tables_mle*) are weak references of the library: linked against an implementation of lasso_hip.h alone, the calls
 * that need them return -1 with a message.  Exported by liblasso_prover.so and liblasso_prover_bn254.so. */
#ifndef LASSO_PROVER_VALUES_H
#define LASSO_PROVER_VALUES_H
#include "lasso_prover.h"
#include "lasso_hip_values.h"
#ifdef __cplusplus
extern "C" {
#endif

/* The normative CPU statement; needs no host object.  indices: n_lookups x strategy->c, row-major, every index below 2^log_m; n_lookups >= 1.
 * Writes s = next_pow2(n_lookups) elements — rows n_lookups .. s - 1 are the rows densify pads with: address 0 in every dimension (densified.rs:38) — of 32 bytes
 * (form = LASSO_VALUES_FR: fully reduced field elements, Montgomery form) or 8 bytes (LASSO_VALUES_U64).  *count = s (may be NULL); cap = the elements `out` holds: -2 when
 * that is too few (or out is NULL), with *count set.  The tables are Strategy::materialize_subtables(), Spark's EqPolynomial(tau_i).evals(), or the caller's.
 * The 64-bit form is refused by lasso_lookup_values' rule, with its text (include/lasso_hip_values.h). */
int32_t lasso_host_lookup_values_ref(const lasso_strategy* strategy, const uint64_t* indices, size_t n_lookups, int32_t form, void* out, size_t cap, size_t* count);
/* *s = the (padded) number of lookups of a densified representation: what lasso_host_lookup_values writes */
int32_t lasso_host_dense_len(lasso_host_dense* dense, size_t* s);
/* The same vector for a densified representation (lasso_host_dense_len elements), computed on the device from the representation's own address columns and device tables (materialised,
 * or uploaded for LASSO_CUSTOM) by lasso_lookup_values.  out_on_device = 0: `out` is host memory (downloaded); 1: a device pointer of this host's context, 16-byte aligned.
 * The call returns when the vector is complete.  Works for capacity mode's compact representation; the representation is only read — a proof made afterwards has the bytes it
 * would have had.  -1 with a message: a strategy whose c / log_m do not match the representation; a representation of a slab-mode host (world > 1: a rank holds one residue
 * class of the lookups); the 64-bit form where it is not offered; a device library without lasso_lookup_values. */
int32_t lasso_host_lookup_values(lasso_host* h, lasso_host_dense* dense, const lasso_strategy* strategy, int32_t form, int32_t out_on_device, void* out);
/* DensePolynomial::evaluate (dense_mlpoly.rs) of the caller's vector of s = 2^r_len field elements (memory form, any representative a device array may hold) at r
 * (r[0] <-> the top index bit, as everywhere): *out fully reduced.  values_on_device = 0: host memory; 1: a device pointer of this host's context.  One lasso_tables_mle /
 * lasso_tables_mle_dev call over one table — the eq table is never formed; r_len = 0 is answered on the host.  -1 with a message where the device library has no such entry,
 * and for r_len above 30.  64-bit vectors are not taken. */
int32_t lasso_host_values_evaluate(lasso_host* h, const lasso_fr* values, int32_t values_on_device, size_t s, const lasso_fr* r, size_t r_len, lasso_fr* out);
/* claimed_evaluation of a serialized SparsePolynomialEvaluationProof (surge.rs:92-104): behind comm_derefs and the primary sumcheck.  Montgomery form, fully reduced.  The
 * bytes are read with the verifier's reader: truncated bytes, an implausible length prefix or a non-canonical scalar are -1 with its message.  Nothing else of the proof is
 * looked at: this is a read, not a verification. */
int32_t lasso_host_proof_claimed_evaluation(const uint8_t* proof, size_t proof_len, lasso_fr* out);
/* *device_lookups = elements lasso_host_lookup_values has had the device write for this host so far; *available = 1 when the device library has lasso_lookup_values; either
 * may be NULL; reset != 0 zeroes the counter. */
int32_t lasso_host_values_stats(lasso_host* h, uint64_t* device_lookups, int32_t* available, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
