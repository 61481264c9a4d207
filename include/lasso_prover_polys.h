/* lasso_prover_polys.h — several caller vectors under ONE commitment, opened at one point in ONE proof, at the host prover's C ABI: DensePolynomial::merge(polys)
 * (dense_mlpoly.rs:251-261) .commit(gens, None), and CombinedTableEvalProof::prove / verify (subtables/mod.rs:285-375) over the merge — what the Lasso prover does for its
 * own polynomials (Prover::joint_open), for the columns a caller holds: operands, the results of one or more tables over the same rows, further witness columns.
 *   prover    c = polys_commit(x, y, v_and, v_lt);  poly_commitment_append(c);  the Lasso proofs at r on the transcript;  opening, evals = polys_open(.., r, the same transcript and tape)
 *   verifier  poly_commitment_append(c);  lasso_host_verify_cb per proof;  evals[2], evals[3] against lasso_host_proof_claimed_evaluation of the proofs;  evals[0], evals[1]
 *             against its own polys_evaluate(x, y) of the public columns;  polys_verify(c, r, evals, opening) on the same transcript
 * k vectors of s = 2^nv values each; K = next_pow2(k), kappa = log2 K.  The merge has nv + kappa variables: vector b is block b of K, the blocks behind k are zero.  It is
 * never made in memory: every vector is read where it lies and in the form it has (enum lasso_values_form; host or device memory, mixed freely within one call), by the
 * device entries lasso_host_poly_commit / lasso_host_poly_open take for one vector (include/lasso_prover_poly.h: 8 bytes per 64-bit element where the device library has
 * include/lasso_hip_poly.h, the host lift otherwise, the same bytes).  With the point ch || r, L = eq(ch) (x) eq(r[0 .. left - kappa)) (left = (nv + kappa) / 2), so
 *   L * Z = sum_b eq(ch)[b] * M_b,   M_b = eq(r[0 .. left - kappa)) * Z_b,   evals[b] = <M_b, eq(r[left - kappa ..))>:
 * one pass over each vector before any challenge is drawn, the claimed evaluations from it, a k-row mat-vec once ch is known, and one DotProductProofLog.
 * The generators are an ordinary lasso_host_poly_gens for nv + kappa variables; the commitment has lasso_host_poly_commit's layout and is absorbed with
 * lasso_host_poly_commitment_append; the proof bytes are the serialized DotProductProofLog as for lasso_host_poly_open.
 * Refused, -1 with a message, before anything is launched: k = 0; nv + kappa > 30; generators for another number of variables; r_len != nv; a row of the merged matrix that
 * would span several vectors (2^(nv + kappa - left) > s: only where k is large against s, e.g. five vectors of two values); per vector what lasso_host_poly_commit refuses,
 * with the vector's index; a slab-mode host.  Blinded (hiding) commitments: include/lasso_prover_blind.h.  Not offered: vectors of different lengths.
 * Separate from lasso_prover.h for the reason lasso_prover_values.h is.  Exported by liblasso_prover.so and liblasso_prover_bn254.so. */
#ifndef LASSO_PROVER_POLYS_H
#define LASSO_PROVER_POLYS_H
#include "lasso_prover_poly.h"
#ifdef __cplusplus
extern "C" {
#endif

/* one vector: the (values, form, on_device) of lasso_host_poly_commit */
typedef struct { const void* values; int32_t form; int32_t on_device; } lasso_host_poly_vec;

/* DensePolynomial::merge(vecs[0 .. k)).commit(gens, None): out = [u64 L'][L' x 32 B], L' = 2^((nv + kappa) / 2); the rows of the blocks behind k are the identity's encoding.
 * cap / *len as for lasso_host_commit. */
int32_t lasso_host_polys_commit(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, uint8_t* out, size_t cap, size_t* len);
/* CombinedTableEvalProof::prove label for label: protocol name "Lasso CombinedTableEvalProof"; evals zero-padded to K; append_scalars("evals_ops_val");
 * challenge_vector("challenge_combine_n_to_one", kappa); the fold by bound_poly_var_bot from the last challenge down; append_scalar("joint_claim_eval");
 * PolyEvalProof::prove at ch || r.  evals: k elements, evals[b] = MLE(vecs[b])(r), memory form, fully reduced.  r: r_len = nv field elements. */
int32_t lasso_host_polys_open(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len,
                              const lasso_transcript_vtbl* transcript, void* transcript_user, const lasso_transcript_vtbl* tape, void* tape_user,
                              lasso_fr* evals, uint8_t* proof, size_t cap, size_t* len);
/* CombinedTableEvalProof::verify: *ok = 1 (Ok) or 0 (Err); -1 with the reason as for lasso_host_poly_verify.  r_len = g's variables - kappa. */
int32_t lasso_host_polys_verify(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const lasso_fr* evals, size_t k,
                                const lasso_transcript_vtbl* transcript, void* transcript_user, const uint8_t* proof, size_t proof_len,
                                const uint8_t* commitment, size_t commitment_len, int32_t* ok);
/* evals[b] = MLE(vecs[b])(r) by the same pass (the M_b), without generators or transcript: what a verifier computes of the columns it holds itself. */
int32_t lasso_host_polys_evaluate(lasso_host* h, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len, lasso_fr* evals);
/* vectors this host has committed to / opened through the two calls above so far; either may be NULL; reset != 0 zeroes both.  The 64-bit elements among them that went
 * through the 8-byte device entries are counted by lasso_host_poly_stats. */
int32_t lasso_host_polys_stats(lasso_host* h, uint64_t* vectors_committed, uint64_t* vectors_opened, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
