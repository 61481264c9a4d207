/* lasso_prover_blind.h — the HIDING form of the commitments of lasso_prover_poly.h and lasso_prover_polys.h, at the host prover's C ABI: DensePolynomial::commit(gens,
 * Some(random_tape)) (dense_mlpoly.rs:153-181), PolyEvalProof::prove(poly, Some(blinds), r, Zr, Some(blind_Zr), ..) with its C_Zr' (:302-359) and PolyEvalProof::verify
 * (:361-386) — the surface of dense_mlpoly.rs, commitments.rs, dot_product.rs and bullet.rs.  Not zk.rs: the Lasso proof's own claimed_evaluation and its sumchecks stay
 * in the clear.
 * Why: without blinds a commitment is a function of the vector alone, so whoever can guess a column (operands, 0/1 comparison results) checks the guess against the
 * commitment bytes, and an opening names Zr.  With row blinds, row i is <Z_i, G> + blinds[i] * h; with blind_Zr, the opening is about C_Zr = Zr * G_1 + blind_Zr * h.
 *   prover    c, blinds = poly_commit_blinded(v, tape);   opening, Zr, C_Zr = poly_open_blinded(v, r, blinds, blind_Zr, transcript, tape)
 *   verifier  poly_verify_committed(c, r, C_Zr, opening)           (blind_Zr = NULL: lasso_host_poly_verify(c, r, Zr, opening) accepts it as it stands)
 * The code is the Lasso prover's and verifier's own (Prover::poly_eval_prove_resident, Prover::polys_eval_prove, Prover::dot_product_log_prove with their optional blinds,
 * Verifier::poly_eval_verify), composed of the device entries of lasso_hip.h: no device entry of its own.  Routes of a blinded row commitment, by the form the device reads:
 *   field elements   lasso_hyrax_commit_rows_dev over the data, the same call over the L x 1 matrix of blinds and the one-point base [h], lasso_points_reduce_compress
 *                    (groups = 2): the rows never leave the device unblinded.  A device library whose lasso_hyrax_commit_rows_dev reports LASSO_ERR_UNSUPPORTED takes the
 *                    route below over lasso_hyrax_commit_compressed.
 *   64-bit integers  lasso_hyrax_commit_compressed_u64 (8 bytes per element, counted by lasso_host_poly_stats), its rows decoded by the verifier's batch decoder (the
 *                    device decoder of lasso_hip_wire.h from its threshold on, the host decoder otherwise), blinds[i] * h added and the rows compressed on the host.
 * Without the entries of lasso_hip_poly.h the integers are lifted on the host and take the first route.  The bytes are the same on every route.
 * Arguments, refusals and cap / *len as for lasso_host_poly_commit / lasso_host_polys_commit; blinds are field elements in memory form in host memory, 8-byte aligned.
 * Not offered: slab mode (world > 1), blinded commitments of the Lasso prover's own polynomials (lasso_host_commit).
 * Separate from lasso_prover.h for the reason lasso_prover_values.h is.  Exported by liblasso_prover.so and liblasso_prover_bn254.so. */
#ifndef LASSO_PROVER_BLIND_H
#define LASSO_PROVER_BLIND_H
#include "lasso_prover_polys.h"
#ifdef __cplusplus
extern "C" {
#endif

/* DensePolynomial::commit(gens, Some(tape)): blinds = tape.random_vector("poly_blinds", L) drawn from the caller's live tape (the callbacks of lasso_host_prove_cb's
 * tape), returned in blinds_out (L elements, memory form, fully reduced: the PolyCommitmentBlinds); out = lasso_host_poly_commit's layout.  The draw precedes the
 * size check of `out`: a call that returns -2 has advanced the tape.  -1 with a message: what lasso_host_poly_commit refuses, a null tape or blinds_out, a misaligned blinds_out. */
int32_t lasso_host_poly_commit_blinded(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s,
                                       const lasso_transcript_vtbl* tape, void* tape_user, lasso_fr* blinds_out, uint8_t* out, size_t cap, size_t* len);
/* PolyEvalProof::prove(poly, blinds, r, Zr, blind_Zr, gens, transcript, tape).  blinds: the L row blinds of the commitment, or NULL (None: zero); blind_Zr: one
 * element, or NULL (zero).  *Zr as for lasso_host_poly_open (may be NULL); C_Zr (may be NULL) receives Zr * G_1 + blind_Zr * h compressed: the proof's Cy. */
int32_t lasso_host_poly_open_blinded(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len,
                                     const lasso_fr* blinds, const lasso_fr* blind_Zr, const lasso_transcript_vtbl* transcript, void* transcript_user,
                                     const lasso_transcript_vtbl* tape, void* tape_user, lasso_fr* Zr, uint8_t C_Zr[32], uint8_t* proof, size_t cap, size_t* len);
/* PolyEvalProof::verify(gens, transcript, r, C_Zr, commitment): *ok = 1 (Ok) or 0 (Err).  -1 with the reason as for lasso_host_poly_verify; an invalid encoding of C_Zr is one. */
int32_t lasso_host_poly_verify_committed(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const uint8_t C_Zr[32],
                                         const lasso_transcript_vtbl* transcript, void* transcript_user, const uint8_t* proof, size_t proof_len,
                                         const uint8_t* commitment, size_t commitment_len, int32_t* ok);
/* DensePolynomial::merge(vecs).commit(gens, Some(tape)): ONE draw random_vector("poly_blinds", L'), L' = 2^((nv + kappa) / 2), serves the whole merge; every row is blinded,
 * the rows of the zero blocks behind k too (they are blinds[i] * h, not the identity's encoding).  blinds_out: L' elements. */
int32_t lasso_host_polys_commit_blinded(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s,
                                        const lasso_transcript_vtbl* tape, void* tape_user, lasso_fr* blinds_out, uint8_t* out, size_t cap, size_t* len);
/* lasso_host_polys_open under the L' row blinds (NULL: zero).  The evaluations stay in the clear — CombinedTableEvalProof appends them to the transcript — so the opening
 * verifies with lasso_host_polys_verify as it stands. */
int32_t lasso_host_polys_open_blinded(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len,
                                      const lasso_fr* blinds, const lasso_transcript_vtbl* transcript, void* transcript_user, const lasso_transcript_vtbl* tape, void* tape_user,
                                      lasso_fr* evals, uint8_t* proof, size_t cap, size_t* len);
/* *rows_device = rows this host has blinded on the device (lasso_points_reduce_compress) so far; *rows_host = rows blinded on the host: the decode route, and the rows of a
 * merge's zero blocks (blinds[i] * h alone).  Either may be NULL; reset != 0 zeroes both. */
int32_t lasso_host_blind_stats(lasso_host* h, uint64_t* rows_device, uint64_t* rows_host, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
