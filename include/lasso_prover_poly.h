/* lasso_prover_poly.h — a commitment to a caller's vector and its opening at a point, at the host prover's C ABI: DensePolynomial::commit (dense_mlpoly.rs:153-181),
 * PolyCommitment::append_to_transcript (:281-289), PolyEvalProof::prove / verify_plain (:302-400) and PolyCommitmentGens::new (:38-45), blinds None throughout.
 * What it is for: lasso_host_lookup_values gives v[k] = combine_lookups(T[dim(k)]) and the Lasso proof's one scalar is MLE(v)(r) (lasso_prover_values.h).  A verifier does
 * not hold v.  It holds a commitment to v; an opening of that commitment at r to the proof's claimed_evaluation makes the scalar a statement about committed lookup results:
 *   prover    c = poly_commit(v);  proof = lasso_host_prove_cb(.., r, transcript, tape);  opening = poly_open(v, r, the same transcript and tape)   (Zr comes back too)
 *   verifier  lasso_host_verify_cb(proof) on its transcript;  Zr = lasso_host_proof_claimed_evaluation(proof);  poly_verify(c, r, Zr, opening) on the same transcript
 * The code is the Lasso prover's and verifier's own (Prover::poly_eval_prove_resident, Prover::dot_product_log_prove, Verifier::poly_eval_verify_plain), not a copy.
 * Vectors come as field elements or as 64-bit integers (enum lasso_values_form, lasso_hip_values.h), from host memory or from device memory of this host's context.  The
 * 64-bit form is read as it is on the device (include/lasso_hip_poly.h: 8 bytes per element in the commitment's MSM and in the opening's L * Z).  Those device entries are
 * weak references of the library: linked against an implementation of lasso_hip.h alone, the integers are lifted to field elements on the host and the 32-byte entries
 * serve — the bytes are the same.  Blinded (hiding) commitments and openings: include/lasso_prover_blind.h.  Not offered: slab mode (world > 1).  Several vectors under one commitment
 * and in one opening: include/lasso_prover_polys.h.
 * The evaluation of a 64-bit vector at r is Zr of lasso_host_poly_open (the opening computes <L * Z, R> anyway); lasso_host_values_evaluate keeps taking field elements only.
 * Separate from lasso_prover.h for the reason lasso_prover_values.h is.  Exported by liblasso_prover.so and liblasso_prover_bn254.so. */
#ifndef LASSO_PROVER_POLY_H
#define LASSO_PROVER_POLY_H
#include "lasso_prover.h"
#include "lasso_hip_values.h"
#ifdef __cplusplus
extern "C" {
#endif

typedef struct lasso_host_poly_gens lasso_host_poly_gens;
/* PolyCommitmentGens::new(num_vars, label): the first n + 2 points of the label's stream, n = 2^(num_vars - num_vars / 2).  num_vars = 1 .. 30. */
int32_t lasso_host_poly_gens_new(lasso_host* h, const char* label, size_t num_vars, lasso_host_poly_gens** out);
/* The caller's own generators: n + 2 affine points [G[0..n), gens_1.G[0], h] in the order and form lasso_host_gens_from_points takes one set; any other count is refused. */
int32_t lasso_host_poly_gens_from_points(lasso_host* h, size_t num_vars, const lasso_affine* points, size_t n_points, lasso_host_poly_gens** out);
void lasso_host_poly_gens_free(lasso_host_poly_gens* g);

/* DensePolynomial::commit(gens, None) of the s = 2^num_vars values: out = [u64 L][L x 32 B], L = 2^(num_vars / 2) rows — one block of lasso_host_commit's layout.
 * values: s elements of `form` (LASSO_VALUES_FR: memory form, any representative a device array may hold; LASSO_VALUES_U64); on_device = 0: host memory, 8-byte aligned;
 * 1: device memory of this host's context, 16-byte aligned.  cap / *len as for lasso_host_commit (-2 when cap is too small, *len set).
 * -1 with a message: num_vars outside 1 .. 30 (the generators'), s not a power of two or not 2^num_vars, a slab-mode host, a misaligned pointer. */
int32_t lasso_host_poly_commit(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, uint8_t* out, size_t cap, size_t* len);
/* PolyCommitment::append_to_transcript(label): begin, one poly_commitment_share per row, end — against the caller's live transcript.  The rows are absorbed as the bytes
 * given (a verifier that has not decoded them yet learns of a bad encoding from lasso_host_poly_verify). */
int32_t lasso_host_poly_commitment_append(const lasso_transcript_vtbl* transcript, void* transcript_user, const char* label, const uint8_t* commitment, size_t len);
/* PolyEvalProof::prove(poly, None, r, Zr, None, gens, transcript, tape) with Zr = poly.evaluate(r) computed on the way (<L * Z, R>) and returned in *Zr (memory form, fully
 * reduced; may be NULL).  proof = the serialized DotProductProofLog, as it stands inside a Lasso proof.  r: r_len = num_vars field elements.  Arguments and refusals as for
 * lasso_host_poly_commit. */
int32_t lasso_host_poly_open(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len,
                             const lasso_transcript_vtbl* transcript, void* transcript_user, const lasso_transcript_vtbl* tape, void* tape_user,
                             lasso_fr* Zr, uint8_t* proof, size_t cap, size_t* len);
/* PolyEvalProof::verify_plain(gens, transcript, r, Zr, commitment): *ok = 1 (Ok) or 0 (Err).  Bytes that do not deserialize (truncated, trailing data, a non-canonical
 * scalar, an invalid point encoding) and shapes the reference asserts on (rows of the commitment, generator count against r_len) are -1 with the reason. */
int32_t lasso_host_poly_verify(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const lasso_fr* Zr, const lasso_transcript_vtbl* transcript, void* transcript_user,
                               const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok);
/* *u64_commit_elements / *u64_open_elements = 64-bit elements this host has committed to / opened through the device entries of lasso_hip_poly.h so far (the host-lift
 * route counts nothing); *available = 1 when the device library has all three entries; any may be NULL; reset != 0 zeroes the counters. */
int32_t lasso_host_poly_stats(lasso_host* h, uint64_t* u64_commit_elements, uint64_t* u64_open_elements, int32_t* available, int32_t reset);

#ifdef __cplusplus
}
#endif
#endif
