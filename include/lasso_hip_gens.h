/* lasso_hip_gens.h — label-derived generators on the device: the ARITHMETIC half of ark-ec's `Projective::rand` (coordinate to point, or no point) for a batch of
 * candidates the host has drawn from the ChaCha stream.  This header is separate so that a library which implements lasso_hip.h alone stays a complete
 * implementation of that header.  Exported by liblasso_hip.so and liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_GENS_H
#define LASSO_HIP_GENS_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Outcome of ONE candidate. */
#ifndef LASSO_CAND_STATUS_DEFINED
#define LASSO_CAND_STATUS_DEFINED
enum lasso_cand_status {
  LASSO_CAND_OK = 0,            /* a point was produced */
  LASSO_CAND_NONCANONICAL = 1,  /* the limbs are not below the field modulus: no arithmetic done, output zero */
  LASSO_CAND_NO_POINT = 2       /* no curve point has this coordinate (curve25519: (1 - y^2) / (-1 - d y^2) is no square, or the denominator is 0; BN254: x^3 + 3 is no
                                   square): output zero */
};
#endif

/* n candidates in, per candidate a status and a point out.  Candidate i is
 *   limbs[4 i .. 4 i + 4)   four 64-bit words that ARE ark-ff's Montgomery representation of the coordinate (curve25519: y; BN254: x), exactly as Fq::rand takes
 *                           them from the stream after masking the top bits
 *   greatest[i]             non-zero: the larger of the two roots (as canonical integers), zero: the smaller — the bool `rand` draws after the coordinate
 * and yields
 *   status[i]               a lasso_cand_status
 *   out[i]                  the affine point in the limb form lasso_bases_create takes (canonical Montgomery limbs); all zero unless status[i] == LASSO_CAND_OK.
 *                           curve25519: the point times the cofactor 8, normalised — a small-order start leaves as the affine identity (0, 1).  BN254: cofactor 1,
 *                           out[i].x is limbs[4 i .. 4 i + 4).
 * All pointers are host pointers; out may be NULL; n = 0 is a no-op.  Synchronous: one upload, one launch (k_points_from_candidates, one lane per candidate),
 * one download.  Scratch comes from the context's pool: LASSO_ERR_UNSUPPORTED when the buffer would have to grow while a resident kernel is active.
 * Returns 0 even when some candidates yield no point — that is data, reported per candidate; non-zero only for bad arguments or a device error. */
int32_t lasso_points_from_candidates(lasso_ctx* ctx, const uint64_t* limbs, const uint8_t* greatest, size_t n, lasso_affine* out, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif
