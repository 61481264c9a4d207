/* lasso_hip_wire.h — the READING half of the wire format: ark-serialize 0.4 compressed points (deserialize_compressed with Validate::Yes) decoded and
 * validated on the device.  The writing half (lasso_hyrax_commit_compressed, lasso_points_reduce_compress) is in lasso_hip.h; this header is separate so
 * that a library which implements lasso_hip.h alone stays a complete implementation of that header.  Exported by liblasso_hip.so and liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_WIRE_H
#define LASSO_HIP_WIRE_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* Outcome of decoding ONE 32-byte encoding, in the order the checks are made (the first failing check names the status). */
#ifndef LASSO_WIRE_STATUS_DEFINED
#define LASSO_WIRE_STATUS_DEFINED
enum lasso_wire_status {
  LASSO_WIRE_OK = 0,            /* a point of the prime-order group other than the BN254 identity */
  LASSO_WIRE_OK_IDENTITY = 1,   /* BN254: the infinity flag was set (the point is the identity WHATEVER canonical x the bytes hold) */
  LASSO_WIRE_NONCANONICAL = 2,  /* the coordinate is not below the field modulus (curve25519: y >= p; BN254: x >= q, checked even under the infinity flag) */
  LASSO_WIRE_BAD_FLAGS = 3,     /* BN254: both flag bits set — no SWFlags value */
  LASSO_WIRE_NOT_ON_CURVE = 4,  /* no point with this coordinate (curve25519: (1 - y^2) / (-1 - d y^2) is no square; BN254: x^3 + 3 is no square) */
  LASSO_WIRE_NOT_IN_SUBGROUP = 5 /* curve25519: on the curve, outside the prime-order subgroup ([l]P != O) */
};
#endif

/* Decode n encodings (wire32: n x 32 bytes).  Per point i:
 *   status[i]              a lasso_wire_status
 *   out[i]                 the affine point in the limb form lasso_bases_create takes; all zero unless status[i] == LASSO_WIRE_OK (the identity has no affine form)
 *   canon32[32 i .. +32)   serialize_compressed of the DECODED point — what a transcript absorbs; differs from the input for the malleable encodings (curve25519 x = 0 with
 *                          the sign bit; BN254 infinity flag over a non-zero x); all zero for a rejected encoding
 * All pointers are host pointers; out and canon32 may be NULL.  Synchronous: one upload, one launch (k_points_decompress, one lane per point), one download.
 * Returns 0 even when some encodings are invalid — invalid encodings are data, reported per point; non-zero only for bad arguments or a device error. */
int32_t lasso_points_decompress(lasso_ctx* ctx, const uint8_t* wire32, size_t n, lasso_affine* out, uint8_t* canon32, uint8_t* status);

#ifdef __cplusplus
}
#endif
#endif
