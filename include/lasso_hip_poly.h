/* lasso_hip_poly.h — a caller's vector of 64-bit integers as a multilinear polynomial: Z[i] = F::from(v[i]), committed to (DensePolynomial::commit, dense_mlpoly.rs:153-181)
 * and multiplied from the left by an eq half (dense_mlpoly.rs:184-207, the pass over the whole vector that PolyEvalProof::prove makes) without the 32-byte elements ever
 * being formed.  lasso_lookup_values (lasso_hip_values.h) writes the lookup results in this form where they fit: 8 bytes per lookup instead of 32.
 * This header is separate so that a library which implements lasso_hip.h alone stays a complete implementation of that header.  Exported by liblasso_hip.so and
 * liblasso_hip_bn254.so.  No kernel behind these entries waits on the device for the host; every argument check fails before anything is launched; scratch requests go
 * through the context's guarded, pattern-filled scratch like every other entry's (LASSO_SCRATCH_GUARD, LASSO_POISON). */
#ifndef LASSO_HIP_POLY_H
#define LASSO_HIP_POLY_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* *out = the OR of d_v[0 .. n): which bits are populated (the smallest bound of the form 2^k - 1).  d_v: device memory, 8-byte aligned; n >= 1.  One pass, 8 bytes per
 * element; synchronous (the word comes back).  Not legal while a launch of the context waits on the device for its challenge.  Profiling family LASSO_K_MISC. */
int32_t lasso_u64_or(lasso_ctx* ctx, const uint64_t* d_v, size_t n, uint64_t* out);

/* lasso_hyrax_commit_compressed for Z[i] = F::from(d_v[i]): row j of the l_size x r_size matrix is committed over the first r_size generators, out32 receives l_size x 32
 * wire bytes.  max_value bounds every element (a larger element is the caller's error: its high bits are ignored, nothing outside the arrays is touched).
 *   max_value < 2^32   the low words are written to the scratch (8 bytes read, 4 written per element) and the commitment is lasso_hyrax_commit_compressed_u32's from there
 *                      on, byte-multiple tables included where that call would take them
 *   otherwise          the bucket kernel reads the 8-byte scalars in place: ceil(bits(max_value) / 4) <= 16 windows of 4 bits over the nibble-window table.  No 64-bit
 *                      byte-window tables are built and the 12-bit-window kernels are not used (they take 32-byte scalars).
 * d_v: device memory, 8-byte aligned.  Synchronous like lasso_hyrax_commit_compressed.  Same group elements, hence the same bytes, as that call on the lifted array. */
int32_t lasso_hyrax_commit_compressed_u64(lasso_ctx* ctx, const uint64_t* d_v, uint64_t max_value, size_t l_size, size_t r_size, const lasso_bases* bases, uint8_t* out32);

/* d_out[col] = sum_j d_L[j] * F::from(d_Z[j * r_size + col]), col < r_size: lasso_matvec_left_dev over integers.  d_Z: l_size * r_size 64-bit integers, 16-byte aligned;
 * d_L: l_size field elements in memory form (any representative a device array may hold); d_out: r_size field elements, canonical — the bytes lasso_matvec_left_dev writes
 * for the lifted array.  Enqueued on the context's stream (not synchronous); scratch: the row-chunk partials, as for lasso_matvec_left_dev.  Profiling family LASSO_K_MATVEC
 * with 8 bytes per element. */
int32_t lasso_matvec_left_u64_dev(lasso_ctx* ctx, const uint64_t* d_Z, const lasso_fr* d_L, size_t l_size, size_t r_size, lasso_fr* d_out);

#ifdef __cplusplus
}
#endif
#endif
