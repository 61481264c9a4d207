/* lasso_hip_msm.h — multi-scalar multiplication over the CALLER's points, with nothing prepared: no lasso_bases object, no window tables, no inversion per point.
 * lasso_msm (lasso_hip.h) runs over a lasso_bases, whose tables are the right trade for generators that live as long as a gens object and the wrong one for points
 * that are used once (the verifier's commitment rows).  This header is separate so that a library which implements lasso_hip.h alone stays a complete implementation
 * of that header.  Exported by liblasso_hip.so and liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_MSM_H
#define LASSO_HIP_MSM_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* VariableBaseMSM::msm (src/msm/mod.rs:36-40) over the caller's own points: out = sum_j scalars[j] * points[j].  Host pointers.
 *   points   n affine points in the limb form lasso_bases_create takes, ANY multiset of points of the group (repeats, P next to -P); an all-zero entry stands for the
 *            identity (what lasso_points_decompress writes for LASSO_WIRE_OK_IDENTITY) and is skipped
 *   scalars  n Montgomery-form field elements, any representative lasso_hip.h allows (lazily reduced ones included); zero scalars cost nothing
 *   n        0 is allowed (out = the identity), as is everything skipped; n < 2^28
 * Scratch comes from the context (counted by lasso_mem_stats): 257 bytes per point (161 for the _dev form, which uploads nothing) plus 4.8 KB per 1024 points.
 * LASSO_ERR_UNSUPPORTED, with a message, when that buffer would have to grow while a resident kernel is active.  Synchronous. */
int32_t lasso_msm_points(lasso_ctx* ctx, const lasso_affine* points, const lasso_fr* scalars, size_t n, lasso_point* out);
/* the same with points and scalars resident on the device: both arrays are only read (the digits and sorted pairs live in the context's scratch), `out` is host memory */
int32_t lasso_msm_points_dev(lasso_ctx* ctx, const lasso_affine* d_points, const lasso_fr* d_scalars, size_t n, lasso_point* out);

#ifdef __cplusplus
}
#endif
#endif
