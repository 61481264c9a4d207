/* lasso_hip_operands.h — densify from OPERAND columns: the chunk indices of a strategy are formed on the device, inside the densify pass.
 * lasso_densify_dim(_slab) (lasso_hip.h) read the reference's Vec<[usize; C]>: 8 C bytes per lookup, an artefact of the decomposition into C chunks.  What a caller
 * holds are operands — two 64-bit columns x, y for AND / OR / XOR / LT, one for a range check: 16 or 8 bytes per lookup, whatever C is.  This header is separate, as
 * lasso_hip_wire.h and lasso_hip_msm.h are, so that a library which implements lasso_hip.h alone stays a complete implementation of that header.  Exported by
 * liblasso_hip.so and liblasso_hip_bn254.so. */
#ifndef LASSO_HIP_OPERANDS_H
#define LASSO_HIP_OPERANDS_H
#include "lasso_hip.h"
#ifdef __cplusplus
extern "C" {
#endif

/* How an operand pair becomes the C table addresses of one lookup.  For dimension dim of C:
 *     j        = msb_first ? C - 1 - dim : dim
 *     chunk(v) = (j * chunk_bits >= 64) ? 0 : (v >> (j * chunk_bits)) & (2^chunk_bits - 1)
 *     index    = operands == 2 ? (chunk(x) << chunk_bits) | chunk(y) : chunk(x)
 * and an operand v FITS when C * chunk_bits >= 64 or v < 2^(C * chunk_bits).  lasso_amd/csrc/operand_layout.cuh is this statement as code (host and device compile the
 * same text); lasso_host_operand_indices (lasso_prover.h) is its CPU entry point.  The built-in strategies' layouts (lasso_host_operand_layout) follow the reference:
 *     AND / OR / XOR   {2, log_m / 2, 0}   split_bits(idx, log M / 2) = (lhs, rhs), chunk i weighs 2^(i b)                       and.rs, or.rs, xor.rs
 *     LT               {2, log_m / 2, 1}   LT[0] is unconditioned: dimension 0 is the MOST significant chunk                       lt.rs:60-69
 *     RangeCheck       {1, log_m, 0}       chunk i weighs 2^(i log_m)                                                            range_check.rs:78-86
 * A caller who gets the layout wrong proves a different statement, and that proof verifies: the layout is part of the statement. */
typedef struct {
  uint32_t operands;    /* 1 or 2 columns */
  uint32_t chunk_bits;  /* b: bits taken from EACH operand per dimension; 1 <= b, operands * b <= log_m */
  uint32_t msb_first;   /* 0: dimension i takes chunk i counted from the least significant end;
                           1: dimension i takes chunk C-1-i (dimension 0 = the top chunk) */
} lasso_operand_layout;

/* lasso_densify_dim_slab (lasso_hip.h) with the dimension's addresses formed from the operand columns instead of read from an index array: same outputs, same semantics
 * (world = 1, rank = 0 is the single-GPU form; the padded tail k >= n_lookups has address 0), same sort, run and timestamp kernels — only the first kernel differs, and it
 * reads 8 (one operand) or 16 contiguous bytes per lookup.  d_x, d_y: n_lookups device-resident 64-bit operands each; d_y is NULL exactly when layout->operands == 1.
 * LASSO_ERR_INVALID with a message of its own when an operand does not fit (its key is clamped to 0 before anything indexes by it; the context stays usable), when the
 * layout breaks a rule above, or on the conditions lasso_densify_dim_slab puts on s, log_m, world and rank.  Synchronous. */
int32_t lasso_densify_dim_operands(lasso_ctx* ctx, const uint64_t* d_x, const uint64_t* d_y, size_t n_lookups, const lasso_operand_layout* layout, size_t C, size_t dim, size_t s,
                                   uint32_t log_m, uint32_t world, uint32_t rank, uint32_t* d_dim_u32, lasso_fr* d_dim, lasso_fr* d_read, lasso_fr* d_final);

#ifdef __cplusplus
}
#endif
#endif
