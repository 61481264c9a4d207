// A caller's vector of 64-bit integers as a polynomial (include/lasso_hip_poly.h): Z[i] = F::from(v[i]) is committed to and opened without ever forming the 32-byte elements.
//   k_u64_or            the OR of all elements (which bits are populated): one grid-stride pass, a wave OR-reduce, one atomic per wave — k_fr_to_u32's flag, 64 bits wide.
//   k_u64_to_u32        the low words, for vectors whose bound is below 2^32: 8 bytes read, 4 written; the commitment then takes the 4-byte route of the MSMs.
//   k_matvec_left_u64   L * Z (dense_mlpoly.rs:184-207), the pass over the whole vector an opening makes: 8 bytes per element instead of k_matvec_left's 32.
// k_matvec_left_u64.  grid = (blocks of 256 lane PAIRS of columns, matvec_plan's row chunks); the partials have k_matvec_left's layout and k_matvec_reduce finishes them.  A lane
// owns two adjacent columns: on an even element index they arrive as one 16-byte load; with an odd r_size every other row starts on an odd index and takes two 8-byte loads,
// and the last lane of an odd r_size owns one column.  Per element the product with L[j] (s-form) is fr29_mul_acc_u64: 27 multiply-adds into columns 0..10.  The carry pass
// is fr29_acc_carry cut to the columns this kernel can reach (fr29_acc_carry_u64, fr29.cuh) — a sum of 2^20 products of a 64-bit integer and a 261-bit operand is below
// 2^345, so column 11 (everything from 2^319 up, below 2^26) absorbs the top carry and columns 12..16 stay the constant zero they start as: 24 live 64-bit columns for the
// two sums instead of 34 (the entry point refuses more than 2^20 rows per chunk).  One pass every
// FR29_U64_ACC_PERIOD rows (mont29.cuh derives the 15).  At the end fr29_acc_reduce leaves the integer residue sum_j Z[j][col] L_j and one product with R2S lifts it to memory
// form: in (-2p, 3p) as in k_matvec_left, canonical after fr29_store — the same bytes k_matvec_left writes for the lifted array.
#pragma once
#include "poly_kernels.cuh"

__global__ void __launch_bounds__(256) k_u64_or(const uint64_t* __restrict__ src, size_t n, unsigned long long* __restrict__ out) {
  uint64_t acc = 0;
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) acc |= src[i];
  uint32_t lo = (uint32_t)acc, hi = (uint32_t)(acc >> 32);
  for (int off = 32; off > 0; off >>= 1) { lo |= (uint32_t)__shfl_down(lo, off, 64); hi |= (uint32_t)__shfl_down(hi, off, 64); }
  if ((threadIdx.x & 63) == 0 && (lo | hi)) atomicOr(out, ((unsigned long long)hi << 32) | lo);
}
__global__ void __launch_bounds__(256) k_u64_to_u32(const uint64_t* __restrict__ src, size_t n, uint32_t* __restrict__ dst) {
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) dst[i] = (uint32_t)src[i];
}

__global__ void __launch_bounds__(LASSO_BLOCK) k_matvec_left_u64(const uint64_t* __restrict__ Z, const fr_t* __restrict__ Lv, size_t l_size, size_t r_size, size_t rows_per_chunk,
                                                                  fr_t* __restrict__ partials) {
  const size_t col = 2 * (blockIdx.x * (size_t)blockDim.x + threadIdx.x);
  if (col >= r_size) return;
  const bool two = col + 1 < r_size;
  size_t j0 = (size_t)blockIdx.y * rows_per_chunk, j1 = j0 + rows_per_chunk; if (j1 > l_size) j1 = l_size;
  fr29_acc w0 = fr29_acc_zero(), w1 = fr29_acc_zero(); uint32_t cnt = 0;
  for (size_t j = j0; j < j1; j++) {
    const fr29 l = fr29_unpack_s(Lv[j]);
    const size_t e = j * r_size + col;
    uint64_t z0, z1 = 0;
    if (two && !(e & 1)) { const ulonglong2 v = *reinterpret_cast<const ulonglong2*>(Z + e); z0 = v.x; z1 = v.y; }
    else { z0 = Z[e]; if (two) z1 = Z[e + 1]; }
    fr29_mul_acc_u64(w0, z0, l); fr29_mul_acc_u64(w1, z1, l);
    if (++cnt == FR29_U64_ACC_PERIOD) { fr29_acc_carry_u64(w0); fr29_acc_carry_u64(w1); cnt = 0; }
  }
  fr29_acc_carry_u64(w0); fr29_acc_carry_u64(w1);
  const fr29 r2s = fr29_r2s();
  fr_t* o = partials + (size_t)blockIdx.y * r_size + col;
  o[0] = fr29_store(fr29_mul(fr29_acc_reduce(w0), r2s));
  if (two) o[1] = fr29_store(fr29_mul(fr29_acc_reduce(w1), r2s));
}
