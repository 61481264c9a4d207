// Label-derived generators on the device (include/lasso_hip_gens.h): stream candidates turned into points, one lane per candidate.
// A curve25519 candidate costs ~290 products for the combined inversion / square root, 3 x 8 for the cofactor's doublings and ~270 for the normalising inversion;
// a BN254 candidate ~380 (the root and its check).  The 17 k candidates of the headline's generator set are 270 waves: as in wire_kernels.cuh every wave has a SIMD
// to itself and the launch takes one candidate's time, so one lane per candidate and workgroups of ONE wave (the batch spreads over as many compute units as it
// has waves).
#pragma once
#include "fe29.cuh"

#define GENS_THREADS 64
__global__ void __launch_bounds__(GENS_THREADS) k_points_from_candidates(const uint4* __restrict__ limbs, const uint8_t* __restrict__ greatest, size_t n, uint4* __restrict__ aff, uint8_t* __restrict__ status) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 lo = limbs[2 * i], hi = limbs[2 * i + 1];
  const uint32_t in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t a[16];
  const uint32_t st = pt_from_candidate(in, greatest[i] != 0, a);
#pragma unroll
  for (int k = 0; k < 4; k++) aff[4 * i + k] = make_uint4(a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]);
  status[i] = (uint8_t)st;
}
