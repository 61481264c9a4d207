// The reading half of the wire format on the device (include/lasso_hip_wire.h): ark-serialize compressed points decoded and validated, one lane per point.
// A curve25519 point costs ~290 products for the combined inversion / square root and ~2600 for the subgroup check [l]P == O; a BN254 point ~380 (the root and its
// check).  The verifier's 8.4 k points of the headline instance are 133 waves: every wave has a SIMD to itself and the launch takes one point's time.  Four lanes per
// point (pt_coop4_*) would shorten only the additions of the subgroup ladder (65 of its 317 steps; the doublings have no four-way form here), so one lane it is.
// Workgroups of ONE wave: the batch spreads over as many compute units as it has waves.
#pragma once
#include "fe29.cuh"

#define WIRE_THREADS 64
__global__ void __launch_bounds__(WIRE_THREADS) k_points_decompress(const uint4* __restrict__ wire, size_t n, uint4* __restrict__ aff, uint4* __restrict__ canon, uint8_t* __restrict__ status) {
  const size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x;
  if (i >= n) return;
  const uint4 lo = wire[2 * i], hi = wire[2 * i + 1];
  const uint32_t in[8] = {lo.x, lo.y, lo.z, lo.w, hi.x, hi.y, hi.z, hi.w};
  uint32_t a[16], c[8];
  const uint32_t st = pt_decompress(in, a, c);
#pragma unroll
  for (int k = 0; k < 4; k++) aff[4 * i + k] = make_uint4(a[4 * k], a[4 * k + 1], a[4 * k + 2], a[4 * k + 3]);
  canon[2 * i] = make_uint4(c[0], c[1], c[2], c[3]); canon[2 * i + 1] = make_uint4(c[4], c[5], c[6], c[7]);
  status[i] = (uint8_t)st;
}
