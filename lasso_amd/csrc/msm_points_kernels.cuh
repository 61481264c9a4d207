// Table-free MSM over the CALLER's points (include/lasso_hip_msm.h: VariableBaseMSM::msm, src/msm/mod.rs:36-40) for gfx950.
//
// Every other MSM of this library runs over a lasso_bases object: 64 window multiples per point with an inversion each, plus the digit- and byte-multiple tables.  That is
// the right trade for generators and the wrong one for points used once (the verifier's commitment rows).  Here nothing is precomputed and nothing is inverted:
//   k_msmp_prepare   one lane per point: affine -> Niels form (no inversion on either curve), the Montgomery scalar -> its canonical integer -> 33 signed 8-bit digits
//                    (msm_points_recode.cuh).  An all-zero affine entry stands for the identity: its digits are all zero, so it costs nothing further;
//   k_msmp_buckets   one workgroup per (window, chunk of 1024 points): k_msm_buckets' scheme with 128 buckets (digit magnitudes 1 .. 128, the sign applied to the Niels
//                    entry for free) — LDS counting sort of the chunk's (digit, point) pairs, the 256 threads shared out over the buckets in proportion to their pair
//                    counts (every bucket keeps one thread; all scalars equal = one bucket with 129 threads, not one thread with 1024 additions), the next entry fetched
//                    while the current one is added, a segmented LDS tree per bucket.  Then sum_d d B_d by running sums: lane t < 32 owns digits 4t+1 .. 4t+4
//                    (S_t = their sum, T_t = sum_k (k+1) B_{4t+k+1}), and sum_d d B_d = sum_t T_t + 4 sum_t t S_t, the last sum through a suffix scan of the S_t;
//   k_points_sum     (msm_kernels.cuh, its pt29 output form) adds the chunks of each window;
//   k_msmp_horner    one lane: 32 x (8 doublings + 1 addition) join the 33 window sums, and the result leaves in the ABI's point form.
// Cost model (n points): 33 n mixed additions spread over 33 ceil(n / 1024) workgroups (2^13 points: 264 workgroups, 4 additions per lane), a fixed ~45 additions deep
// tail per workgroup, and the 256 dependent doublings of the last kernel — the latency floor of any table-free MSM, and at verifier sizes the whole cost.
// The group laws are complete on both builds (fe29.cuh: unified Edwards addition on the prime-order subgroup; bn254_fe29.cuh: Renes-Costello-Batina), so equal points,
// P and -P in one bucket and buckets that sum to the identity need no special case, and none is made.
#pragma once
#include "msm_kernels.cuh"
#include "msm_points_recode.cuh"

#define MSMP_BUCKETS (1u << (MSMP_C - 1u))     // 128 digit magnitudes
#define MSMP_CHUNK 1024u                       // points per workgroup (the LDS sort buffer holds 9216 pairs)
static_assert(2 * MSMP_BUCKETS == MSM_THREADS && MSMP_CHUNK * 4 <= MSM_THREADS * sizeof(pt29), "k_msmp_buckets: two sort bins and at least one thread per bucket");

// nl[j] = Niels form of points[j]; dig[w * n + j] = digit w of scalars[j] (window-major: a workgroup of k_msmp_buckets reads one contiguous run)
__global__ void __launch_bounds__(256) k_msmp_prepare(const fq_t* __restrict__ aff, const fr_t* __restrict__ scal, uint32_t n, niels29* __restrict__ nl, int8_t* __restrict__ dig) {
  const uint32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const fq_t x = aff[2 * (size_t)j], y = aff[2 * (size_t)j + 1];
  uint32_t any = 0;
#pragma unroll
  for (int k = 0; k < 8; k++) any |= x.v[k] | y.v[k];
#ifdef LASSO_BN254
  nl[j] = niels_from_affine(x, y);
#else
  nl[j] = niels_from_affine(fq_from_mont(x), fq_from_mont(y));
#endif
  fr_t s = fr29_to_integer(fr29_unpack_u(scal[j]));
  if (!any) { for (int k = 0; k < 8; k++) s.v[k] = 0; }   // (0, 0) is on neither curve: the identity, skipped
  uint32_t carry = 0;
#pragma unroll 1
  for (uint32_t w = 0; w < MSMP_NW; w++) dig[(size_t)w * n + j] = (int8_t)msmp_digit(s.v, MSMP_C, w, carry);
}

// grid = (MSMP_NW windows, K chunks).  out[w * K + chunk] = sum over the chunk's points of digit_w * point (pt29)
__global__ void __launch_bounds__(MSM_THREADS) k_msmp_buckets(const int8_t* __restrict__ dig, uint32_t n, const niels29* __restrict__ nl, pt29* __restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t raw[MSM_THREADS * sizeof(pt29)];   // sorted[] during accumulation, points during the trees
  __shared__ uint32_t counts[MSM_THREADS], start[MSM_THREADS], cursor[MSM_THREADS];
  __shared__ uint32_t toff[MSMP_BUCKETS + 2], tree_top;
  uint32_t* sorted = reinterpret_cast<uint32_t*>(raw);
  pt29* pts = reinterpret_cast<pt29*>(raw);
  const fe29 d2 = fe_d2();
  const uint32_t t = threadIdx.x;
  const int8_t* row = dig + (size_t)blockIdx.x * n;
  const uint32_t c0 = blockIdx.y * MSMP_CHUNK;
  uint32_t c1 = c0 + MSMP_CHUNK; if (c1 > n) c1 = n; if (c1 < c0) c1 = c0;
  // counting sort by digit magnitude; two bins per bucket (even / odd points) keep the LDS atomics apart
  counts[t] = 0;
  __syncthreads();
  for (uint32_t c = c0 + t; c < c1; c += MSM_THREADS) {
    const int32_t d = row[c];
    if (d) atomicAdd(&counts[(((uint32_t)(d < 0 ? -d : d) - 1u) << 1) | (c & 1u)], 1u);
  }
  __syncthreads();
  start[t] = counts[t];
  __syncthreads();
  for (uint32_t off = 1; off < MSM_THREADS; off <<= 1) { const uint32_t v = t >= off ? start[t - off] : 0; __syncthreads(); start[t] += v; __syncthreads(); }   // inclusive scan
  cursor[t] = start[t] - counts[t];
  __syncthreads();
  for (uint32_t c = c0 + t; c < c1; c += MSM_THREADS) {
    const int32_t d = row[c];
    if (d) sorted[atomicAdd(&cursor[(((uint32_t)(d < 0 ? -d : d) - 1u) << 1) | (c & 1u)], 1u)] = c | (d < 0 ? 0x80000000u : 0u);   // at most MSMP_CHUNK pairs: inside raw[]
  }
  // the threads over the buckets, in proportion to the pair counts; every bucket keeps one thread (128 + at most 128 shared out = at most 256)
  if (t == 0) {
    const uint32_t total = start[MSM_THREADS - 1];
    uint32_t acc = 0, top = 1; toff[0] = 0; toff[1] = 0;
    for (uint32_t d = 1; d <= MSMP_BUCKETS; d++) {
      const uint32_t b = 2u * (d - 1u), cnt = start[b + 1] - (start[b] - counts[b]);
      const uint32_t T = 1u + (total ? (uint32_t)(((uint64_t)cnt * (MSM_THREADS - MSMP_BUCKETS)) / total) : 0u);
      acc += T; toff[d + 1] = acc; if (T > top) top = T;
    }
    uint32_t p2 = 1; while (p2 < top) p2 <<= 1;
    tree_top = p2 >> 1;
  }
  __syncthreads();
  uint32_t my_d = 0, my_j = 0, my_T = 0;   // this thread's digit magnitude, its rank among the bucket's threads, and how many threads share the bucket
  for (uint32_t d = 1; d <= MSMP_BUCKETS; d++) if (t >= toff[d] && t < toff[d + 1]) { my_d = d; my_j = t - toff[d]; my_T = toff[d + 1] - toff[d]; }
  pt29 B = pt_identity();
  if (my_T) {
    const uint32_t b = 2u * (my_d - 1u), lo = start[b] - counts[b], hi = start[b + 1];
    uint32_t pos = lo + my_j;
    if (pos < hi) {
      uint32_t p_cur = sorted[pos];
      niels29 cur = nl[p_cur & 0x7fffffffu];
      for (pos += my_T; pos < hi; pos += my_T) {
        const uint32_t p_nxt = sorted[pos];
        const niels29 nxt = nl[p_nxt & 0x7fffffffu];   // in flight during the addition below
        B = pt_madd(B, niels_cond_neg(cur, (p_cur >> 31) != 0));
        cur = nxt; p_cur = p_nxt;
      }
      B = pt_madd(B, niels_cond_neg(cur, (p_cur >> 31) != 0));
    }
  }
  __syncthreads();   // sorted[] has been read: raw[] becomes points
  pts[t] = B;
  __syncthreads();
  // segmented tree: the threads of one bucket are contiguous; pts[toff[d]] ends up holding B_d
  for (uint32_t s = tree_top; s > 0; s >>= 1) {
    pt29 sum;
    const bool act = my_j < s && my_j + s < my_T;
    if (act) sum = pt_add(pts[t], pts[t + s], d2);
    __syncthreads();
    if (act) pts[t] = sum;
    __syncthreads();
  }
  // running sums over four digits per lane, read where the tree left them: R = S_t, T = sum_k (k + 1) B_{4t+k+1}
  constexpr uint32_t PER = 4, LANES = MSMP_BUCKETS / PER;   // 32
  pt29 R = pt_identity(), T = pt_identity();
  if (t < LANES) {
#pragma unroll 1
    for (uint32_t k = PER; k-- > 0;) { R = pt_add(R, pts[toff[PER * t + k + 1]], d2); T = pt_add(T, R, d2); }
  }
  __syncthreads();
  if (t < LANES) { pts[t] = T; pts[LANES + t] = R; }
  __syncthreads();
  for (uint32_t off = 1; off < LANES; off <<= 1) {   // inclusive suffix sums of the S_t in pts[32 .. 64)
    pt29 v; const bool a = t < LANES && t + off < LANES;
    if (a) v = pts[LANES + t + off];
    __syncthreads();
    if (a) pts[LANES + t] = pt_add(pts[LANES + t], v, d2);
    __syncthreads();
  }
  if (t == 0) pts[LANES] = pt_identity();   // sum_t t S_t = sum_{j >= 1} suffix_j
  __syncthreads();
  // two trees side by side: lanes 0 .. 31 over the T_t, lanes 32 .. 63 over the suffix sums
  const uint32_t base = t < LANES ? 0u : LANES, i = t & (LANES - 1u);
  for (uint32_t s = LANES / 2; s > 0; s >>= 1) {
    if (t < 2 * LANES && i < s) pts[base + i] = pt_add(pts[base + i], pts[base + i + s], d2);
    __syncthreads();
  }
  if (t == 0) out[(size_t)blockIdx.x * gridDim.y + blockIdx.y] = pt_add(pts[0], pt_dbl(pt_dbl(pts[LANES])), d2);   // + 4 sum_t t S_t
}

// wsum[w] = the sum of window w (k_points_sum's pt29 output).  out = sum_w 2^(8 w) wsum[w] in the ABI's point form: one lane, the chain of doublings no table-free MSM avoids
__global__ void __launch_bounds__(64) k_msmp_horner(const pt29* __restrict__ wsum, ed_point* __restrict__ out) {
  if (threadIdx.x != 0 || blockIdx.x != 0) return;
  const fe29 d2 = fe_d2();
  pt29 acc = pt_add(pt_identity(), wsum[MSMP_NW - 1], d2);
#pragma unroll 1
  for (uint32_t w = MSMP_NW - 1; w-- > 0;) {
#pragma unroll 1
    for (uint32_t k = 0; k < MSMP_C; k++) acc = pt_dbl(acc);
    acc = pt_add(acc, wsum[w], d2);
  }
#ifdef LASSO_BN254
  out[0] = pt_to_abi(acc);
#else
  ed_point p = pt_to_ed(acc), o; o.X = fq_to_mont(p.X); o.Y = fq_to_mont(p.Y); o.T = fq_to_mont(p.T); o.Z = fq_to_mont(p.Z); out[0] = o;
#endif
}
