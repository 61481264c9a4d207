// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_POLY): the three entry points of include/lasso_hip_poly.h as literal loops over the oracle's field type and MSM, so that
// lasso_host_poly_commit and lasso_host_poly_open take the 64-bit route on the CPU; a library built without this fragment takes the host lift.
#include "../../include/lasso_hip_poly.h"

extern "C" int32_t lasso_u64_or(lasso_ctx* c, const uint64_t* v, size_t n, uint64_t* out) {
  REQ(c, v && out && n >= 1);
  uint64_t acc = 0; for (size_t i = 0; i < n; i++) acc |= v[i];
  *out = acc; return 0;
}
extern "C" int32_t lasso_hyrax_commit_compressed_u64(lasso_ctx* c, const uint64_t* v, uint64_t max_value, size_t ls, size_t rs, const lasso_bases* b, uint8_t* out32) {
  REQ(c, v && out32 && b && ls >= 1 && rs >= 1 && rs <= b->pts.size());
  std::vector<Point> bases(b->pts.begin(), b->pts.begin() + rs);
  for (size_t i = 0; i < ls; i++) {
    std::vector<Fr> sc(rs);
    for (size_t j = 0; j < rs; j++) { REQ(c, v[i * rs + j] <= max_value); sc[j] = Fr::from_u64(v[i * rs + j]); }
    msm(bases, sc).compress(out32 + 32 * i);   // dense_mlpoly.rs:118-127, commitments.rs:84-93 with blind = 0
  }
  return 0;
}
extern "C" int32_t lasso_matvec_left_u64_dev(lasso_ctx* c, const uint64_t* Z, const lasso_fr* L, size_t ls, size_t rs, lasso_fr* out) {
  REQ(c, Z && L && out && ls >= 1 && rs >= 1);
  for (size_t i = 0; i < rs; i++) { Fr s = Fr::zero(); for (size_t j = 0; j < ls; j++) s += F(L)[j] * Fr::from_u64(Z[j * rs + i]); F(out)[i] = s; }   // dense_mlpoly.rs:184-207
  return 0;
}
