// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_MSM_POINTS): the entry points of include/lasso_hip_msm.h, implemented on the mock's own literal MSM
// (oracle/lasso_oracle.hpp msm, the function its lasso_msm runs).  The verifier takes its table-free path on the CPU.  An all-zero affine entry is the identity and is
// skipped, as the header says.
#include "../../include/lasso_hip_msm.h"

extern "C" int32_t lasso_msm_points(lasso_ctx* c, const lasso_affine* points, const lasso_fr* scalars, size_t n, lasso_point* out) {
  if (!c || !out || (n && (!points || !scalars))) return LASSO_ERR_INVALID;
  std::vector<Point> bases; std::vector<Fr> sc;
  for (size_t i = 0; i < n; i++) {
    uint64_t any = 0; for (int k = 0; k < 4; k++) any |= points[i].x[k] | points[i].y[k];
    if (!any) continue;
    bases.push_back(Point::from_affine(Fq::from_raw(points[i].x), Fq::from_raw(points[i].y))); sc.push_back(F(scalars)[i]);
  }
  put_point(msm(bases, sc), out);
  return 0;
}
extern "C" int32_t lasso_msm_points_dev(lasso_ctx* c, const lasso_affine* d_points, const lasso_fr* d_scalars, size_t n, lasso_point* out) { return lasso_msm_points(c, d_points, d_scalars, n, out); }
