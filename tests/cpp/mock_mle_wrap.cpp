// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_MLE): the entry points of include/lasso_hip_mle.h as a literal statement over the oracle's field type: the whole eq table
// by the oracle's EqPolynomial(point).evals(), then one serial dot product per table.  The verifier takes its device route on the CPU.
#include "../../include/lasso_hip_mle.h"

extern "C" int32_t lasso_tables_mle(lasso_ctx* c, const uint32_t* const* tables_u32, const lasso_fr* const* tables_fr, uint32_t num_tables, uint32_t log_m, const lasso_fr* point, lasso_fr* out) {
  REQ(c, point && out && (tables_u32 != nullptr) != (tables_fr != nullptr) && num_tables >= 1 && num_tables <= 32 && log_m >= 1 && log_m <= 30);
  for (uint32_t k = 0; k < num_tables; k++) REQ(c, tables_u32 ? tables_u32[k] != nullptr : tables_fr[k] != nullptr);
  const std::vector<Fr> pt(F(point), F(point) + log_m);
  const std::vector<Fr> chi = EqPolynomial(pt).evals();
  for (uint32_t k = 0; k < num_tables; k++) {
    Fr sum = Fr::zero();
    for (size_t i = 0; i < chi.size(); i++) sum += chi[i] * (tables_u32 ? Fr::from_u64(tables_u32[k][i]) : F(tables_fr[k])[i]);
    F(out)[k] = sum;
  }
  return 0;
}
extern "C" int32_t lasso_tables_mle_dev(lasso_ctx* c, const uint32_t* const* d_tables_u32, const lasso_fr* const* d_tables_fr, uint32_t num_tables, uint32_t log_m, const lasso_fr* point, lasso_fr* out) {
  return lasso_tables_mle(c, d_tables_u32, d_tables_fr, num_tables, log_m, point, out);
}
