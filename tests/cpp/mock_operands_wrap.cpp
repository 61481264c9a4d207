// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_OPERANDS): the entry point of include/lasso_hip_operands.h, implemented as expand (the shared
// lasso_amd/csrc/operand_layout.cuh) then the mock's own lasso_densify_dim_slab — the reference's serial loop.  lasso_host_densify_operands takes its device path on the CPU.
#include "../../lasso_amd/csrc/operand_layout.cuh"

static size_t g_operand_calls = 0;
extern "C" size_t mock_operand_calls() { return g_operand_calls; }
extern "C" int32_t lasso_densify_dim_operands(lasso_ctx* c, const uint64_t* x, const uint64_t* y, size_t n_lookups, const lasso_operand_layout* layout, size_t C, size_t dim, size_t s, uint32_t log_m,
                                              uint32_t world, uint32_t rank, uint32_t* dim_u32, lasso_fr* d_dim, lasso_fr* d_read, lasso_fr* d_final) {
  REQ(c, x && dim_u32 && d_dim && d_read && d_final && C >= 1 && dim < C && n_lookups <= s);
  if (const int bad = operand_layout_check(layout, C, log_m)) { c->err = std::string("lasso_densify_dim_operands: ") + operand_layout_error(bad); return LASSO_ERR_INVALID; }
  if ((y != nullptr) != (layout->operands == 2u)) return fail(c, "lasso_densify_dim_operands: " OPL_MSG_Y);
  g_operand_calls++;
  std::vector<uint64_t> idx(n_lookups);      // this dimension's column only: C = 1, dim = 0 for the loop below
  for (size_t k = 0; k < n_lookups; k++) {
    const uint64_t vx = x[k], vy = y ? y[k] : 0;
    if (!operand_fits(vx, C, layout->chunk_bits) || !operand_fits(vy, C, layout->chunk_bits)) return fail(c, "lasso_densify_dim_operands: " OPL_MSG_FIT);
    idx[k] = operand_index(*layout, vx, vy, C, dim);
  }
  return lasso_densify_dim_slab(c, idx.data(), n_lookups, 1, 0, s, log_m, world, rank, dim_u32, d_dim, d_read, d_final);
}
