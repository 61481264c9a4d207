// Test-only: tests/cpp/slab_threads.cpp (included, not edited) with every rank densifying from OPERAND columns: the harness's lasso_host_densify call is renamed to the shim
// below, which ignores the index array and calls lasso_host_densify_operands on the columns slab_set_operands stored.  Everything else — the ranks as threads, the shared-memory
// all-gather, commit, prove, the comparison between ranks — is the harness tests/test_slab_sharding_cpu.py uses.
#include "../../include/lasso_prover.h"
#include <atomic>

namespace {
lasso_operand_layout g_layout; const uint64_t* g_x = nullptr; const uint64_t* g_y = nullptr;
std::atomic<unsigned long long> g_device_dims{0};
int32_t densify_from_operands(lasso_host* h, const uint64_t*, size_t n_lookups, size_t c, size_t log_m, lasso_host_dense** out) {
  const int32_t rc = lasso_host_densify_operands(h, &g_layout, g_x, g_y, n_lookups, c, log_m, 0, out);
  uint64_t dims = 0;
  if (rc == 0 && lasso_host_densify_stats(h, &dims, nullptr, 0) == 0) g_device_dims += dims;
  return rc;
}
}  // namespace
extern "C" void slab_set_operands(const lasso_operand_layout* layout, const uint64_t* x, const uint64_t* y) { g_layout = *layout; g_x = x; g_y = y; g_device_dims = 0; }
extern "C" unsigned long long slab_operand_dims_on_device() { return g_device_dims; }   // summed over the ranks since slab_set_operands

#define lasso_host_densify densify_from_operands
#include "slab_threads.cpp"
#undef lasso_host_densify
