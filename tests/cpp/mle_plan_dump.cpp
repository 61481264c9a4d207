// The device library's own launch decision for lasso_tables_mle (launch_plan.cuh mle_plan, as tables_mle_impl calls it), printed for tests/test_mle_cpu.py: one JSON line
// per table size with the whole-table plan, and — argv: strip lengths — the plans of every strip of a 2^10-entry table at each given length.
#include "../../lasso_amd/csrc/launch_plan.cuh"
#include <cstdio>
#include <cstdlib>

static void line(uint32_t log_m, uint64_t e0, uint64_t e1, uint64_t strip) {
  const MlePlan p = mle_plan(log_m, e0, e1);
  printf("{\"log_m\": %u, \"e0\": %llu, \"e1\": %llu, \"strip\": %llu, \"hi_bits\": %u, \"lo_bits\": %u, \"row_first\": %u, \"rows\": %u, \"rows_per_task\": %u, \"tasks\": %llu, \"nx\": %u, \"max_nx\": %u, "
         "\"block\": %d, \"rows_per_task_default\": %u, \"max_nx_cap\": %u}\n",
         log_m, (unsigned long long)e0, (unsigned long long)e1, (unsigned long long)strip, p.hi_bits, p.lo_bits, p.row_first, p.rows, p.rows_per_task, (unsigned long long)p.tasks, p.nx,
         mle_max_nx(log_m, strip ? strip : e1 - e0), LASSO_BLOCK, MLE_ROWS_PER_TASK, MLE_MAX_NX);
}

int main(int argc, char** argv) {
  for (uint32_t log_m = 1; log_m <= 30; log_m++) line(log_m, 0, (uint64_t)1 << log_m, 0);
  for (int a = 1; a < argc; a++) {
    const uint64_t strip = strtoull(argv[a], nullptr, 10), m = 1 << 10;
    for (uint64_t e0 = 0; strip && e0 < m; e0 += strip) line(10, e0, e0 + strip < m ? e0 + strip : m, strip);
  }
  printf("{\"strip_default_32_fr\": %llu, \"strip_default_1_u32\": %llu}\n", (unsigned long long)mle_strip_len(32, 32, 0), (unsigned long long)mle_strip_len(1, 4, 0));
  return 0;
}
