// The device library's own launch decision for lasso_lookup_values (launch_plan.cuh values_plan, as the entry point calls it), printed for
// tests/test_lookup_values_cpu.py: argv = the x-extent cap (LASSO_VALUES_NX; 0 = unset), then any number of n; one JSON line per n and kernel shape.
#include "../../lasso_amd/csrc/launch_plan.cuh"
#include <cstdio>
#include <cstdlib>

int main(int argc, char** argv) {
  const long cap = argc > 1 ? atol(argv[1]) : 0;
  for (int a = 2; a < argc; a++) {
    const size_t n = (size_t)strtoull(argv[a], nullptr, 10);
    for (int pair = 0; pair < 2; pair++) {
      const ValuesPlan p = values_plan(n, pair != 0, cap);
      printf("{\"n\": %zu, \"pair\": %d, \"per_item\": %u, \"items\": %llu, \"nx\": %u, \"passes\": %llu, \"last_block_items\": %llu, \"block\": %d, \"max_nx\": %u}\n", n, pair, p.per_item,
             (unsigned long long)p.items, p.nx, (unsigned long long)p.passes, (unsigned long long)p.last_block_items, LASSO_BLOCK, VALUES_MAX_NX);
    }
  }
  return 0;
}
