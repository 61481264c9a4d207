// CPU driver of lasso_amd/csrc/values_combine.cuh — the integer combine of k_lookup_values_int and the rule of the 64-bit form — for tests/test_lookup_values_cpu.py,
// which holds its output against Python integers, once built plain and once with -fsanitize=undefined (a shift past the width or a signed overflow is then a failure).
// stdin, any number of cases:
//   lin <kind> <c> <log_m> <n>  then n entries (decimal)     ->  offered bound_hi bound_lo sum_hi sum_lo l0 l1 l2 l3 l4      (sum = sum_i entry_i << (i * inc), 128 bits; its five limbs)
//   lt <c>  then c pairs  <lt> <eq>                           ->  g                                                             (the walk from the last chunk to the first)
#include "../../lasso_amd/csrc/values_combine.cuh"
#include <cstdio>
#include <cstring>
#include <cstdlib>

int main() {
  char what[8];
  while (scanf("%7s", what) == 1) {
    if (!strcmp(what, "lin")) {
      int kind; unsigned c, log_m, n;
      if (scanf("%d %u %u %u", &kind, &c, &log_m, &n) != 4) return 2;
      const uint32_t inc = values_inc(kind, log_m);
      values_u128 acc = 0;
      for (unsigned i = 0; i < n; i++) { unsigned long long e; if (scanf("%llu", &e) != 1) return 2; values_linear_add(acc, (uint32_t)e, i * inc); }
      const values_u128 b = values_linear_bound(c, inc, values_max_entry(kind, log_m));
      int32_t l[5]; values_limbs(acc, l);
      printf("%d %llu %llu %llu %llu %d %d %d %d %d\n", values_u64_offered(kind, c, log_m) ? 1 : 0, (unsigned long long)(b >> 64), (unsigned long long)b, (unsigned long long)(acc >> 64),
             (unsigned long long)acc, l[0], l[1], l[2], l[3], l[4]);
    } else if (!strcmp(what, "lt")) {
      unsigned c; if (scanf("%u", &c) != 1 || c < 1 || c > 64) return 2;
      unsigned lt[64], eq[64];
      for (unsigned i = 0; i < c; i++) if (scanf("%u %u", &lt[i], &eq[i]) != 2) return 2;
      uint64_t g = lt[c - 1];
      for (unsigned m = c - 1; m-- > 0;) g = values_lt_step(lt[m], eq[m], g);
      printf("%llu\n", (unsigned long long)g);
    } else return 2;
  }
  return 0;
}
