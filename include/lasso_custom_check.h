/* lasso_custom_check.h — the one validation of a caller-defined strategy (include/lasso_hip.h lasso_strategy_custom), shared by the device library
 * (lasso_sumcheck_combine_round, lasso_combine_claim: need_tables = 0, they never read the tables) and the host prover / verifier (need_tables = 1).
 * Returns NULL when the descriptor is well formed, otherwise the reason as a static string.  Header-only: no symbol is added to either library's C ABI. */
#ifndef LASSO_CUSTOM_CHECK_H
#define LASSO_CUSTOM_CHECK_H
#include "lasso_hip.h"

static inline const char* custom_strategy_check(const lasso_strategy_custom* s, int need_tables) {
  if (!s) return "custom strategy: null descriptor";
  if (s->base.kind != LASSO_CUSTOM) return "custom strategy: kind is not LASSO_CUSTOM";
  if (s->base.c < 1) return "custom strategy: c must be at least 1";
  if (s->base.log_m < 1 || s->base.log_m > 30) return "custom strategy: log_m must be in 1..30";
  if (s->num_memories < 1 || s->num_memories > 32) return "custom strategy: num_memories must be in 1..32 (LASSO_MAX_ALPHA)";
  if (s->num_subtables < 1 || s->num_subtables > 32) return "custom strategy: num_subtables must be in 1..32";
  if (need_tables) {
    if ((s->tables_u32 != 0) == (s->tables_fr != 0)) return "custom strategy: exactly one of tables_u32 / tables_fr must be given";
    for (uint32_t i = 0; i < s->num_subtables; i++)
      if (s->tables_u32 ? !s->tables_u32[i] : !s->tables_fr[i]) return "custom strategy: a table pointer is null";
  }
  if ((s->memory_subtable != 0) != (s->memory_dimension != 0)) return "custom strategy: memory_subtable and memory_dimension are given together or not at all";
  if (s->memory_subtable) {
    for (uint32_t i = 0; i < s->num_memories; i++) {
      if (s->memory_subtable[i] >= s->num_subtables) return "custom strategy: memory_subtable index out of range";
      if (s->memory_dimension[i] >= s->base.c) return "custom strategy: memory_dimension index out of range";
    }
  } else if ((s->num_memories + s->num_subtables - 1) / s->num_subtables > s->base.c) return "custom strategy: the default memory map (i / num_subtables) needs num_memories <= c * num_subtables";
  if (s->num_terms < 1 || s->num_terms > LASSO_CUSTOM_MAX_TERMS) return "custom strategy: num_terms must be in 1..256 (LASSO_CUSTOM_MAX_TERMS)";
  if (!s->coeff || !s->term_start) return "custom strategy: coeff / term_start is null";
  if (s->term_start[0] != 0) return "custom strategy: term_start[0] must be 0";
  for (uint32_t t = 0; t < s->num_terms; t++) {
    if (s->term_start[t + 1] < s->term_start[t]) return "custom strategy: term_start is not monotone";
    if (s->term_start[t + 1] > LASSO_CUSTOM_MAX_FACTORS) return "custom strategy: more than 2048 factor entries (LASSO_CUSTOM_MAX_FACTORS)";
    if (s->term_start[t + 1] - s->term_start[t] + 1 > LASSO_CUSTOM_MAX_DEGREE) return "custom strategy: a term has more than 16 factors (sumcheck degree over 17)";
  }
  if (s->term_start[s->num_terms] > 0 && !s->term_mem) return "custom strategy: term_mem is null";
  for (uint32_t j = 0; j < s->term_start[s->num_terms]; j++)
    if (s->term_mem[j] >= s->num_memories) return "custom strategy: term_mem index out of range";
  return 0;
}
/* g_poly_degree: the longest term */
static inline uint32_t custom_strategy_degree(const lasso_strategy_custom* s) {
  uint32_t d = 0;
  for (uint32_t t = 0; t < s->num_terms; t++) { const uint32_t l = s->term_start[t + 1] - s->term_start[t]; if (l > d) d = l; }
  return d;
}
#endif
