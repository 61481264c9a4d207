// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_CUSTOM), which compiles the mock's lasso_sumcheck_combine_round and lasso_combine_claim — the two entry points that take a
// strategy on a caller-defined strategy's path — as mock_builtin_*: here they are wrapped.  For kind = LASSO_CUSTOM a literal loop over the descriptor's term list
// (sumcheck.rs:179-218 and subtables/mod.rs:197-213 with comb_func = the caller's g), everything else forwarded to the mock.
#include "../../include/lasso_custom_check.h"

static Fr custom_g(const lasso_strategy_custom* s, const Fr* v) {
  Fr sum = Fr::zero();
  for (uint32_t t = 0; t < s->num_terms; t++) {
    Fr term = *F(s->coeff + t);
    for (uint32_t j = s->term_start[t]; j < s->term_start[t + 1]; j++) term = term * v[s->term_mem[j]];
    sum += term;
  }
  return sum;
}

extern "C" {
int32_t lasso_sumcheck_combine_round(lasso_ctx* c, const lasso_strategy* s, const lasso_fr* const* polys, const lasso_fr* eq, size_t n, uint32_t degree, lasso_fr* out) {
  if (!s || s->kind != LASSO_CUSTOM) return mock_builtin_combine_round(c, s, polys, eq, n, degree, out);
  const lasso_strategy_custom* cs = (const lasso_strategy_custom*)s;
  if (const char* why = custom_strategy_check(cs, 0)) return fail(c, why);
  REQ(c, polys && eq && out && n >= 2 && (n & (n - 1)) == 0 && degree == custom_strategy_degree(cs) + 1);
  const size_t alpha = cs->num_memories, half = n / 2;
  std::vector<Fr> ev(degree + 1, Fr::zero()), lo(alpha + 1), hi(alpha + 1), cur(alpha + 1);
  for (size_t i = 0; i < half; i++) {
    for (size_t j = 0; j < alpha; j++) { lo[j] = F(polys[j])[i]; hi[j] = F(polys[j])[half + i]; }
    lo[alpha] = F(eq)[i]; hi[alpha] = F(eq)[half + i];
    ev[0] += lo[alpha] * custom_g(cs, lo.data()); ev[1] += hi[alpha] * custom_g(cs, hi.data());
    cur = hi;
    for (uint32_t k = 2; k <= degree; k++) { for (size_t j = 0; j <= alpha; j++) cur[j] = cur[j] + hi[j] - lo[j]; ev[k] += cur[alpha] * custom_g(cs, cur.data()); }
  }
  memcpy(out, ev.data(), ev.size() * 32); return 0;
}
int32_t lasso_combine_claim(lasso_ctx* c, const lasso_strategy* s, const lasso_fr* const* polys, const lasso_fr* eq, size_t n, lasso_fr* out) {
  if (!s || s->kind != LASSO_CUSTOM) return mock_builtin_combine_claim(c, s, polys, eq, n, out);
  const lasso_strategy_custom* cs = (const lasso_strategy_custom*)s;
  if (const char* why = custom_strategy_check(cs, 0)) return fail(c, why);
  REQ(c, polys && eq && n >= 1);
  const size_t alpha = cs->num_memories; std::vector<Fr> v(alpha); Fr claim = Fr::zero();
  for (size_t k = 0; k < n; k++) { for (size_t j = 0; j < alpha; j++) v[j] = F(polys[j])[k]; claim += F(eq)[k] * custom_g(cs, v.data()); }
  if (c->defer) { c->defer = false; c->pending.assign(1, claim); return 0; }   // lasso_defer_next, as the mock's
  REQ(c, out);
  *F(out) = claim; return 0;
}
}
