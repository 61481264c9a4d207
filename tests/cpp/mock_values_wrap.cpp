// Fragment of tests/cpp/mock_device.cpp (-DMOCK_EXT_VALUES; requires custom, for custom_g): the entry point of include/lasso_hip_values.h as a literal statement over the
// oracle's field type: per lookup the NUM_MEMORIES table entries, then combine_lookups as subtables/*.rs state it.
#include "../../include/lasso_hip_values.h"
#include "../../lasso_amd/csrc/values_combine.cuh"   // the refusal's rule and text only; the arithmetic below is the mock's own

extern "C" int32_t lasso_lookup_values(lasso_ctx* c, const lasso_strategy* s, const uint32_t* const* d_dim, const uint32_t* const* tu32, const lasso_fr* const* tfr, size_t n, int32_t form, void* d_out) {
  REQ(c, s && d_dim && d_out && (form == LASSO_VALUES_FR || form == LASSO_VALUES_U64) && (tu32 != nullptr) != (tfr != nullptr));
  const bool custom = s->kind == LASSO_CUSTOM, spark = s->kind == LASSO_SPARK_UNCONFIRMED, lt = s->kind == LASSO_LT;
  const lasso_strategy_custom* cs = custom ? (const lasso_strategy_custom*)s : nullptr;
  if (custom) { if (const char* why = custom_strategy_check(cs, 0)) return fail(c, why); }
  const size_t C = s->c, nsub = custom ? cs->num_subtables : lt ? 2 : s->kind == LASSO_RANGE ? 3 : spark ? C : 1, alpha = custom ? cs->num_memories : lt ? 2 * C : C;
  REQ(c, custom || (tu32 != nullptr) != spark);
  if (form == LASSO_VALUES_U64 && (custom || spark || !tu32 || !values_u64_offered(s->kind, s->c, s->log_m))) { c->err = "lasso_lookup_values: " VALUES_MSG_U64; return LASSO_ERR_UNSUPPORTED; }
  const size_t inc = s->kind == LASSO_RANGE ? s->log_m : s->log_m / 2;
  std::vector<Fr> v(alpha);
  for (size_t k = 0; k < n; k++) {
    for (size_t i = 0; i < alpha; i++) {
      size_t sub, dim;
      if (custom) { sub = cs->memory_subtable ? cs->memory_subtable[i] : i % nsub; dim = cs->memory_dimension ? cs->memory_dimension[i] : i / nsub; }
      else if (s->kind == LASSO_RANGE) { sub = i * s->log_m > s->log_r ? 2 : (i + 1) * s->log_m > s->log_r ? 1 : 0; dim = i; }
      else { sub = i % nsub; dim = spark ? i : i / nsub; }
      const uint32_t a = d_dim[dim][k];
      REQ(c, ((uint64_t)a >> s->log_m) == 0);
      v[i] = tu32 ? Fr::from_u64(tu32[sub][a]) : F(tfr[sub])[a];
    }
    Fr g = Fr::zero();
    if (custom) g = custom_g(cs, v.data());
    else if (spark) { g = Fr::one(); for (size_t i = 0; i < alpha; i++) g = g * v[i]; }
    else if (lt) { Fr run = Fr::one(); for (size_t i = 0; i < C; i++) { g += v[2 * i] * run; run = run * v[2 * i + 1]; } }
    else for (size_t i = 0; i < alpha; i++) g += Fr::from_u64((uint64_t)1 << (i * inc)) * v[i];
    if (form == LASSO_VALUES_FR) { F((lasso_fr*)d_out)[k] = g; continue; }
    // the 64-bit form: the same sum over the integers (offered only where it fits)
    unsigned __int128 x = 0;
    if (lt) { uint64_t run = 1; for (size_t i = 0; i < C; i++) { x += (uint64_t)tu32[0][d_dim[i][k]] * run; run *= tu32[1][d_dim[i][k]]; } }
    else for (size_t i = 0; i < alpha; i++) {
      const size_t sub = s->kind == LASSO_RANGE ? (i * s->log_m > s->log_r ? 2 : (i + 1) * s->log_m > s->log_r ? 1 : 0) : 0;
      x += (unsigned __int128)tu32[sub][d_dim[i][k]] << (i * inc);
    }
    ((uint64_t*)d_out)[k] = (uint64_t)x;
  }
  return 0;
}
