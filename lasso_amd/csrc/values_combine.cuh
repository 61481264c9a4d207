// The integer side of lasso_lookup_values (include/lasso_hip_values.h, values_kernels.cuh), host and device: combine_lookups of the kinds whose subtables hold small
// integers, in integer arithmetic, and the rule that says when the result fits 64 bits.  Plain C++ beside the LHD marker, so that a stand-alone program holds these lines to
// Python integers (tests/cpp/test_values_combine_host.cpp, plain and under -fsanitize=undefined) and the host prover states the same rule with the same words.
//
//   AND / OR / XOR (and.rs:45-53), RangeCheck (range_check.rs:78-86):  g = sum_i 2^(i * inc) * v_i,  inc = log_m / 2 (RangeCheck: log_m),  i < NUM_MEMORIES = C.
//       The reference forms the weight as `1u64 << (i * inc)`: (C - 1) * inc < 64 is required everywhere in this project (make_strategy, Strategy::weights).  An entry is below
//       2^32, so a term is below 2^95 and a sum of up to 32 of them below 2^100: the sum runs in 128 bits and never wraps, whatever the tables hold.
//   LT (lt.rs:62-71):  g = sum_i LT_i * prod_{j < i} EQ_j  =  LT_0 + EQ_0 (LT_1 + EQ_1 (... + EQ_{C-2} LT_{C-1}))  (the Horner form of k_combine_claim), one step per chunk from
//       the last chunk to the first.  The LT / EQ subtables hold bits and at most one of LT_i, EQ_i is set for an address, so g stays 0 or 1; the step is plain 64-bit arithmetic.
#pragma once
#include <stdint.h>
#include "../../include/lasso_hip.h"

#ifndef LHD
#if defined(__HIPCC__)
#define LHD __host__ __device__ __forceinline__
#else
#define LHD inline
#endif
#endif

typedef unsigned __int128 values_u128;

// one text for the refusal of the 64-bit form, whichever library states it
#define VALUES_MSG_U64 "the 64-bit form is offered over integer tables for LT, and for AND / OR / XOR / RangeCheck when sum_i 2^(i * inc) * max_table_value is below 2^64; every other strategy has the field form only"

// kinds whose combine is the weighted sum above / the LT walk
LHD bool values_kind_linear(int32_t kind) { return kind == LASSO_AND || kind == LASSO_OR || kind == LASSO_XOR || kind == LASSO_RANGE; }
LHD uint32_t values_inc(int32_t kind, uint32_t log_m) { return kind == LASSO_RANGE ? log_m : log_m / 2; }
// the largest entry of any subtable of a built-in integer kind (Strategy::max_table_value): l op r < 2^(log_m / 2); LT / EQ are bits; range tables hold addresses
LHD uint32_t values_max_entry(int32_t kind, uint32_t log_m) {
  if (kind == LASSO_LT) return 1u;
  if (kind == LASSO_RANGE) return log_m >= 32 ? 0xffffffffu : (uint32_t)(((uint64_t)1 << log_m) - 1);
  return (uint32_t)(((uint64_t)1 << (log_m / 2)) - 1);
}
// sum_i 2^(i * inc) * max_entry over alpha memories ((alpha - 1) * inc < 64, alpha <= 32: below 2^100)
LHD values_u128 values_linear_bound(uint32_t alpha, uint32_t inc, uint32_t max_entry) {
  values_u128 b = 0;
  for (uint32_t i = 0; i < alpha; i++) b += (values_u128)max_entry << (i * inc);
  return b;
}
// is LASSO_VALUES_U64 offered for this built-in kind and shape?  (Spark and caller-defined strategies: never — the caller of this function has sent them away already)
LHD bool values_u64_offered(int32_t kind, uint32_t c, uint32_t log_m) {
  if (kind == LASSO_LT) return true;
  if (!values_kind_linear(kind)) return false;
  return (values_linear_bound(c, values_inc(kind, log_m), values_max_entry(kind, log_m)) >> 64) == 0;
}
// one memory of the weighted sum
LHD void values_linear_add(values_u128& acc, uint32_t entry, uint32_t shift) { acc += (values_u128)entry << shift; }
// one chunk of the LT walk: g <- LT_m + EQ_m g
LHD uint64_t values_lt_step(uint32_t lt, uint32_t eq, uint64_t g) { return (uint64_t)lt + (uint64_t)eq * g; }
// a value below 2^128 as five 29-bit limbs (the integer operand of fr29_mul(x, R2S): the one conversion into memory form)
LHD void values_limbs(values_u128 v, int32_t* l) {
  for (int k = 0; k < 4; k++) { l[k] = (int32_t)((uint32_t)v & 0x1fffffffu); v >>= 29; }
  l[4] = (int32_t)(uint32_t)v;   // 128 - 116 = 12 bits
}
