// How an operand pair becomes the C table addresses of one lookup (include/lasso_hip_operands.h lasso_operand_layout) — written ONCE: k_densify_extract_operands
// (densify_kernels.cuh), the host library (lasso_host_operand_indices, the fallback of lasso_host_densify_operands) and a stand-alone host program
// (tests/cpp/test_operand_layout_host.cpp, against Python big integers) compile this text.
//   j        = msb_first ? C - 1 - dim : dim
//   chunk(v) = (j b >= 64) ? 0 : (v >> (j b)) & (2^b - 1)
//   index    = operands == 2 ? (chunk(x) << b) | chunk(y) : chunk(x)
//   v fits   when C b >= 64 or v < 2^(C b)
// The j b >= 64 branch is not cosmetic: RangeCheck at C = 5, log_m = 16 shifts by 64, and a 64-bit shift takes the low six bits of its count (gfx950's v_lshrrev_b64 and
// x86's shr alike; undefined in C), so the unguarded form returns v itself.
#pragma once
#include <stddef.h>
#include <stdint.h>
#include "../../include/lasso_hip_operands.h"

#ifndef LHD
#if defined(__HIPCC__)
#define LHD __host__ __device__ __forceinline__
#else
#define LHD inline
#endif
#endif

// What makes a layout unusable for C dimensions of 2^log_m addresses; 0 = well formed.  One list for the device entry, the host entry and the fallback, so that a
// refusal reads the same whichever path would have run.
enum { OPL_OK = 0, OPL_NULL = 1, OPL_OPERANDS = 2, OPL_MSB = 3, OPL_BITS = 4, OPL_LOG_M = 5 };
LHD int operand_layout_check(const lasso_operand_layout* L, size_t C, size_t log_m) {
  if (!L || C < 1) return OPL_NULL;
  if (L->operands != 1u && L->operands != 2u) return OPL_OPERANDS;
  if (L->msb_first > 1u) return OPL_MSB;
  if (log_m > 32) return OPL_LOG_M;
  if (L->chunk_bits < 1u || (uint64_t)L->operands * L->chunk_bits > log_m) return OPL_BITS;
  return OPL_OK;
}
inline const char* operand_layout_error(int code) {
  switch (code) {
    case OPL_NULL: return "operand layout: null layout, or no dimension";
    case OPL_OPERANDS: return "operand layout: operands must be 1 or 2";
    case OPL_MSB: return "operand layout: msb_first must be 0 or 1";
    case OPL_BITS: return "operand layout: chunk_bits must be at least 1 and operands * chunk_bits at most log_m";
    case OPL_LOG_M: return "operand layout: log_m must be at most 32";
    default: return "";
  }
}
#define OPL_MSG_FIT "an operand does not fit C * chunk_bits bits (lasso_operand_layout)"
#define OPL_MSG_Y "the second operand column must be given exactly when the layout has two operands"

// chunk j (counted from the least significant end) of v, b bits wide; b <= 32 (operand_layout_check)
LHD uint64_t operand_chunk(uint64_t v, uint64_t j, uint32_t b) {
  const uint64_t sh = j * b;
  return sh >= 64 ? 0 : (v >> sh) & (((uint64_t)1 << b) - 1);
}
// the address dimension `dim` of C reads for the operands (x, y); y is ignored when the layout has one operand.  Below 2^(operands * chunk_bits) <= 2^log_m by construction.
LHD uint64_t operand_index(const lasso_operand_layout& L, uint64_t x, uint64_t y, size_t C, size_t dim) {
  const uint64_t j = L.msb_first ? C - 1 - dim : dim;
  const uint64_t cx = operand_chunk(x, j, L.chunk_bits);
  return L.operands == 2u ? (cx << L.chunk_bits) | operand_chunk(y, j, L.chunk_bits) : cx;
}
// whether the C chunks of b bits hold all of v (otherwise the lookup would silently be one of v mod 2^(C b))
LHD bool operand_fits(uint64_t v, size_t C, uint32_t b) {
  const uint64_t bits = (uint64_t)C * b;
  return bits >= 64 || (v >> bits) == 0;
}
