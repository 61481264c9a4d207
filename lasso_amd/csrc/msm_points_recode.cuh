// Signed window digits of a 256-bit integer — the recoding of the table-free MSM (msm_points_kernels.cuh), host and device, so that the CPU tests
// can hold it against big integers (tests/cpp/test_msm_points_recode_host.cpp).
//   k = sum_w d_w 2^(c w),   d_w in [-2^(c-1), 2^(c-1) - 1],   w = 0 .. MSMP_WINDOWS(c) - 1
// Window w takes its c bits plus the carry of the window below; a value >= 2^(c-1) becomes value - 2^c with a carry into the next window.  Exact for EVERY
// k < 2^256, canonical or not: the windows cover at least 257 bits, so the last one holds at most the carry (0 or 1 < 2^(c-1)) and nothing leaves it.
#pragma once
#include <stdint.h>
#include "fr.cuh"   // LHD

#define MSMP_WINDOWS(c) ((256u + (c)) / (c))   // the smallest number of c-bit windows that covers 257 bits
#define MSMP_C 8u                              // the window width the kernels are built with: digits in [-128, 127]
#define MSMP_NW MSMP_WINDOWS(MSMP_C)           // 33

// bits [bit, bit + c) of the little-endian integer s[0..8); bits from 256 on are zero.  c <= 16
LHD uint32_t msmp_bits(const uint32_t* s, uint32_t bit, uint32_t c) {
  if (bit >= 256u) return 0u;
  const uint32_t word = bit >> 5, sh = bit & 31u;
  uint64_t v = s[word]; if (word < 7u) v |= (uint64_t)s[word + 1] << 32;
  return (uint32_t)(v >> sh) & ((1u << c) - 1u);
}
// digit of window w given the carry out of window w - 1 (0 for w = 0); leaves the carry into window w + 1 in `carry`
LHD int32_t msmp_digit(const uint32_t* s, uint32_t c, uint32_t w, uint32_t& carry) {
  const uint32_t raw = msmp_bits(s, c * w, c) + carry;   // 0 .. 2^c
  carry = raw >= (1u << (c - 1u)) ? 1u : 0u;
  return (int32_t)raw - (int32_t)(carry << c);
}
