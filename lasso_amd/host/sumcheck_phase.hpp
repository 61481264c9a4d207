// The plan of one eq-weighted sumcheck phase (prover.hpp linear_rounds / cubic_rounds): `rounds` rounds over point[v0 .. v0+rounds) on arrays of `len` elements.  The eq
// polynomial is never bound: after j binds it is  s_run * eq1(point_j, x) * T_j  with T_j the prefix of the phase's table times 1 / prod_{t<=j}(1 - point[v0+t]), so a round
// needs the scalars below and nothing else.  Plain C++ on field_host.hpp types: no device call (tests/cpp/test_phase_plan_host.cpp).
#pragma once
#include "field_host.hpp"

namespace lasso {
struct EqPhase {
  const ScVec& point; const size_t v0, rounds;
  ScVec inv;                 // inv[j] = 1 / prod_{t<=j}(1 - point[v0+t]), one inversion for the phase
  bool degenerate = false;   // a coordinate equals 1: no inverse, the rounds read an explicit table T_j instead (Prover::degenerate_table) and the scale is 1
  EqPhase(const ScVec& point_, size_t v0_, size_t rounds_) : point(point_), v0(v0_), rounds(rounds_), inv(rounds_) {
    Sc prod = Sc::one();
    for (size_t j = 0; j < rounds; j++) { Sc o = om(j); if (o.is_zero()) degenerate = true; prod *= o; }
    if (!degenerate) { Sc pi = prod.inverse(); for (size_t j = rounds; j-- > 0;) { inv[j] = pi; pi *= om(j); } }
  }
  const Sc& r(size_t j) const { return point[v0 + j]; }
  Sc om(size_t j) const { return Sc::one() - r(j); }
  bool no_zero_from(size_t j0) const { for (size_t j = j0; j < rounds; j++) if (r(j).is_zero()) return false; return true; }
  // round j's factor f(x) = s_run * scale_j * eq1(point_j, x), eq1(r, x) = (1 - r)(1 - x) + r x: linear in x, given by its values at 0..3
  Sc base(size_t j, const Sc& s_run) const { return s_run * (degenerate ? Sc::one() : inv[j]); }
  Sc f0(size_t j, const Sc& base_j) const { return base_j * om(j); }
  Sc f1(size_t j, const Sc& base_j) const { return base_j * r(j); }
  Sc f2(size_t j, const Sc& base_j) const { return base_j * (r(j) + r(j) - om(j)); }
  Sc f3(size_t j, const Sc& base_j) const { return base_j * (r(j) + r(j) + r(j) - om(j) - om(j)); }
  void advance(Sc& s_run, size_t j, const Sc& r_j) const { s_run *= om(j) * (Sc::one() - r_j) + r(j) * r_j; }   // eq1(point_j, r_j)
};

// First round served by the resident tail kernel (== rounds: none).  The kernel holds tail_q indices per array: round 0 reads len / 2 of them, a later round j binds first and
// reads a quarter of the length before its bind.  eligible: the caller's conditions (heads wanted, no collective between rounds, not degenerate, not switched off);
// no_zero_from(j0): no coordinate of [j0, rounds) may be 0 (the cubic rounds' condition; the linear rounds pass "always").
template <class NoZeroFrom> inline size_t tail_from(size_t rounds, size_t len, size_t tail_q, bool eligible, NoZeroFrom no_zero_from) {
  if (!eligible) return rounds;
  size_t j0 = 0, l = len;   // l = array length before round j0's bind
  while (j0 < rounds && (j0 == 0 ? l / 2 : l / 4) > tail_q) { if (j0) l /= 2; j0++; }
  return j0 < rounds && no_zero_from(j0) ? j0 : rounds;
}
// Elements per array at which the host takes a layer of k circuits over: a power of two within the budget (elements x circuits) and at most 64; 1 = never.
inline size_t host_m_stop(size_t k, size_t budget) {
  size_t m0 = 1; if (budget && k) while (2 * m0 * k <= budget && 2 * m0 <= 64) m0 *= 2;
  return m0;
}
// The resident tail runs the rounds [tail_from, j_host) and hands arrays of m_stop elements to the host, which runs [j_host, rounds): only for a whole layer
// (len == 2^rounds) whose arrays are still longer than m0 = host_m_stop(k, budget) when the tail begins.
struct HostHandover { size_t m_stop, j_host; };
inline HostHandover host_handover(size_t rounds, size_t len, size_t tail_from, size_t m0) {
  if (tail_from < rounds && len == ((size_t)1 << rounds) && m0 >= 2 && m0 < (len >> tail_from)) { size_t lg = 0; while (((size_t)1 << lg) < m0) lg++; return {m0, rounds - lg}; }
  return {1, rounds};
}
}  // namespace lasso
