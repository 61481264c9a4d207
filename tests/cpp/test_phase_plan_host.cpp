// lasso_amd/host/sumcheck_phase.hpp: the plan of an eq-weighted sumcheck phase.  The pure planning functions (tail_from, host_m_stop, host_handover) against a literal
// restatement of the loops linear_rounds / cubic_rounds carried before the plan existed, at the shapes where they can go wrong: zero to three rounds, arrays of 2 and 4 elements,
// the resident kernel's capacity met exactly and exceeded by one step, a zero coordinate exactly at the tail's first round and one before it, 1 .. 33 circuits against the
// host's budgets.  And EqPhase itself: inv[j] * prod_{t<=j}(1 - point[v0+t]) == 1 on a random point, `degenerate` when a coordinate equals 1, the per-round scalars.
#include <cstdio>
#include <cstring>
#include "../../lasso_amd/host/sumcheck_phase.hpp"
using namespace lasso;
static uint64_t st = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { st ^= st << 13; st ^= st >> 7; st ^= st << 17; return st; }
static Sc canon_rand() { Sc s; for (;;) { uint64_t l[4] = {rnd(), rnd(), rnd(), rnd() >> 3}; memcpy(s.v.v, l, 32); if (!fr_geq_p(s.v.v)) return s; } }
static size_t ceil_log2(size_t n) { size_t k = 0; while (((size_t)1 << k) < n) k++; return k; }

// ---- the loops as the two drivers had them (cubic: with the "no zero coordinate in the tail" condition)
static size_t old_tail_from(size_t rounds, size_t len, size_t tail_q, bool eligible, bool cubic, const ScVec& rand, size_t v0) {
  size_t tail_from = rounds;
  if (eligible) {
    size_t j0 = 0; size_t l = len;
    while (j0 < rounds && (j0 == 0 ? l / 2 : l / 4) > tail_q) { if (j0) l /= 2; j0++; }
    bool plain = j0 < rounds;
    if (cubic) for (size_t j = j0; j < rounds && plain; j++) if (rand[v0 + j].is_zero()) plain = false;
    if (plain) tail_from = j0;
  }
  return tail_from;
}
static size_t old_host_m_stop(size_t k, size_t budget) {
  if (!budget || !k) return 1;
  size_t m0 = 1; while (2 * m0 * k <= budget && 2 * m0 <= 64) m0 *= 2;
  return m0;
}
static void old_handover(size_t rounds, size_t len, size_t tail_from, size_t k, size_t budget, size_t& m_stop, size_t& j_host) {
  m_stop = 1; j_host = rounds;
  if (tail_from < rounds && len == ((size_t)1 << rounds)) {
    const size_t m0 = old_host_m_stop(k, budget), lt = len >> tail_from;
    if (m0 >= 2 && m0 < lt) { m_stop = m0; j_host = rounds - ceil_log2(m0); }
  }
}

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

int main() {
  // ---- tail_from
  for (size_t q : {1, 2, 4, 256}) {
    const size_t lens[] = {2, 4, 2 * q, 2 * q + 2, 4 * q, 4 * q + 4, 8 * q, 32 * q};   // len / 2 == q, len / 4 == q, one step above each, and further out
    for (size_t len : lens) for (size_t rounds = 0; rounds <= 7 && ((size_t)1 << rounds) <= len; rounds++) for (size_t v0 : {0, 2}) {
      ScVec rand(v0 + rounds); for (auto& x : rand) { x = canon_rand(); if (x.is_zero()) x = Sc::one(); }
      const EqPhase ph(rand, v0, rounds);
      auto cubic = [&](size_t j0) { return ph.no_zero_from(j0); };
      auto linear = [](size_t) { return true; };
      const size_t j0 = old_tail_from(rounds, len, q, true, true, rand, v0);   // no zero coordinate yet
      CHECK(tail_from(rounds, len, q, true, cubic) == j0 && tail_from(rounds, len, q, true, linear) == j0);
      CHECK(tail_from(rounds, len, q, false, cubic) == rounds && tail_from(rounds, len, q, false, linear) == rounds);
      if (rounds) CHECK(j0 == rounds || (j0 == 0 ? len / 2 : (len >> (j0 - 1)) / 4) <= q);                // the tail's first round fits the kernel ...
      if (j0 && j0 < rounds) CHECK((j0 == 1 ? len / 2 : (len >> (j0 - 2)) / 4) > q);                      // ... and the round before it did not
      for (size_t z = 0; z < rounds; z++) {   // one zero coordinate at every position: exactly at the tail's first round, before it, after it
        ScVec r2 = rand; r2[v0 + z] = Sc::zero();
        const EqPhase p2(r2, v0, rounds);
        const size_t got = tail_from(rounds, len, q, true, [&](size_t a) { return p2.no_zero_from(a); });
        CHECK(got == old_tail_from(rounds, len, q, true, true, r2, v0));
        CHECK(got == (z >= j0 ? rounds : j0));                                                             // at or after tail_from: no tail; before it: unchanged
        CHECK(tail_from(rounds, len, q, true, linear) == old_tail_from(rounds, len, q, true, false, r2, v0));
      }
      // ---- m_stop / j_host for every first tail round the phase could have
      for (size_t k : {0, 1, 2, 16, 33}) for (size_t budget : {0, 4, 32, 128, 512, 1024}) {
        CHECK(host_m_stop(k, budget) == old_host_m_stop(k, budget));
        for (size_t tf = 0; tf <= rounds; tf++) {
          size_t m_stop, j_host; old_handover(rounds, len, tf, k, budget, m_stop, j_host);
          const HostHandover ho = host_handover(rounds, len, tf, host_m_stop(k, budget));
          CHECK(ho.m_stop == m_stop && ho.j_host == j_host);
          CHECK(ho.j_host <= rounds && (ho.m_stop == 1 ? ho.j_host == rounds : ((size_t)1 << (rounds - ho.j_host)) == ho.m_stop && ho.j_host > tf));
        }
      }
    }
  }
  CHECK(host_m_stop(1, 32) == 32 && host_m_stop(2, 32) == 16 && host_m_stop(16, 32) == 2 && host_m_stop(33, 32) == 1 && host_m_stop(33, 128) == 2 && host_m_stop(33, 512) == 8 && host_m_stop(1, 512) == 64 && host_m_stop(2, 4) == 2 && host_m_stop(16, 4) == 1);

  // ---- EqPhase
  for (int it = 0; it < 50; it++) {
    const size_t v0 = it % 3, rounds = 1 + it % 6;
    ScVec point(v0 + rounds + 1); for (auto& x : point) x = canon_rand();
    const EqPhase ph(point, v0, rounds);
    CHECK(!ph.degenerate && ph.inv.size() == rounds);
    Sc prod = Sc::one(), s_run = canon_rand();
    for (size_t j = 0; j < rounds; j++) {
      const Sc rj = point[v0 + j], om = Sc::one() - rj;
      prod *= om;
      CHECK(ph.inv[j] * prod == Sc::one());
      CHECK(ph.om(j) == om && ph.r(j) == rj);
      const Sc base = s_run * ph.inv[j];   // the drivers' scalars as they computed them
      CHECK(ph.base(j, s_run) == base && ph.f0(j, base) == base * om && ph.f1(j, base) == base * rj);
      CHECK(ph.f2(j, base) == base * (rj + rj - om) && ph.f3(j, base) == base * (rj + rj + rj - om - om));
      const Sc r_j = canon_rand(), next = s_run * (om * (Sc::one() - r_j) + rj * r_j);
      ph.advance(s_run, j, r_j);
      CHECK(s_run == next);
    }
    ScVec one = point; one[v0 + it % rounds] = Sc::one();   // a coordinate equal to 1: no inverse, scale 1
    const EqPhase pd(one, v0, rounds);
    CHECK(pd.degenerate && pd.base(0, s_run) == s_run);
    ScVec outside = point; outside[v0 + rounds] = Sc::one(); if (v0) outside[0] = Sc::one();   // ... but only inside the phase's own coordinates
    CHECK(!EqPhase(outside, v0, rounds).degenerate);
    ScVec zero = point; zero[v0 + rounds - 1] = Sc::zero();
    CHECK(!EqPhase(zero, v0, rounds).degenerate && !EqPhase(zero, v0, rounds).no_zero_from(0) && EqPhase(zero, v0, rounds).no_zero_from(rounds));
  }
  CHECK(EqPhase(ScVec(), 0, 0).inv.empty() && !EqPhase(ScVec(), 0, 0).degenerate);
  printf("OK %ld checks\n", checks);
  return 0;
}
