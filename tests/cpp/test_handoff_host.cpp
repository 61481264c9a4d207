// CPU check of the hand-off protocol between the kernels and the host, from the product's own headers.  The two encodings: the DEVICE side's result_store /
// result_check / mail_valid (lasso_amd/csrc/handoff_device.cuh, compiled for the host with clang for ext_vector_type, under the shims below) and the HOST side's tagged_element /
// mail_chunks (handoff.cuh) played against each other: what one side writes the other accepts, and a stale, torn or corrupted chunk is refused.  The state machine: every sequence
// of transitions the prover uses, step by step, with the values the entry points of lasso_hip.hip leave behind.
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <emmintrin.h>
#include "../../lasso_amd/csrc/fr.cuh"
#define __device__
#define __forceinline__ inline
#define __restrict__
// round 6: result_store's partials path (flag == nullptr) uses write-through 8-byte stores on the device; on the host they are plain stores of the same bytes
#define __HIP_MEMORY_SCOPE_AGENT 0
#define __hip_atomic_store(ptr, val, order, scope) (*(ptr) = (val))
#include "../../lasso_amd/csrc/handoff_device.cuh"
#define CHECK(c) do { if (!(c)) { printf("FAIL %s line %d\n", #c, __LINE__); return 1; } } while (0)
static bool is(const Handoff& h, uint32_t seq, size_t count, bool tagged, uint32_t groups, uint32_t K) { return h.seq == seq && h.count == count && h.tagged == tagged && h.groups == groups && h.K == K; }
static bool fresh(const HandoffState& p) {
  return p.idle() && !p.waiting_on_device() && p.may_grow() && !p.pending && !p.defer_next && !p.ahead_active && !p.ahead_bullet && !p.lay_active && !p.lay_tail && !p.tail_active &&
         !p.tail_unstarted && !p.handover_next && !p.no_grow && !p.gate_sent && p.result.groups == 1 && p.result.K == 0;
}
// the states the prover can stop in (an exception between two entry points): lasso_abort's reset must leave every one of them idle
static void s_pending(HandoffState& p) { p.park(Handoff{5, 4, true, 3, 2}); }
static void s_deferred(HandoffState& p) { p.defer_next = true; }
static void s_round_ahead(HandoffState& p) { s_pending(p); p.arm_ahead(Handoff{6, 4, true, 3, 2}, false); }
static void s_bullet_ahead(HandoffState& p) { p.arm_ahead(Handoff{7, 8, true}, true); }
static void s_tail(HandoffState& p) { p.begin_tail(Handoff{20, 6, true}, 3, 24, false); }
static void s_tail_unstarted(HandoffState& p) { s_pending(p); p.begin_tail(Handoff{30, 6, false}, 2, 6, true); }
static void s_layer(HandoffState& p) { s_tail(p); p.gate_sent = 40; p.arm_layer(Handoff{40, 4, true, 2, 2}, 7); }
static void s_layer_tail(HandoffState& p) { s_tail(p); p.gate_sent = 50; p.arm_layer_tail(Handoff{50, 4, true}, 2, 3, 4); }
static void s_posted(HandoffState& p) { s_round_ahead(p); p.collect(); p.post_ahead(); }
static void s_no_grow(HandoffState& p) { s_tail(p); p.no_grow = true; }

static int state_machine() {
  { HandoffState p; CHECK(fresh(p)); }
  {   // plain begin -> collect (lasso_sumcheck_cubic_eqw2_begin, lasso_result_wait)
    HandoffState p; s_pending(p);
    CHECK(p.pending && !p.idle() && !p.waiting_on_device() && p.may_grow() && is(p.result, 5, 4, true, 3, 2));
    const Handoff h = p.collect(); CHECK(is(h, 5, 4, true, 3, 2) && !p.pending && p.idle());
  }
  {   // deferred call -> collect (lasso_defer_next, then an entry point that ends in wait_flag)
    HandoffState p;
    CHECK(!p.park_deferred(Handoff{8, 3, true}) && fresh(p));            // not armed: the caller waits for the result itself
    s_deferred(p); CHECK(p.idle() && p.defer_next);
    CHECK(p.park_deferred(Handoff{8, 12, false, 4, 3}) && !p.defer_next && p.pending && is(p.result, 8, 12, false, 4, 3));
    CHECK(!p.park_deferred(Handoff{9, 1, true}) && is(p.result, 8, 12, false, 4, 3));   // one-shot
    CHECK(is(p.collect(), 8, 12, false, 4, 3) && p.idle());
  }
  {   // round ahead -> challenge post -> collect, enqueued while the previous round's result is pending; then bullet ahead -> bullet post -> collect
    HandoffState p; s_round_ahead(p);
    CHECK(p.ahead_active && !p.ahead_bullet && p.pending && p.waiting_on_device() && !p.may_grow() && !p.idle() && is(p.ahead, 6, 4, true, 3, 2) && is(p.result, 5, 4, true, 3, 2));
    CHECK(is(p.collect(), 5, 4, true, 3, 2) && !p.pending && p.ahead_active && !p.idle());
    CHECK(p.post_ahead() == 6 && !p.ahead_active && !p.waiting_on_device() && p.may_grow() && p.pending && is(p.result, 6, 4, true, 3, 2));
    CHECK(is(p.collect(), 6, 4, true, 3, 2) && p.idle());
    s_bullet_ahead(p);                                                     // after a round with groups > 1: a bullet round's result is one group, whatever came before
    CHECK(p.ahead_active && p.ahead_bullet && !p.pending && p.waiting_on_device() && is(p.ahead, 7, 8, true, 1, 0));
    CHECK(p.post_ahead() == 7 && !p.ahead_active && p.ahead_bullet && p.pending && is(p.result, 7, 8, true, 1, 0));
    CHECK(is(p.collect(), 7, 8, true, 1, 0) && p.idle());
    p.arm_ahead(Handoff{10, 6, true}, false); CHECK(!p.ahead_bullet);     // the next round ahead is not a bullet round
  }
  for (int form = 0; form < 3; form++) {   // tail begin -> next x turns: heads, hand-over of the arrays (m_stop = 4), nothing after the last challenge
    const uint32_t turns = 3; const size_t fin = form == 0 ? 6 : form == 1 ? 24 : 0;
    HandoffState p; p.handover_next = form == 1 ? 4 : 0;
    CHECK(p.take_handover() == (form == 1 ? 4u : 0u) && p.handover_next == 0 && p.take_handover() == 0);   // one-shot, taken before the begin
    p.begin_tail(Handoff{20, 6, true}, turns, fin, false);
    CHECK(p.tail_active && !p.tail_unstarted && p.pending && !p.idle() && !p.waiting_on_device() && p.may_grow() && is(p.result, 20, 6, true, 1, 0) && p.tail_turn == 0 && p.tail_turns == turns && p.tail_final == fin);
    for (uint32_t t = 1; t <= turns; t++) {
      CHECK(is(p.collect(), 20 + t - 1, 6, true, 1, 0) && !p.pending && p.tail_active);
      CHECK(p.tail_next() == 20 + t && p.tail_turn == t);
      if (t < turns) CHECK(p.tail_active && p.pending && is(p.result, 20 + t, 6, true, 1, 0));
    }
    CHECK(!p.tail_active && p.pending == (fin != 0));                     // the last turn ends the tail; its publication is the heads / the arrays
    if (fin) { CHECK(is(p.result, 20 + turns, fin, true, 1, 0)); CHECK(is(p.collect(), 20 + turns, fin, true, 1, 0)); }
    CHECK(p.idle());
  }
  {   // tail launched ahead of its first challenge, while the previous round's result is pending: the first next starts it
    HandoffState p; s_tail_unstarted(p);
    CHECK(p.tail_active && p.tail_unstarted && p.pending && is(p.result, 5, 4, true, 3, 2) && !p.waiting_on_device());
    CHECK(is(p.collect(), 5, 4, true, 3, 2) && !p.pending);
    CHECK(p.tail_next() == 30 && !p.tail_unstarted && p.tail_turn == 0 && p.tail_active && p.pending && is(p.result, 30, 6, false, 1, 0));   // the flag protocol's tail: tagged as begun
    p.collect(); CHECK(p.tail_next() == 31 && is(p.result, 31, 6, false, 1, 0) && p.tail_active);
    p.collect(); CHECK(p.tail_next() == 32 && is(p.result, 32, 6, false, 1, 0) && !p.tail_active);
    p.collect(); CHECK(p.idle());
  }
  {   // layer ahead, round-0 form, enqueued in the middle of the previous layer's tail -> point post
    HandoffState p; s_layer(p);
    CHECK(p.lay_active && !p.lay_tail && p.lay_ell == 7 && is(p.lay, 40, 4, true, 2, 2) && p.waiting_on_device() && !p.may_grow() && p.tail_active && p.pending && is(p.result, 20, 6, true, 1, 0) && is(p.tail, 20, 6, true, 1, 0));
    for (uint32_t t = 1; t <= 3; t++) { p.collect(); CHECK(p.tail_next() == 20 + t && p.lay_active); }
    CHECK(is(p.collect(), 23, 24, true, 1, 0) && !p.tail_active && !p.pending && p.lay_active && !p.idle());
    p.post_layer();
    CHECK(!p.lay_active && !p.lay_tail && !p.tail_active && p.pending && is(p.result, 40, 4, true, 2, 2) && !p.waiting_on_device() && p.gate_sent == 40);
    p.collect(); CHECK(p.idle());
  }
  {   // layer ahead, tail form -> point post -> tail turns
    HandoffState p; s_layer_tail(p);
    CHECK(p.lay_active && p.lay_tail && p.lay_ell == 2 && p.lay_turns == 3 && p.lay_final == 4 && is(p.lay, 50, 4, true, 1, 0) && is(p.tail, 20, 6, true, 1, 0) && p.tail_turns == 3 && p.tail_final == 24);
    for (uint32_t t = 1; t <= 3; t++) { p.collect(); p.tail_next(); }
    p.collect(); CHECK(!p.tail_active && !p.pending && p.lay_active);
    p.post_layer();
    CHECK(!p.lay_active && !p.lay_tail && p.tail_active && !p.tail_unstarted && is(p.tail, 50, 4, true, 1, 0) && p.tail_turn == 0 && p.tail_turns == 3 && p.tail_final == 4 && p.pending && is(p.result, 50, 4, true, 1, 0));
    for (uint32_t t = 1; t <= 3; t++) { CHECK(is(p.collect(), 50 + t - 1, 4, true, 1, 0)); CHECK(p.tail_next() == 50 + t); }
    CHECK(!p.tail_active && is(p.collect(), 53, 4, true, 1, 0) && p.idle());
  }
  for (int tail_form = 0; tail_form < 2; tail_form++) {   // layer ahead -> cancel: the previous layer's state is untouched
    HandoffState p; if (tail_form) s_layer_tail(p); else s_layer(p);
    p.cancel_layer();
    CHECK(!p.lay_active && !p.lay_tail && !p.waiting_on_device() && p.may_grow() && p.tail_active && is(p.tail, 20, 6, true, 1, 0) && p.tail_final == 24 && p.pending && is(p.result, 20, 6, true, 1, 0));
  }
  {   // a launch enqueued behind a resident kernel: nothing may grow while it is being enqueued
    HandoffState p; s_no_grow(p); CHECK(!p.may_grow() && !p.waiting_on_device()); p.no_grow = false; CHECK(p.may_grow());
  }
  void (*const states[])(HandoffState&) = {s_pending, s_deferred, s_round_ahead, s_bullet_ahead, s_tail, s_tail_unstarted, s_layer, s_layer_tail, s_posted, s_no_grow};
  for (auto make : states) { HandoffState p; make(p); p.handover_next = 8; CHECK(!fresh(p)); p.reset(); CHECK(fresh(p) && p.take_handover() == 0); }
  return 0;
}
int main() {
  if (state_machine()) return 1;
  std::mt19937_64 rng(5);
  alignas(16) uint32_t area[12 * 8]; alignas(16) fr_t plain[8];
  for (int trial = 0; trial < 2000; trial++) {
    const uint32_t seq = (uint32_t)rng() | 1u, slot = (uint32_t)(rng() % 8);
    fr_t v; for (int k = 0; k < 8; k++) v.v[k] = (uint32_t)rng();
    if (trial % 7 == 0) memset(v.v, 0, 32);
    if (trial % 11 == 0) memset(v.v, 0xff, 32);
    memset(area, 0, sizeof(area));
    // device -> device, block partials (flag == nullptr): the element's 32 bytes as they are, at 32 * slot
    result_store(plain, slot, v, (uint32_t*)nullptr, seq);
    CHECK(memcmp(plain[slot].v, v.v, 32) == 0);
    // device -> host, tagged: three chunks at 48 * slot, accepted with exactly the stored words
    result_store(reinterpret_cast<fr_t*>(area), slot, v, LASSO_TAGGED, seq);
    uint32_t w[8];
    CHECK(tagged_element(area + 12 * slot, seq, w) && memcmp(w, v.v, 32) == 0);
    CHECK(!tagged_element(area + 12 * slot, seq + 1, w));                        // another hand-off's number
    CHECK(!tagged_element(area + 12 * ((slot + 1) % 8), seq, w));                // an untouched slot
    for (int c = 0; c < 3; c++) {                                                // one chunk still from an older hand-off
      uint32_t save[4]; memcpy(save, area + 12 * slot + 4 * c, 16);
      area[12 * slot + 4 * c] = seq - 1; CHECK(!tagged_element(area + 12 * slot, seq, w));
      memcpy(area + 12 * slot + 4 * c, save, 16);
    }
    for (int k = 0; k < 12; k++) if (k % 4) {                                    // a flipped bit in any word (the check word included)
      area[12 * slot + k] ^= 1u << (rng() % 32); CHECK(!tagged_element(area + 12 * slot, seq, w)); area[12 * slot + k] = 0; result_store(reinterpret_cast<fr_t*>(area), slot, v, LASSO_TAGGED, seq);
    }
    // the same through the direct-publication sentinel, and the plain path (a flag pointer): out[slot] = v
    memset(area, 0, sizeof(area)); result_store(reinterpret_cast<fr_t*>(area), slot, v, LASSO_TAGGED_DIRECT, seq); CHECK(tagged_element(area + 12 * slot, seq, w) && memcmp(w, v.v, 32) == 0);
    uint32_t flagword = 0; memset(plain, 0, sizeof(plain)); result_store(plain, slot, v, &flagword, seq); CHECK(memcmp(plain[slot].v, v.v, 32) == 0);
    // host -> device: the mailbox
    alignas(16) uint32_t mail[12]; mail_chunks(mail, seq, v.v);
    lasso_u32x4 c0, c1, c2; memcpy(&c0, mail, 16); memcpy(&c1, mail + 4, 16); memcpy(&c2, mail + 8, 16);
    CHECK(mail_valid(c0, c1, c2, seq) && !mail_valid(c0, c1, c2, seq + 1));
    CHECK(c0.y == v.v[0] && c0.z == v.v[1] && c0.w == v.v[2] && c1.y == v.v[3] && c1.z == v.v[4] && c1.w == v.v[5] && c2.y == v.v[6] && c2.z == v.v[7]);   // the words the kernels take the challenge from
    lasso_u32x4 t = c1; t.z ^= 4u; CHECK(!mail_valid(c0, t, c2, seq));
    t = c1; t.x = seq - 1; CHECK(!mail_valid(c0, t, c2, seq));
  }
  printf("OK\n");
  return 0;
}
