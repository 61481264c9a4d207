// The hand-off protocol between the kernels and the host: the wire encoding both sides share, and the host's record of what is in flight.
// Plain C++17 — no HIP runtime, no device memory: tests/cpp/test_handoff_host.cpp includes it as it is.  The kernels' half of the encoding is handoff_device.cuh.
#pragma once
#include <cstddef>
#include <cstdint>
#include <initializer_list>
#if defined(__SSE2__)
#include <emmintrin.h>   // 16-byte single-copy stores / loads of the hand-off chunks; other hosts take the per-word fallbacks (the check word covers tearing)
#endif

// ------------------------------------------------------------------ the wire encoding
// An element (a result for the host, a challenge for a resident kernel) travels as three self-validating 16-byte chunks [tag, w0, w1, w2] [tag, w3, w4, w5] [tag, w6, w7, check],
// each ONE aligned 16-byte store; the reader accepts it once all three carry the hand-off's sequence number and the check word agrees, which also rejects a chunk that arrived in pieces.
#define LASSO_MAIL_POISON 0xFFFFFFFFu   // mailbox tag written by lasso_abort: resident kernels waiting for a challenge leave at once (sequence tags never reach it)
// the check word of eight data words under a tag (a macro: the kernels' code is the expression itself, whatever form their words come in)
#define HANDOFF_CHECK(w0, w1, w2, w3, w4, w5, w6, w7, tag) (((w0) ^ (w1) ^ (w2) ^ (w3) ^ (w4) ^ (w5) ^ (w6) ^ (w7)) + (tag) * 0x9E3779B9u)
// One element of the tagged result area (handoff_device.cuh result_store): true once all three chunks carry `seq` and the check word agrees.  Each chunk is read with
// one aligned 16-byte load (the device wrote it with one aligned 16-byte store); the check word also covers a platform that would tear either.
static inline bool tagged_element(const uint32_t* e, uint32_t seq, uint32_t* w8) {
  uint32_t c[12];
#if defined(__SSE2__)
  for (int k = 0; k < 3; k++) _mm_storeu_si128((__m128i*)(c + 4 * k), _mm_load_si128((const __m128i*)(e + 4 * k)));
#else
  for (int k = 0; k < 12; k++) c[k] = __atomic_load_n(e + k, __ATOMIC_ACQUIRE);
#endif
  if (c[0] != seq || c[4] != seq || c[8] != seq) return false;
  w8[0] = c[1]; w8[1] = c[2]; w8[2] = c[3]; w8[3] = c[5]; w8[4] = c[6]; w8[5] = c[7]; w8[6] = c[9]; w8[7] = c[10];
  return c[11] == HANDOFF_CHECK(w8[0], w8[1], w8[2], w8[3], w8[4], w8[5], w8[6], w8[7], seq);
}
// the host -> device direction: one mailbox entry (the kernels check it with mail_valid)
static inline void mail_chunks(uint32_t* mail, uint32_t tag, const uint32_t w[8]) {
  const uint32_t chk = HANDOFF_CHECK(w[0], w[1], w[2], w[3], w[4], w[5], w[6], w[7], tag);
#if defined(__SSE2__)
  _mm_store_si128((__m128i*)(mail + 0), _mm_set_epi32((int)w[2], (int)w[1], (int)w[0], (int)tag));
  _mm_store_si128((__m128i*)(mail + 4), _mm_set_epi32((int)w[5], (int)w[4], (int)w[3], (int)tag));
  _mm_store_si128((__m128i*)(mail + 8), _mm_set_epi32((int)chk, (int)w[7], (int)w[6], (int)tag));
#else   // no 16-byte store: data words first, the tags last (a reader that sees all three tags with a matching check word has the whole message)
  const uint32_t m[12] = {tag, w[0], w[1], w[2], tag, w[3], w[4], w[5], tag, w[6], w[7], chk};
  for (int k : {1, 2, 3, 5, 6, 7, 9, 10, 11}) __atomic_store_n(mail + k, m[k], __ATOMIC_RELAXED);
  for (int k : {0, 4, 8}) __atomic_store_n(mail + k, m[k], __ATOMIC_RELEASE);
#endif
}
// what every post ends with
static inline void mail_fence() {
#if defined(__SSE2__)
  _mm_sfence();   // release: the chunks are globally visible before anything the host does next
#else
  __atomic_thread_fence(__ATOMIC_SEQ_CST);
#endif
}

// ------------------------------------------------------------------ the host's record of what is in flight
// What wait_flag needs to collect one result: `count` elements published under sequence number `seq`, as tagged chunks or through the flag; groups > 1: every workgroup of a
// row published its own block sums (LASSO_TAGGED_DIRECT), `groups` per row and K values per row, and the host adds them.
struct Handoff { uint32_t seq = 0; size_t count = 0; bool tagged = false; uint32_t groups = 1, K = 0; };

// One per context.  The transitions below only move state and say what the caller has to post or wait for: no HIP call, no mailbox.  An entry point checks its REQUIREs,
// launches, and calls the transition once the launch has succeeded.
struct HandoffState {
  bool pending = false, defer_next = false; Handoff result;   // a result not yet collected by lasso_result_wait; lasso_defer_next: the next hand-off is parked instead of awaited
  // a round (or, `ahead_bullet`, a bullet round / the end of an opening) launched ahead of its challenge: lasso_challenge_post / lasso_bullet_post turn it into the pending result
  bool ahead_active = false, ahead_bullet = false; Handoff ahead;
  // a LAYER's first launch enqueued ahead of the layer's eq point (legal while the previous layer's tail is still active): lasso_point_post turns it into the pending result and,
  // in the tail form (lay_tail), the active tail; lasso_point_cancel ends it without a result
  bool lay_active = false, lay_tail = false; Handoff lay; uint32_t lay_ell = 0, lay_turns = 0; size_t lay_final = 0;
  // the resident sumcheck-tail kernel: publication t of its tail_turns + 1 carries sequence number tail.seq + t; tail.count values per round of sums, tail_final after the last
  // challenge (the heads, or the handed-over arrays).  tail_unstarted: launched AHEAD of the challenge it binds first, the first next() starts it
  bool tail_active = false, tail_unstarted = false; Handoff tail; uint32_t tail_turn = 0, tail_turns = 0; size_t tail_final = 0;
  uint32_t handover_next = 0;   // lasso_tail_handover_next: the next cubic tail stops at this many elements per array and hands the arrays over (one-shot)
  bool no_grow = false;         // set around a launch enqueued behind a resident kernel: a buffer that would have to grow is LASSO_ERR_UNSUPPORTED, the caller takes the ordinary path
  uint32_t gate_sent = 0;       // sequence number of the last point gate launched: the point mailbox is its until the gate has acknowledged it (gate_free)

  // ---- predicates
  // nothing in flight: memory may be released and the sequence numbers may start a new epoch
  bool idle() const { return !pending && !tail_active && !ahead_active && !lay_active; }
  // a launch is waiting on the device for the host: whatever synchronises the stream would sit in the kernel's 5 s bail-out and lose the round
  bool waiting_on_device() const { return ahead_active || lay_active; }
  // a context buffer may be reallocated (which synchronises the stream)
  bool may_grow() const { return !no_grow && !waiting_on_device(); }

  // ---- transitions
  void park(const Handoff& h) { pending = true; result = h; }
  // lasso_defer_next is armed: the result is parked for lasso_result_wait instead of awaited now
  bool park_deferred(const Handoff& h) { if (!defer_next) return false; defer_next = false; park(h); return true; }
  Handoff collect() { pending = false; return result; }
  void arm_ahead(const Handoff& h, bool bullet) { ahead_active = true; ahead_bullet = bullet; ahead = h; }
  uint32_t post_ahead() { ahead_active = false; park(ahead); return ahead.seq; }
  void arm_layer(const Handoff& h, uint32_t ell) { lay_active = true; lay_tail = false; lay = h; lay_ell = ell; }
  void arm_layer_tail(const Handoff& first, uint32_t ell, uint32_t turns, size_t final_count) { lay_active = true; lay_tail = true; lay = first; lay_ell = ell; lay_turns = turns; lay_final = final_count; }
  void post_layer() { lay_active = false; if (lay_tail) begin_tail(lay, lay_turns, lay_final, false); else park(lay); lay_tail = false; }
  void cancel_layer() { lay_active = false; lay_tail = false; }
  // `first`: the first round's sums; a hand-over only shows in `turns` and `final_count`.  unstarted: nothing is pending until the first challenge has been posted
  void begin_tail(const Handoff& first, uint32_t turns, size_t final_count, bool unstarted) {
    tail_active = true; tail_unstarted = unstarted; tail = first; tail_turn = 0; tail_turns = turns; tail_final = final_count;
    if (!unstarted) park(first);
  }
  // a challenge for the tail: returns the tag to post it under (= the sequence number of the publication it enables: tags are unique, the mailbox is never reset) and installs
  // that publication as the pending result; the last turn ends the tail
  uint32_t tail_next() {
    if (tail_unstarted) { tail_unstarted = false; park(tail); return tail.seq; }
    const uint32_t tag = tail.seq + ++tail_turn;
    const bool last = tail_turn == tail_turns;
    const size_t cnt = last ? tail_final : tail.count;
    if (cnt) park(Handoff{tag, cnt, tail.tagged});
    if (last) tail_active = false;
    return tag;
  }
  uint32_t take_handover() { const uint32_t m = handover_next; handover_next = 0; return m; }
  void reset() { *this = HandoffState(); }   // lasso_abort, once the stream is drained
};
