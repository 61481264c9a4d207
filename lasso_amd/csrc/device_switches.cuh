// Every LASSO_* environment variable the DEVICE library reads (lasso_hip.hip), one line each: name, default, clamp, meaning.  The host prover's are lasso_amd/host/switches.hpp; the
// conventions are the same: a switch is read once per process, on first use (tests change one per child process); on / off goes by the first character: "0" switches a
// default-on switch off, "1" a default-off one on.  They select WHICH kernel or protocol serves the same arithmetic: no setting changes a byte of a commitment or a proof — except
// the one marked EXPERIMENT.  Plain C++, no HIP include: tests/cpp/test_launch_plan_host.cpp includes it as it is.
#pragma once
#include <cstddef>
#include <cstdint>
#include <cstdlib>

namespace lasso { namespace dsw {
inline bool unless0(const char* e) { return !(e && e[0] == '0'); }   // default on
inline bool if1(const char* e) { return e && e[0] == '1'; }           // default off
#define LASSO_DSWITCH(type, name, value) inline type name() { static const type v = (value); return v; }
// ---- the hand-off protocol
LASSO_DSWITCH(bool, tagged_results, unless0(getenv("LASSO_TAGGED_RESULTS")))   // on; results handed over as self-validating tagged chunks (off: the flag protocol for every hand-off)
LASSO_DSWITCH(long long, seq_start, [] { const char* e = getenv("LASSO_SEQ_START"); return e ? (long long)(uint32_t)strtoul(e, nullptr, 0) : -1LL; }())   // unset (-1: a context starts at 0); tests: a context's first hand-off sequence number (to cross next_seq's epoch restart)
LASSO_DSWITCH(bool, msm_tagged, unless0(getenv("LASSO_MSM_TAGGED")))           // on; the few-row MSMs hand their points over as tagged elements where the context is in tagged mode
// ---- the sumcheck rounds
LASSO_DSWITCH(long, cubic_nx, [] { const char* e = getenv("LASSO_CUBIC_NX"); return e ? atol(e) : 0L; }())   // 0 (unset or <= 0): about 512 workgroups over the whole grid; > 0: the x-extent cap of the round grids itself (experiments)
LASSO_DSWITCH(long, reduce_nx, [] { const char* e = getenv("LASSO_REDUCE_NX"); return e ? atol(e) : 0L; }())   // 0 (unset or <= 0): each launch's own cap; > 0: the x-extent cap of the reduction launches outside the round grids (combine rounds and claims, multi_dot, inner_products_lr; tests)
LASSO_DSWITCH(long, values_nx, [] { const char* e = getenv("LASSO_VALUES_NX"); return e ? atol(e) : 0L; }())   // 0 (unset or <= 0): up to 4096 workgroups; > 0: the x-extent cap of lasso_lookup_values' launch (tests: several grid-stride passes per lane on small arrays)
LASSO_DSWITCH(bool, cubic_wide,unless0(getenv("LASSO_CUBIC_WIDE")))           // on; double-width accumulators in the two-sum fused round
LASSO_DSWITCH(unsigned, direct_nx, [] { const char* e = getenv("LASSO_DIRECT_NX"); const long x = e ? atol(e) : 16; return (unsigned)(x < 0 ? 0 : x > 64 ? 64 : x); }())   // 16, 0..64; launches of up to this many workgroups per circuit hand over every workgroup's block sums (0: never)
LASSO_DSWITCH(bool, eq_inline_big, if1(getenv("LASSO_EQ_INLINE_BIG")))         // off; eq tables above 2^14 entries formed inside round 0 (EqGlobal) instead of by k_eq_outer in front of it
LASSO_DSWITCH(bool, lb_pipeline, unless0(getenv("LASSO_LB_PIPELINE")))         // on; software pipelining in the evaluation-only round
LASSO_DSWITCH(bool, lb_nt, if1(getenv("LASSO_LB_NT")))                         // off; non-temporal loads of A and B in the evaluation-only round (only with the pipeline on)
LASSO_DSWITCH(unsigned, ahead_inkernel_wgs, [] { const char* e = getenv("LASSO_AHEAD_INKERNEL_WGS"); const long x = e ? atol(e) : 32; return (unsigned)(x < 0 ? 0 : x > 4096 ? 4096 : x); }())   // 32, 0..4096; up to this many workgroups a round launched ahead waits inside its own kernel (0: always the gate kernel)
LASSO_DSWITCH(bool, rounds_ahead, unless0(getenv("LASSO_ROUNDS_AHEAD")))       // on; rounds may be launched ahead of their challenge (lasso_rounds_ahead_ok; the host prover reads the same variable, host/switches.hpp)
LASSO_DSWITCH(bool, layer_ahead, unless0(getenv("LASSO_LAYER_AHEAD")))         // on; a layer's first launch may be enqueued ahead of its eq point (lasso_layer_ahead_ok)
LASSO_DSWITCH(bool, tail_q_256, [] { const char* e = getenv("LASSO_TAIL_Q"); return (e ? atol(e) : 0) == 256; }())   // off (any other value: CUBIC_TAIL_Q = 512); LASSO_TAIL_Q=256: the resident tails' capacity of round 2 (lasso_sumcheck_tail_capacity)
LASSO_DSWITCH(bool, exp_no_leaf_store, if1(getenv("LASSO_EXP_NO_LEAF_STORE"))) // off; EXPERIMENT, timing only: the fingerprint kernel without its leaf stores — the proof that follows is INVALID
// ---- the MSMs
LASSO_DSWITCH(size_t, msm_direct_max_n, [] { const char* e = getenv("LASSO_MSM_DIRECT_MAX_N"); return e ? (size_t)atoll(e) : (((size_t)1 << 17) + 64); }())   // 2^17 + 64; generator sets up to this size get the digit-multiple table (k_msm_direct)
LASSO_DSWITCH(size_t, msm_direct8_max_n, [] { if (!unless0(getenv("LASSO_MSM_DIRECT8"))) return (size_t)0; const char* e = getenv("LASSO_MSM_DIRECT8_MAX_N"); return e ? (size_t)atoll(e) : (((size_t)1 << 14) + 64); }())   // 2^14 + 64; ... and the byte-multiple table; LASSO_MSM_DIRECT8=0 (default on): 0, no set gets it
LASSO_DSWITCH(bool, msm_direct, unless0(getenv("LASSO_MSM_DIRECT")))           // on; the few-row full-width MSMs by the latency-shaped kernel over the multiple tables (off: the bucket kernel)
LASSO_DSWITCH(long, msm_direct_wgs, [] { const char* e = getenv("LASSO_MSM_DIRECT_WGS"); return e ? atol(e) : 0L; }())   // 0 (unset), as parsed: workgroups of a latency-shaped MSM launch.  Each user has its own validity rule (launch_plan.cuh): msm_direct_chunks takes 1..4096, bullet_round_fused 4..4096 (1..3 fall back there), anything else is 256
LASSO_DSWITCH(bool, msm_fused, unless0(getenv("LASSO_MSM_FUSED")))             // on; conversions and the bullet fold inside the MSM launch
LASSO_DSWITCH(bool, msm_rows8, unless0(getenv("LASSO_MSM_ROWS8")))             // on; commitments of small scalars over byte-multiple tables (k_msm_rows8 / k_msm_rows8w), built on first use
LASSO_DSWITCH(bool, msm_rows8w, unless0(getenv("LASSO_MSM_ROWS8W")))           // on; many short rows: one wave per row (k_msm_rows8w) instead of the 256-lane form
LASSO_DSWITCH(size_t, msm_rows8w_waves, [] { const char* e = getenv("LASSO_MSM_ROWS8W_WAVES"); const long x = e ? atol(e) : 0; return (size_t)(x < 0 ? 0 : x); }())   // 0 (one row per wave), at least 0; N: at most N waves per k_msm_rows8w launch, several rows per wave
LASSO_DSWITCH(bool, msm_full8, if1(getenv("LASSO_MSM_FULL8")))                 // off; full-width commitments over the signed byte-multiple table (k_msm_rows_full<8>) instead of the bucket kernel
LASSO_DSWITCH(bool, bullet_ahead, unless0(getenv("LASSO_BULLET_AHEAD")))       // on; the openings' folding rounds may be enqueued ahead of their challenge
LASSO_DSWITCH(bool, bullet_tail_ahead, unless0(getenv("LASSO_BULLET_TAIL_AHEAD")))   // on; the opening's last fold, heads and delta MSM as one chain enqueued ahead of the last challenge
// ---- the context's own buffers
LASSO_DSWITCH(bool, scratch_guard, if1(getenv("LASSO_SCRATCH_GUARD")))         // off; tests: a guard pattern directly behind the REQUESTED size of every scratch / sort / big-result request, verified by lasso_sync and lasso_trim (launch_plan.cuh SCRATCH_GUARD_BYTES)
LASSO_DSWITCH(bool, poison, if1(getenv("LASSO_POISON")))                       // off; tests: every allocation the library makes, and the requested range of every first scratch / sort / big-result request of a call, starts as POISON_WORD repeated instead of as whatever was there (launch_plan.cuh poison_range)
// the fill of LASSO_POISON, as 32-bit words: a stale field element, counter or flag is non-zero, and a stale word used as an index stays inside any table of two or more entries
// (all-ones or random bytes would turn a stray indexed read into an access out of bounds).  The oracle's mock fills its lasso_alloc with the same word.
static const uint32_t POISON_WORD = 0x00000001u;
// host memory [p, p + bytes) as `word` repeated from p on (p 4-byte aligned; a tail of 1..3 bytes gets the word's first bytes in memory order)
inline void poison_fill_host(void* p, size_t bytes, uint32_t word) {
  uint32_t* w = (uint32_t*)p; for (size_t i = 0; i < bytes / 4; i++) w[i] = word;
  for (size_t i = bytes & ~(size_t)3; i < bytes; i++) ((uint8_t*)p)[i] = ((const uint8_t*)&word)[i & 3];
}
// ---- the four read per CALL, not per process (a commitment of that size is milliseconds; one test process runs both forms):
inline long long mle_strip() { const char* e = getenv("LASSO_MLE_STRIP"); const long long x = e ? atoll(e) : 0; return x < 0 ? 0 : x; }   // 0 (unset): 64 MiB of strips over all tables; N: lasso_tables_mle uploads N entries of every table per strip (tests: strip boundaries within small tables)
inline bool msm_pip() { return unless0(getenv("LASSO_MSM_PIP")); }   // on; many long rows of full-width scalars by the 12-bit-window kernels (k_msm_pip_*) instead of the bucket kernel
inline size_t msm_pip_min_cols() { const char* e = getenv("LASSO_MSM_PIP_MIN_COLS"); const long x = e ? atol(e) : 512; return (size_t)(x < 1 ? 1 : x); }   // 512, at least 1; columns from which they serve
inline size_t msm_pip_scratch_mb() { const char* e = getenv("LASSO_MSM_PIP_SCRATCH_MB"); const long x = e ? atol(e) : 1200; return (size_t)(x < 16 ? 16 : x); }   // 1200, at least 16; MiB of scratch a group of rows may take
#undef LASSO_DSWITCH
} }  // namespace lasso::dsw
