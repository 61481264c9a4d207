// Every LASSO_* environment variable the HOST sources read (prover.hpp, prover_capi.cpp, field52.hpp), one line each: name, default, meaning.  A switch is read once per
// process, on first use (tests change one per child process); on / off goes by the first character: "0" switches a default-on switch off, "1" a default-off one on.
// They select WHERE and WHEN the same field arithmetic runs: no setting changes a byte of a proof.  The device library's own switches are listed in the same way in lasso_amd/csrc/device_switches.cuh.
#pragma once
#include <cstdlib>

namespace lasso { namespace sw {
inline bool unless0(const char* e) { return !(e && e[0] == '0'); }   // default on
inline bool if1(const char* e) { return e && e[0] == '1'; }           // default off
#define LASSO_SWITCH(type, name, value) inline type name() { static const type v = (value); return v; }
// LASSO_MLE_DEVICE_MIN's default: the smallest MEASURED num_subtables * 2^log_m from which the device route's slowest verify stays below the host loop's fastest
// (4 subtables of 2^12 entries: 12.24 ms [12.05, 12.33] against 13.30 ms [12.92, 13.48]; profiles/verify_device_mle.json) — smaller strategies stay on the host
#define LASSO_MLE_DEVICE_MIN_DEFAULT ((size_t)16384)
LASSO_SWITCH(int, trace, [] { const char* e = getenv("LASSO_TRACE"); return e && e[0] >= '1' && e[0] <= '3' ? e[0] - '0' : 0; }())   // 0; 1: wall-clock spans (Trace), 2: host time buckets (HostClock), 3: device bytes per span
LASSO_SWITCH(bool, capacity, if1(getenv("LASSO_CAPACITY")))                  // off; capacity mode for every host (Dev::capacity; lasso_host_set_capacity sets it per host)
LASSO_SWITCH(bool, capacity_compact, unless0(getenv("LASSO_CAPACITY_COMPACT")))   // on; capacity mode holds dim / read as 32-bit integers
LASSO_SWITCH(size_t, leafless_min, [] { const char* e = getenv("LASSO_LEAFLESS_MIN"); const size_t x = e ? (size_t)atoll(e) : ((size_t)1 << 16); return x < 64 ? (size_t)64 : x; }())   // 2^16, at least 64; capacity mode: local lookups from which the trees are kept without leaves
LASSO_SWITCH(bool, throughput_ahead, if1(getenv("LASSO_THROUGHPUT_AHEAD")))  // off; throughput mode launches ahead of the challenge all the same
LASSO_SWITCH(bool, side_stream, unless0(getenv("LASSO_SIDE_STREAM")))        // on; a second context per host for work that does not depend on the transcript
LASSO_SWITCH(bool, slab_open, unless0(getenv("LASSO_SLAB_OPEN")))            // on; slab mode shares the openings' MSMs between the ranks
LASSO_SWITCH(bool, eq_inline, unless0(getenv("LASSO_EQ_INLINE")))            // on; a layer's eq table is built inside round 0's launch (off: by its own kernels, no layer ahead)
LASSO_SWITCH(bool, cubic_tail, unless0(getenv("LASSO_CUBIC_TAIL")))          // on; the last cubic rounds of a phase in one resident kernel
LASSO_SWITCH(bool, linear_tail, unless0(getenv("LASSO_LINEAR_TAIL")))        // on; the same for the linear strategies' sumcheck
LASSO_SWITCH(bool, rounds_ahead, unless0(getenv("LASSO_ROUNDS_AHEAD")))      // on; round j + 1 enqueued behind round j, ahead of its challenge
LASSO_SWITCH(bool, slab_ahead, unless0(getenv("LASSO_SLAB_AHEAD")))          // on; the same with a collective between the rounds (slab-local phases)
LASSO_SWITCH(bool, cubic_three_sums, if1(getenv("LASSO_CUBIC_THREE_SUMS")))  // off; every streaming cubic round takes the three-sum form of the rand_j = 0 path
LASSO_SWITCH(bool, slab_host_tail, unless0(getenv("LASSO_SLAB_HOST_TAIL")))  // on; slab mode: the last log2 P rounds of a layer on the host (off: replicated device arrays)
LASSO_SWITCH(bool, slab_host_tops, unless0(getenv("LASSO_SLAB_HOST_TOPS")))  // on; slab mode: the replicated top layers built and proved on the host
LASSO_SWITCH(bool, sumcheck_u32, unless0(getenv("LASSO_SUMCHECK_U32")))      // on; the primary sumcheck's first round reads E as 32-bit integers
LASSO_SWITCH(bool, host_ifma, unless0(getenv("LASSO_HOST_IFMA")))            // on; the host's rounds eight elements at a time where the CPU has AVX-512 IFMA (field52.hpp)
inline size_t host_tail(bool ifma) { static const size_t v = [&] { const char* e = getenv("LASSO_HOST_TAIL"); const long x = e ? atol(e) : (ifma ? 128 : 32); return (size_t)(x < 0 ? 0 : x > 1024 ? 1024 : x); }(); return v; }   // 128 with IFMA, else 32; 0..1024: elements x circuits at which the host takes a layer over, 0 = never
LASSO_SWITCH(bool, verify_device_points, unless0(getenv("LASSO_VERIFY_DEVICE_POINTS")))   // on; the verifier decodes compressed points on the device
LASSO_SWITCH(size_t, wire_device_min, [] { const char* e = getenv("LASSO_WIRE_DEVICE_MIN"); const long long x = e ? atoll(e) : 376; return (size_t)(x < 1 ? 1 : x); }())   // 376 (the smallest batch measured with the device ahead), at least 1
LASSO_SWITCH(bool, verify_msm_points, unless0(getenv("LASSO_VERIFY_MSM_POINTS")))         // on; the verifier's MSMs over commitment rows run table-free (lasso_msm_points) instead of lasso_bases_create + lasso_msm
LASSO_SWITCH(bool, densify_operands, unless0(getenv("LASSO_DENSIFY_OPERANDS")))           // on; lasso_host_densify_operands forms the chunk indices on the device (off: expanded on the host, then the index path)
LASSO_SWITCH(bool, gens_device, unless0(getenv("LASSO_GENS_DEVICE")))                     // on; label-derived generators: the candidates' arithmetic in one lasso_points_from_candidates launch (off: one by one on the host)
LASSO_SWITCH(size_t, gens_device_min, [] { const char* e = getenv("LASSO_GENS_DEVICE_MIN"); const long long x = e ? atoll(e) : 8194; return (size_t)(x < 1 ? 1 : x); }())   // 8194 (the smallest set measured with the device ahead on both curves), at least 1; smaller sets stay on the host
LASSO_SWITCH(size_t, gens_device_batch, [] { const char* e = getenv("LASSO_GENS_DEVICE_BATCH"); const long long x = e ? atoll(e) : 0; return (size_t)(x < 1 ? 0 : x); }())   // 0 = no cap; most candidates per device call (bounds the call's scratch: 98 bytes per candidate)
LASSO_SWITCH(bool, verify_device_mle, unless0(getenv("LASSO_VERIFY_DEVICE_MLE")))         // on; the verifier evaluates a caller-defined strategy's subtable MLEs in one lasso_tables_mle call (off: the host loop, 2^log_m products per subtable)
LASSO_SWITCH(size_t, mle_device_min, [] { const char* e = getenv("LASSO_MLE_DEVICE_MIN"); if (!e) return LASSO_MLE_DEVICE_MIN_DEFAULT; const long long x = atoll(e); return (size_t)(x < 0 ? 0 : x); }())   // see LASSO_MLE_DEVICE_MIN_DEFAULT; strategies with num_subtables * 2^log_m below it stay on the host
// the two read per CALL, not per process (a test sets them between calls):
inline bool slab_rccl() { return unless0(getenv("LASSO_SLAB_RCCL")); }             // on; slab mode's bulk exchange over RCCL (lasso_host_set_comm_shm)
inline bool debug_cubic_host() { return if1(getenv("LASSO_DEBUG_CUBIC_HOST")); }   // off; lasso_host_debug_prove_cubic_batched runs the HOST rounds
#undef LASSO_SWITCH
} }  // namespace lasso::sw
