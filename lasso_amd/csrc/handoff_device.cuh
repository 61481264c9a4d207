// The kernels' half of the hand-off encoding (handoff.cuh): how a launch hands its few field elements to the host, and how a resident kernel checks the host's mail.
// Needs a compiler with ext_vector_type (hipcc, clang); the host test includes it under shims for __device__, __forceinline__, __restrict__ and __hip_atomic_store.
#pragma once
#include "fr.cuh"
#include "handoff.cuh"
// Two ways a launch hands its few field elements to the host, chosen by the `flag` argument every round kernel takes:
//  * flag = a word of host-mapped memory: elements stored to out[slot] (host-mapped), then row_done: system-scope fence, an agent-scope ticket over the
//    grid rows, and the row that arrives last stores the sequence number to the flag.  4.1 us from the host's word to the host seeing the answer for a
//    resident workgroup (tools/handoff_bench.hip);
//  * flag = LASSO_TAGGED: `out` is an area of SELF-VALIDATING 16-byte chunks, three per element: [seq, w0, w1, w2] [seq, w3, w4, w5] [seq, w6, w7, check].
//    Every row stores its own chunks (one aligned dwordx4 each = one PCIe write) and releases them with ONE system-scope fence: no ticket, no flag store, no
//    cross-row ordering.  The host accepts an element once its three chunks carry the hand-off's sequence number (unique for the life of the context) and the
//    check word matches.  2.1-2.3 us for the same turn.
#define LASSO_TAGGED (reinterpret_cast<uint32_t*>(uintptr_t(16)))
// the same area, and EVERY workgroup of a row publishes its own block sums under slot (row * nx + bx) * K + k: the host adds the nx of them (lasso_hip.hip wait_flag) — for launches
// of a few workgroups per row, where the in-launch second stage (agent-scope release, ticket, acquire, re-read, second block reduction) is a third of the kernel's time
#define LASSO_TAGGED_DIRECT (reinterpret_cast<uint32_t*>(uintptr_t(32)))
typedef uint32_t lasso_u32x4 __attribute__((ext_vector_type(4)));
__device__ __forceinline__ uint32_t result_check(const fr_t& v, uint32_t seq) { return HANDOFF_CHECK(v.v[0], v.v[1], v.v[2], v.v[3], v.v[4], v.v[5], v.v[6], v.v[7], seq); }
__device__ __forceinline__ void result_store(fr_t* __restrict__ out, size_t slot, const fr_t& v, uint32_t* flag, uint32_t seq) {
  if (flag == LASSO_TAGGED || flag == LASSO_TAGGED_DIRECT) {
    lasso_u32x4* o = reinterpret_cast<lasso_u32x4*>(out) + 3 * slot;
    const lasso_u32x4 c0 = {seq, v.v[0], v.v[1], v.v[2]}, c1 = {seq, v.v[3], v.v[4], v.v[5]}, c2 = {seq, v.v[6], v.v[7], result_check(v, seq)};
    o[0] = c0; o[1] = c1; o[2] = c2;
  } else {
    // A value another workgroup of THIS launch will read (block partials on their way to last_block_reduce): write-through (sc1) 8-byte stores, so that what publishes them
    // is the storing wave's `s_waitcnt vmcnt(0)` and not an L2 write-back (round 6; cdna_hip_programming.md §6 G16, the sc1 form).  The release fence this replaces wrote back
    // EVERY dirty line of the XCD's L2 — and every workgroup of a fused round has just dirtied 32 KB of bound values there: 512 such fences per launch.
    // (flag != nullptr: the flag protocol's result area in host-mapped memory, LASSO_TAGGED_RESULTS=0 — plain stores, published by row_done's system-scope fence as before)
#ifndef LASSO_PLAIN_PARTIALS
    if (flag == nullptr) {
      uint64_t* o = reinterpret_cast<uint64_t*>(out + slot);
#pragma unroll
      for (int k = 0; k < 4; k++) __hip_atomic_store(o + k, (uint64_t)v.v[2 * k] | ((uint64_t)v.v[2 * k + 1] << 32), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      return;
    }
#endif
    out[slot] = v;
  }
}
// the host -> device direction of a resident kernel (lasso_hip.hip post_mail): the three mailbox chunks carry this tag and the check word of their eight challenge words
__device__ __forceinline__ bool mail_valid(const lasso_u32x4& c0, const lasso_u32x4& c1, const lasso_u32x4& c2, uint32_t tag) {
  return c0.x == tag && c1.x == tag && c2.x == tag && c2.w == HANDOFF_CHECK(c0.y, c0.z, c0.w, c1.y, c1.z, c1.w, c2.y, c2.z, tag);
}
