// The lookup results as a vector (include/lasso_hip_values.h): out[k] = combine_lookups(T[sub(i)][dim[dimension(i)][k]], i < NUM_MEMORIES) — the vector whose multilinear
// extension at r is the proof's claimed_evaluation (subtables/mod.rs:187-216) — without the arrays E_i = T[dim] (32 bytes per lookup and memory) it is otherwise read from.
// Shape.  A streaming pass: per lookup 4 * C bytes of addresses in, 8 or 32 bytes out, nothing in between; lanes walk their items grid-stride (launch_plan.cuh values_plan)
// and every memory is STREAMED — address, table entry, one step of the combine — so no array is indexed by a memory number and nothing lands in scratch at C = 16.  The
// per-memory pointers and shifts travel by value in the kernarg segment and are read at wave-uniform indices (scalar loads).
// Two kernels:
//   k_lookup_values_int    AND / OR / XOR / RangeCheck / LT over u32 tables, in INTEGER arithmetic (values_combine.cuh): shifts and adds into 128 bits, or the LT walk in 64.
//                          An item is two consecutive lookups: the addresses of a dimension arrive as one 8-byte load and the 64-bit form leaves as one 16-byte store (an odd n:
//                          the last item loads and stores one).  The field form is ONE conversion of the integer (fr29_mul with R2S) and the canonical pack per lookup, not a
//                          field multiply-add per memory; it leaves as two 16-byte stores.
//   k_lookup_values_terms  everything else — Spark's product, a caller-defined g over field or u32 tables — by the packed term list the claim kernel reads
//                          (load_custom_terms<true>, k_combine_claim_custom's walk, radix and fold marks: poly_kernels.cuh), without the eq factor and the block sum.  Spark is
//                          the list of one term with C factors and coefficient 1, which the entry point builds.  A u32 entry is lifted to memory form where it is read.
// Table reads go through L2, not LDS.  A 2^16-entry u32 table is 256 KiB — more than a workgroup's 160 KiB of LDS, a sixteenth of an XCD's 4 MiB L2 — and a 2^16-entry field
// table is 2 MiB; staging would copy the table once per workgroup (thousands of copies out of L2 anyway) to save gathers that L2 already serves, and at the smaller tables the
// tests use, the lines stay in the vector cache.  The addresses and the output are the HBM streams; table traffic is L2 traffic and is NOT part of the byte model of the entry
// point's profiling scope or of DESIGN's table, which says so.
// An address is masked to log_m bits before it indexes a table: an address at or above 2^log_m is the caller's error (as for lasso_gather) and must not become a read outside
// the table.
#pragma once
#include "poly_kernels.cuh"
#include "values_combine.cuh"

struct ValuesMems {
  const uint32_t* dim[LASSO_MAX_ALPHA];   // the address column of memory i (its dimension's)
  const void* tab[LASSO_MAX_ALPHA];       // the subtable of memory i
  uint8_t shift[LASSO_MAX_ALPHA];         // linear kinds: i * inc
};

__device__ __forceinline__ void values_store_fr(fr_t* __restrict__ out, size_t k, const fr_t& w) {
  uint4* o = reinterpret_cast<uint4*>(out + k);
  o[0] = make_uint4(w.v[0], w.v[1], w.v[2], w.v[3]); o[1] = make_uint4(w.v[4], w.v[5], w.v[6], w.v[7]);
}
__device__ __forceinline__ fr_t values_int_to_fr(values_u128 v, const fr29& r2s) {
  int32_t l[5]; values_limbs(v, l);
  return fr29_store(fr29_mul(fr29_from_limbs(l[0], l[1], l[2], l[3], l[4], 0, 0, 0, 0), r2s));
}

// LT: memories 2m / 2m + 1 are LT / EQ of chunk m and share chunk m's address column, which is read once (M.dim[2m]); EQ_{C-1} enters no term and is not read.
template <bool LT, bool U64>
__global__ void __launch_bounds__(LASSO_BLOCK) k_lookup_values_int(ValuesMems M, uint32_t alpha, uint32_t mask, size_t n, void* __restrict__ out) {
  const size_t items = (n + 1) / 2;
  const fr29 r2s = fr29_r2s();
  for (size_t j = blockIdx.x * (size_t)blockDim.x + threadIdx.x; j < items; j += (size_t)gridDim.x * blockDim.x) {
    const size_t k = 2 * j; const bool two = k + 1 < n;
    values_u128 v0 = 0, v1 = 0;
    if constexpr (LT) {
      const uint32_t c = alpha / 2; uint64_t g0 = 0, g1 = 0;
      for (uint32_t m = c; m-- > 0;) {
        const uint32_t* __restrict__ d = M.dim[2 * m];
        const uint32_t* __restrict__ lt = static_cast<const uint32_t*>(M.tab[2 * m]);
        uint2 a; if (two) a = *reinterpret_cast<const uint2*>(d + k); else a = make_uint2(d[k], 0u);
        a.x &= mask; a.y &= mask;
        if (m + 1 == c) { g0 = lt[a.x]; g1 = lt[a.y]; }
        else { const uint32_t* __restrict__ eq = static_cast<const uint32_t*>(M.tab[2 * m + 1]); g0 = values_lt_step(lt[a.x], eq[a.x], g0); g1 = values_lt_step(lt[a.y], eq[a.y], g1); }
      }
      v0 = g0; v1 = g1;
    } else {
      for (uint32_t m = 0; m < alpha; m++) {
        const uint32_t* __restrict__ d = M.dim[m];
        const uint32_t* __restrict__ t = static_cast<const uint32_t*>(M.tab[m]);
        uint2 a; if (two) a = *reinterpret_cast<const uint2*>(d + k); else a = make_uint2(d[k], 0u);
        const uint32_t sh = M.shift[m];
        values_linear_add(v0, t[a.x & mask], sh); values_linear_add(v1, t[a.y & mask], sh);
      }
    }
    if constexpr (U64) {
      uint64_t* o = static_cast<uint64_t*>(out);
      if (two) *reinterpret_cast<ulonglong2*>(o + k) = make_ulonglong2((uint64_t)v0, (uint64_t)v1);
      else o[k] = (uint64_t)v0;
    } else {
      fr_t* o = static_cast<fr_t*>(out);
      values_store_fr(o, k, values_int_to_fr(v0, r2s));
      if (two) values_store_fr(o, k + 1, values_int_to_fr(v1, r2s));
    }
  }
}

// a table entry as a memory word: field tables hold them (any representative a device array may hold), u32 entries are lifted
template <bool TFR>
__device__ __forceinline__ fr_t values_entry(const void* __restrict__ tab, uint32_t a, const fr29& r2s) {
  if constexpr (TFR) return static_cast<const fr_t*>(tab)[a];
  else return fr29_store(fr29_mul(fr29_from_u64_int(static_cast<const uint32_t*>(tab)[a]), r2s));
}
// Magnitudes are k_combine_claim_custom's: a finished term is below 4 p, g is folded after every 4 terms; the last fold brings g below 2 p for the canonical pack.
template <bool TFR>
__global__ void __launch_bounds__(LASSO_BLOCK) k_lookup_values_terms(ValuesMems M, uint32_t mask, const CustomTermsDev* __restrict__ G, uint32_t nt, uint32_t nf, size_t n, fr_t* __restrict__ out) {
  __shared__ CustomTermsLds L;
  load_custom_terms<true>(G, nt, nf, L);
  const fr29 r2s = fr29_r2s();
  for (size_t i = blockIdx.x * (size_t)blockDim.x + threadIdx.x; i < n; i += (size_t)gridDim.x * blockDim.x) {
    fr29 g = fr29_zero();
    for (uint32_t t = 0; t < nt; t++) {
      const uint32_t b = __builtin_amdgcn_readfirstlane(L.term_start[t]), e = __builtin_amdgcn_readfirstlane(L.term_start[t + 1]);
      fr29 term;
      if (b == e) term = L.coeff[t];
      else {
        const uint32_t m0 = __builtin_amdgcn_readfirstlane(L.term_mem[b]);
        term = fr29_unpack_u(values_entry<TFR>(M.tab[m0], M.dim[m0][i] & mask, r2s));
        if (!(__builtin_amdgcn_readfirstlane(L.flags[t]) & 2u)) term = fr29_mul(term, L.coeff[t]);
        for (uint32_t j = b + 1; j < e; j++) {
          const uint32_t m = __builtin_amdgcn_readfirstlane(L.term_mem[j]);
          term = fr29_mul(fr29_unpack_s(values_entry<TFR>(M.tab[m], M.dim[m][i] & mask, r2s)), term);
        }
      }
      g = fr29_weak(fr29_add(g, term));
      if ((t & 3u) == 3u) g = fr29_mul(g, fr29_one_s());
    }
    values_store_fr(out, i, fr29_store(fr29_mul(g, fr29_one_s())));
  }
}
