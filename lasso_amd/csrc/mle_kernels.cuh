// SubtableStrategy::evaluate_subtable_mle for caller-defined tables (include/lasso_hip_mle.h): out[k] = sum_i T_k[i] chi_i(point) without the 2^log_m-entry eq table.
//   chi_i = hi[i_hi] * lo[i_lo],  i = i_hi 2^lo_bits + i_lo  (launch_plan.cuh mle_plan: the first ceil(log_m / 2) coordinates in hi, both tables at most 2^15 entries,
//   built by k_eq_small2 in front of the streaming pass and read from L2 afterwards).
// Shape.  A LANE owns a column i_lo and a run of rows, consecutive lanes consecutive columns: every table read of a wave is one contiguous segment (256 B in the u32 form,
// 2 KB in the Fr form), the row factor hi[i_hi] is the same address for all lanes of a run (one broadcast line), and the lazy sum (mle_acc.cuh) runs over ROWS:
//   sum_i T[i] chi_i = sum_{i_lo} lo[i_lo] * (sum_{i_hi} T[i] hi[i_hi]).
// One Montgomery reduction and one full product per lane, whatever the run's length.  The other orientation — the inner sum over i_lo, one product with hi[i_hi] per row —
// needs the lanes of a row to SHARE the row (for the same contiguous reads), so every lane would end every row with its own reduction and product: 256 / 2^lo_bits times
// the products per entry, most where tables are small.
// Radix.  hi carries the call's scale, lo does not: A / 2^261 * lo / 2^261 is 2^10 short of a product of two memory-form values (fr29.cuh), which the block sum's shift
// supplies.  Fr entries are memory form (x 2^256): scale = 1.  u32 entries are plain integers: scale = 2^256 (memory words R^2 mod p), so the sum leaves in memory form.
// Strips.  The launch walks entries [e0, e1) of every table, table k's entry e0 at T.p[k][0]: the host form's strips, or the whole resident table (e0 = 0, e1 = 2^log_m).
#pragma once
#include "poly_kernels.cuh"
#include "mle_acc.cuh"

struct MleTables { const void* p[MLE_MAX_TABLES]; };

template <bool FR>
__global__ void __launch_bounds__(LASSO_BLOCK) k_tables_mle(MleTables T, uint32_t nx, uint32_t ny, const fr_t* __restrict__ hi, const fr_t* __restrict__ lo, uint32_t lo_bits, uint32_t row_first,
                                                            uint32_t rows, uint32_t rows_per_task, uint64_t e0, uint64_t e1, fr_t* __restrict__ partials, uint32_t* counters,
                                                            fr_t* __restrict__ out, uint32_t* flag, uint32_t seq) {
  __shared__ RedScratch S;
  const CubicGrid g = cubic_grid(nx, ny);
  const uint64_t task = (uint64_t)g.bx * LASSO_BLOCK + threadIdx.x;
  const uint32_t i_lo = (uint32_t)(task & (((uint64_t)1 << lo_bits) - 1));
  const uint64_t run = task >> lo_bits;
  fr29 e[3] = {fr29_zero(), fr29_zero(), fr29_zero()};
  if (run * rows_per_task < rows) {
    const uint32_t r0 = row_first + (uint32_t)run * rows_per_task;
    uint32_t r1 = r0 + rows_per_task; if (r1 > row_first + rows) r1 = row_first + rows;
    uint32_t cnt = 0; bool any = false;
    fr29 inner;
    if constexpr (FR) {
      const fr_t* __restrict__ tab = static_cast<const fr_t*>(T.p[g.by]);
      fr29_acc w = fr29_acc_zero();
      for (uint32_t r = r0; r < r1; r++) {
        const uint64_t i = ((uint64_t)r << lo_bits) + i_lo;
        if (i < e0 || i >= e1) continue;   // a strip begins and ends anywhere inside a row
        mle_fr_acc_add(w, fr29_unpack_u(tab[i - e0]), fr29_unpack_u(hi[r])); any = true;
        if (++cnt == MLE_FR_FOLD_EVERY) { fr29_acc_carry(w); cnt = 0; }
      }
      inner = mle_fr_acc_reduce(w);
    } else {
      const uint32_t* __restrict__ tab = static_cast<const uint32_t*>(T.p[g.by]);
      mle_acc a = mle_acc_zero();
      for (uint32_t r = r0; r < r1; r++) {
        const uint64_t i = ((uint64_t)r << lo_bits) + i_lo;
        if (i < e0 || i >= e1) continue;
        mle_acc_add_u32(a, tab[i - e0], fr29_unpack_u(hi[r])); any = true;
        if (++cnt == MLE_FOLD_EVERY) { mle_acc_fold(a); cnt = 0; }
      }
      mle_acc_fold(a);
      inner = mle_acc_reduce(a);
    }
    if (any) e[0] = fr29_mul(inner, fr29_unpack_u(lo[i_lo]));
  }
  // block sums through result_store, the last workgroup of a table adds them (cubic_epilogue: a single-workgroup table writes its result directly); shift 10: see Radix
  cubic_epilogue(e, g, partials, counters, out, flag, seq, S, 10, 1);
}
