// Which kernel serves a shape, with what grid and how much scratch: every such decision of lasso_hip.hip as a pure function of the shape, of what the bases object has and of the
// switches (device_switches.cuh, passed in as values).  lasso_hip.hip reads a plan, allocates, switches on it and launches.  Plain C++17 — no HIP type, no context, no allocation:
// tests/cpp/test_launch_plan_host.cpp walks these functions on the CPU against a literal restatement of the conditions they replaced, on both sides of every boundary.
// The constants the decisions share with the kernels are defined here, once; poly_kernels.cuh includes this file.
#pragma once
#include <cstddef>
#include <cstdint>
#include "../../include/lasso_hip.h"   // lasso_kernel_id, LASSO_PROF_LARGE_ONLY

#define LASSO_BLOCK 256
#define CUBIC_SMALL_Q 64   // rounds with at most this many indices per circuit take the latency-shaped kernel
#define CUBIC_TAIL_Q 512   // the resident kernels take over at <= this many indices per circuit
#define MSM_THREADS 256
#define MSM_WINDOWS 64   // 4-bit windows over 256-bit scalars
#define MSM_PIP_WINDOWS 21            // bucket windows: bits 0 .. 251; what is left above them (bits 252 .. 255 plus the last carry: 0 .. 4 for a canonical scalar) is NOT a bucket digit:
                                      // half the scalars of a row have 1 there (the carry), and a bucket of 4096 pairs in a row of 88-pair buckets is one lane working alone for 35 ms (measured)
#define MSM_PIP_BUCKETS 2048
#define MSM_SMALL_ROWS 16   // results of up to this many rows return through the mapped buffer + flag (no memcpy, no stream sync)
#define MSM_PT29_BYTES 144   // sizeof(pt29), both curves (lasso_hip.hip asserts it)
#ifdef LASSO_BN254
#define FR_MODULUS_BITS 254u
#else
#define FR_MODULUS_BITS 253u
#endif
constexpr uint32_t msm_direct_windows(int wb) { return 256u / (uint32_t)wb; }   // MsmD<WB>::WINDOWS: windows of a scalar over the digit- (WB = 4) / byte-multiple (8) table

static inline unsigned grid_for(size_t n, unsigned cap = 2048) { size_t g = (n + LASSO_BLOCK - 1) / LASSO_BLOCK; if (g < 1) g = 1; if (g > cap) g = cap; return (unsigned)g; }
// every launch of the family is between profiling events: a wait for the host must not be inside them
static inline bool prof_bracketed(uint32_t prof_mask, int family) { return ((prof_mask >> family) & 1u) && !(prof_mask & (uint32_t)LASSO_PROF_LARGE_ONLY); }

// ------------------------------------------------------------------ the sumcheck rounds
// x-extent of the round grids: ~512 workgroups over the whole grid.  Inside a proof (random data, tools/gpu_sweep_roofline.sh) 512 total beats 1024 by 3-10% and 256 by 10%
// for both the cubic (ny = 2) and the linear (ny = 1) rounds, although in isolation on constant data 1024 is 6% faster (profiles/r01_microbench_v2.txt); the kernels are VALU-bound
// and every extra workgroup adds a reduction epilogue).  cubic_nx > 0 (LASSO_CUBIC_NX) overrides for experiments.  items: indices per circuit / polynomial the launch walks.
static inline unsigned round_nx(size_t items, unsigned ny, long cubic_nx) {
  unsigned cap = 512 / (ny ? ny : 1); if (cap < 64) cap = 64;
  return grid_for(items, cubic_nx > 0 ? (unsigned)cubic_nx : cap);
}
// x-extent of a one-dimensional reduction launch outside the round grids (combine rounds and claims, multi_dot, inner_products_lr): the launch's own cap, or reduce_nx_sw > 0
// (LASSO_REDUCE_NX) in its place.  Every one of these kernels strides by its grid, and its partials and second stage are sized from the same value.
static inline unsigned reduce_nx(size_t items, unsigned cap, long reduce_nx_sw) { return grid_for(items, reduce_nx_sw > 0 ? (unsigned)reduce_nx_sw : cap); }
// L * Z by row chunks (k_matvec_left, k_matvec_reduce): enough chunks of whole rows to fill the chip, ~1024 workgroups over the column blocks
struct MatvecPlan { size_t col_blocks, nchunks, rows_per_chunk; };
static inline MatvecPlan matvec_plan(size_t l_size, size_t r_size) {
  MatvecPlan p; p.col_blocks = (r_size + LASSO_BLOCK - 1) / LASSO_BLOCK;
  p.nchunks = (1024 + p.col_blocks - 1) / p.col_blocks; if (p.nchunks > l_size) p.nchunks = l_size; if (p.nchunks < 1) p.nchunks = 1;
  p.rows_per_chunk = (l_size + p.nchunks - 1) / p.nchunks; p.nchunks = (l_size + p.rows_per_chunk - 1) / p.rows_per_chunk;
  return p;
}
// workgroup = capacity of the two resident tails (k_cubic_tail, k_linear_tail): 256 threads / 74 KB of LDS up to 256 indices per circuit, 512 threads / 147 KB above
static inline unsigned tail_threads(size_t q) { return q <= 256 ? 256u : 512u; }

struct CubicSwitches { long cubic_nx; bool wide; unsigned direct_nx; bool eq_inline_big, lb_pipeline, lb_nt; unsigned ahead_inkernel_wgs; };
// One eq-weighted cubic round (cubic_eqw_launch_t).  has_r: the previous challenge is bound first; ahead: it will be, the launch waits for it on the device; has_eqi: the layer's
// point travels as a kernel argument (tables up to 2^14 entries, built in LDS); has_eqg / eqg_ell: the point of a larger table; gate_ell >= 0: the point comes through the point
// gate (the layer is enqueued ahead of it); direct_ok: the caller can take per-workgroup block sums (it passed groups_out, and the context hands results over tagged).
struct CubicShape { size_t n; uint32_t ncirc; int NT; bool ahead, has_r, has_eqi, has_eqg; uint32_t eqg_ell; int gate_ell; uint32_t prof_mask; bool direct_ok; };
enum CubicForm { CUBIC_REFUSED, CUBIC_SMALL, CUBIC_LB, CUBIC_FUSED };   // SMALL: one workgroup per circuit; LB: evaluation only; FUSED: bind, then the next round's sums
enum CubicEq {
  CUBIC_EQ_TABLE,     // the table is in d_E (EqNone) — where factors is set, the kernels in front of the round have just written it there
  CUBIC_EQ_LDS,       // built in LDS from the point in the arguments (EqInline), written to d_E on the way
  CUBIC_EQ_GATED,     // built in LDS from the point the gate left in memory (EqInlineMem)
  CUBIC_EQ_FACTORS    // the product of the two factor tables in memory, inside the round (EqGlobal)
};
// what an evaluation-only round (CUBIC_LB) adds: its eq source and what runs in front of it
struct CubicLbPlan {
  CubicEq eq;
  bool gate;            // k_gate_point in front: the launches behind it read the point (and whether it arrived) from d_gpoint
  bool factors;         // the two factor tables of 2^g_hi and 2^g_lo entries are built behind the partials in the scratch: by k_eq_small2_mem from the gated point (factors_gated), else by k_eq_small2
  bool factors_gated;
  bool eq_outer;        // k_eq_outer writes their product to d_E in front of the round
  uint32_t g_ell, g_hi, g_lo;
  uint32_t pipe;        // the kernel's `pipe` argument
  bool nt;              // the non-temporal instantiation
};
struct CubicPlan {
  CubicForm form; const char* refusal;   // refusal: the message of a CUBIC_REFUSED plan
  bool bind;              // the launch binds a challenge first: it walks n / 4 index quadruples per circuit, otherwise n / 2 pairs
  size_t items;           // ... that number
  unsigned nx, ny;        // the grid (nx * ny workgroups); SMALL: 1 x ncirc
  size_t part_elems;      // block partials in the scratch, and scratch_elems: the same plus the factor tables (field elements)
  size_t scratch_elems;
  bool direct;            // every workgroup's block sums go to the host (nx groups) instead of through the in-launch second stage
  bool wide;              // FUSED, two sums: double-width accumulators
  bool gate, inkernel;    // a FUSED round launched ahead: the wait in a k_gate launch in front of it, or inside the round's kernel
  CubicLbPlan lb;
};
static inline CubicPlan cubic_plan(const CubicShape& s, const CubicSwitches& sw) {
  CubicPlan p = {}; p.ny = s.ncirc; p.nx = 1;
  if (s.ahead && (s.NT != 2 || s.n / 4 <= CUBIC_SMALL_Q)) { p.form = CUBIC_REFUSED; p.refusal = "a round launched ahead of its challenge: two-sum streaming rounds only (more than 64 index quadruples per circuit)"; return p; }
  p.bind = s.has_r || s.ahead; p.items = p.bind ? s.n / 4 : s.n / 2;
  if (p.items <= CUBIC_SMALL_Q) { p.form = CUBIC_SMALL; return p; }   // (never a round launched ahead: refused above)
  p.form = p.bind ? CUBIC_FUSED : CUBIC_LB;
  p.nx = round_nx(p.items, p.ny, sw.cubic_nx);
  p.part_elems = p.scratch_elems = (size_t)p.nx * p.ny * 3;
  p.direct = s.direct_ok && p.nx > 1 && p.nx <= sw.direct_nx;
  if (p.bind) {
    p.wide = s.NT == 2 && sw.wide;
    if (s.ahead) { p.inkernel = p.nx * p.ny <= sw.ahead_inkernel_wgs && !prof_bracketed(s.prof_mask, LASSO_K_CUBIC); p.gate = !p.inkernel; }
    return p;
  }
  CubicLbPlan& l = p.lb;
  const bool gated = s.gate_ell >= 0, gbig = gated && s.gate_ell > 14;   // above 2^14 entries the table does not fit the in-LDS build: factor tables in memory
  l.g_ell = gbig ? (uint32_t)s.gate_ell : s.has_eqg ? s.eqg_ell : 0; l.g_lo = l.g_ell / 2; l.g_hi = l.g_ell - l.g_lo;
  if (s.has_eqg || gbig) p.scratch_elems += ((size_t)1 << l.g_hi) + ((size_t)1 << l.g_lo);
  if (s.NT != 2) { l.eq = CUBIC_EQ_TABLE; l.pipe = 0; return p; }   // the three-sum form reads its table, whatever else the caller passed
  l.gate = gated; l.factors = gbig || s.has_eqg; l.factors_gated = gbig; l.eq_outer = l.factors && !sw.eq_inline_big;
  l.eq = l.eq_outer ? CUBIC_EQ_TABLE : gated ? (gbig ? CUBIC_EQ_FACTORS : CUBIC_EQ_GATED) : s.has_eqg ? CUBIC_EQ_FACTORS : s.has_eqi ? CUBIC_EQ_LDS : CUBIC_EQ_TABLE;
  const bool plain = l.eq == CUBIC_EQ_TABLE;   // the rounds that write their table are always pipelined
  l.pipe = plain ? (sw.lb_pipeline ? 1u : 0u) : 1u;
  l.nt = plain && !l.eq_outer && sw.lb_nt && l.pipe;
  return p;
}

// ------------------------------------------------------------------ the MSMs
// group additions the REFERENCE's msm_bigint_wnaf (msm/mod.rs:91-164) performs for `rows` MSMs of n terms with num_bits-bit scalars:
// bucket accumulation n*W + bucket reduction W*2*2^c + window combine (W-1)*(c+1), c = ln_without_floats(n)+2 (:112-119,:322-325), W = ceil(num_bits/c).
// This is the algorithmic work unit of the MSM families' roofline (bench.py roofline_msm); the kernels here execute a different schedule
// (precomputed 4-bit window tables: one mixed addition per non-zero nibble, no per-window reduction, no doubling chain).
static inline double msm_ref_adds(size_t rows, size_t n, uint32_t num_bits) {
  size_t lg = n <= 1 ? 0 : 64 - (size_t)__builtin_clzll((unsigned long long)(n - 1));
  const size_t cw = n < 32 ? 3 : lg * 69 / 100 + 2, W = (num_bits + cw - 1) / cw;
  return (double)rows * ((double)n * W + (double)W * 2.0 * (double)((size_t)1 << cw) + (double)(W > 0 ? W - 1 : 0) * (cw + 1.0));
}
// chunks per row.  Measured on MI355X (profiles/): the bucket kernel is VALU-issue-bound even at one wave per SIMD (the 81 independent
// multiply-adds of a field product pipeline back to back), so extra workgroups beyond one per CU only multiply the fixed per-workgroup
// reduction tree (2 rows x 482 chunks ran 310 us, 2 x 129 ran 180 us).  Aim for rows*K = 256 workgroups, never below 1024 pairs a chunk.
static inline size_t msm_chunks(size_t rows, size_t n_cols, uint32_t W) {
  size_t pairs = n_cols * W, K = 1;
  if (rows < 256) { K = 256 / rows; size_t kmax = (pairs + 1023) / 1024; if (kmax < 1) kmax = 1; if (K > kmax) K = kmax; }
  size_t cols_per_chunk = (n_cols + K - 1) / K;
  return (n_cols + cols_per_chunk - 1) / cols_per_chunk;
}
// Workgroups of a latency-shaped launch: one per CU by default.  LASSO_MSM_DIRECT_WGS (dsw::msm_direct_wgs, the value as parsed) overrides it for tuning (more workgroups = shorter
// per-thread addition chains, a larger cross-workgroup tree): the BN254 build's additions cost ~2.5x the Edwards ones and its balance point has not been measured yet.
// Its two users accept different ranges: k_msm_direct takes any count from 1, k_bullet_msm needs two workgroups beside at least one chunk per row.
static inline size_t msm_direct_wgs(long parsed) { return (size_t)(parsed >= 1 && parsed <= 4096 ? parsed : 256); }
static inline size_t bullet_wgs(long parsed) { return (size_t)(parsed >= 4 && parsed <= 4096 ? parsed : 256); }
// latency-shaped path (k_msm_direct): rows <= MSM_SMALL_ROWS of full-width canonical scalars, results through the mapped buffer + flag.
// Chunking: the launch's workgroups over all rows, whole multiples of 256 items per workgroup (every thread the same number of mixed adds),
// at most windows * 128 items (128 columns of LDS-staged scalars).  Scratch after the scalars: rows * K partial points.
static inline size_t msm_direct_chunks(size_t rows, size_t n_cols, uint32_t* items_per_chunk, size_t wgs, size_t windows = MSM_WINDOWS) {
  const size_t total = n_cols * windows;
  size_t K = wgs / rows; if (K < 1) K = 1;
  size_t ipc = ((total + K - 1) / K + 255) / 256 * 256;
  const size_t ipc_max = windows * 128;   // 128 columns of LDS-staged scalars
  if (ipc > ipc_max) ipc = ipc_max;
  *items_per_chunk = (uint32_t)ipc;
  return (total + ipc - 1) / ipc;
}
// bytes of point scratch an MSM of `rows` x `n_cols` may need after its scalars (whichever kernel serves it)
static inline size_t msm_pts_bytes(size_t rows, size_t n_cols, size_t wgs) {
  uint32_t ipc; const size_t kd = rows <= MSM_SMALL_ROWS ? msm_direct_chunks(rows, n_cols, &ipc, wgs) : 0, kb = msm_chunks(rows, n_cols, MSM_WINDOWS);
  return (rows * (kd > kb ? kd : kb) + 2 * rows + 4) * MSM_PT29_BYTES + 512;
}
struct MsmDirectPlan { bool w8; size_t windows, K; uint32_t ipc; double ref_adds, adds; };   // w8: over the byte-multiple table (MsmD<8>), else the digit-multiple one; ref_adds / adds: ProfScope's work units
static inline MsmDirectPlan msm_direct_plan(size_t rows, size_t n_cols, bool mult8, long wgs_parsed) {
  MsmDirectPlan p = {}; p.w8 = mult8; p.windows = msm_direct_windows(mult8 ? 8 : 4);
  p.K = msm_direct_chunks(rows, n_cols, &p.ipc, msm_direct_wgs(wgs_parsed), p.windows);
  p.ref_adds = msm_ref_adds(rows, n_cols, FR_MODULUS_BITS); p.adds = (double)rows * n_cols * p.windows;
  return p;
}
// The fused bullet round (k_bullet_msm): K chunk workgroups per row over the longest row's local columns, plus one per row.  Chunks per row: (workgroups of the launch - 2 extra) / 2
// rows, items shared out evenly (a multiple of the window count keeps whole columns together).
struct BulletPlan { bool w8; size_t windows, n_loc, K; uint32_t ipc; };
static inline BulletPlan bullet_plan(size_t n, size_t nk, uint32_t world, bool mult8, long wgs_parsed) {
  BulletPlan p = {}; p.w8 = mult8; p.windows = msm_direct_windows(mult8 ? 8 : 4);
  p.n_loc = n / world; const size_t cols = (nk / 2 >= world) ? p.n_loc / 2 : p.n_loc;   // the longest row's local columns
  const size_t total = cols * p.windows, kmax = (bullet_wgs(wgs_parsed) - 2) / 2;
  size_t ipc = (total + kmax - 1) / kmax; ipc = (ipc + p.windows - 1) / p.windows * p.windows; if (ipc < 256) ipc = 256; if (ipc > p.windows * 128) ipc = p.windows * 128;
  p.ipc = (uint32_t)ipc; p.K = (total + ipc - 1) / ipc;
  return p;
}

struct MsmSwitches { bool direct, rows8, rows8w, full8, pip; size_t rows8w_waves, pip_min_cols, pip_scratch_mb; long direct_wgs; };
struct MsmShape { uint32_t bps, W; size_t rows, n_cols; bool compressed, dev_rows; };   // bps: bytes per scalar (4, 8: W nibbles populated, W <= 8 / 16; 32: full width; 8 is served by the bucket kernel alone — every other kernel asks for 4 or 32); compressed / dev_rows: wire bytes for the host / pt29 row sums left on the device
// n generators; the digit- and byte-multiple tables of the openings; tab8 / pip_scratch: false once the byte-window tables of the commitments (ensure_tab8) / the scratch of the
// 12-bit-window kernels (ensure_pip) have been asked for and refused
struct MsmHave { size_t n; bool mult, mult8, tab8, pip_scratch; };
enum MsmKernel { MSM_K_DIRECT, MSM_K_ROWS8W, MSM_K_ROWS8, MSM_K_PIP, MSM_K_FULL8, MSM_K_BUCKETS };
enum MsmResult {
  MSM_R_FLAG,                // up to MSM_SMALL_ROWS points through the mapped buffer behind the sequence flag
  MSM_R_COMPRESSED_MAPPED,   // wire bytes through the mapped buffer (up to 2^16 rows)
  MSM_R_COMPRESSED_MEMCPY,   // wire bytes by hipMemcpy
  MSM_R_DEVICE_ROWS,         // pt29 row sums copied to the caller's device buffer
  MSM_R_MEMCPY               // points by hipMemcpy
};
struct MsmPlan {
  MsmKernel kernel; MsmResult result;   // MSM_K_DIRECT: run_msm_direct takes the call (msm_direct_plan); the other fields are unset
  size_t K, cols_per_chunk; uint32_t W8;   // chunks per row; byte windows of the small scalars
  size_t rpw, waves;                    // ROWS8W: rows per wave, waves
  size_t pip_items, pip_row_bytes, pip_group;   // PIP: sorted pairs per row, scratch bytes per row, rows per pass
  double ref_adds, adds;                // ProfScope's work units: the reference's additions, the mixed additions the kernel issues at most
};
// ROWS8 / ROWS8W and PIP are wishes: run_msm calls ensure_tab8 / ensure_pip, and plans again with have.tab8 / have.pip_scratch = false where that fails (the bucket kernel serves)
static inline MsmPlan msm_plan(const MsmShape& s, const MsmHave& have, const MsmSwitches& sw) {
  MsmPlan p = {};
  const bool comp = s.compressed || s.dev_rows, small = s.rows <= MSM_SMALL_ROWS && !comp;
  p.result = s.dev_rows ? MSM_R_DEVICE_ROWS : s.compressed ? (s.rows <= ((size_t)1 << 16) ? MSM_R_COMPRESSED_MAPPED : MSM_R_COMPRESSED_MEMCPY) : small ? MSM_R_FLAG : MSM_R_MEMCPY;
  if (s.bps == 32 && small && have.mult && sw.direct) { p.kernel = MSM_K_DIRECT; return p; }
  p.K = msm_chunks(s.rows, s.n_cols, s.W); p.cols_per_chunk = (s.n_cols + p.K - 1) / p.K; p.W8 = (s.W + 1) / 2;
  p.rpw = sw.rows8w_waves ? (s.rows + sw.rows8w_waves - 1) / sw.rows8w_waves : 1; p.waves = (s.rows + p.rpw - 1) / p.rpw;
  // many rows of small scalars (<= 16 bits): one table entry per non-zero byte instead of nibble buckets
  const bool tab8 = s.bps == 4 && s.W <= 4 && s.rows >= 32 && sw.rows8 && have.tab8;
  // full-width scalars over the signed byte-multiple table (k_msm_rows_full: 32 additions per scalar, no buckets) — MEASURED AND NOT THE DEFAULT (round 6, LASSO_MSM_FULL8=1 turns
  // it on): Spark C=16 2^22's E commitment 198 ms against the bucket kernel's 182 ms.  Half the additions, but every one of them reads its own 128-byte line of a 4.3 GB table
  // (8194 generators x 32 windows x 128 multiples): 2.1e9 random line reads = 1.38 TB/s, the rate HBM serves random lines at; the bucket kernel's 64-window table is 67 MB and
  // stays in the Infinity Cache.  profiles/r06_full_width_commit_ab.txt
  const bool full8 = s.bps == 32 && have.mult8 && sw.full8 && !tab8;
  // many long rows of full-width scalars: 12-bit signed windows over the SAME nibble-window table, 2048 buckets per row, 22 additions per scalar instead of 60
  // (msm_kernels.cuh k_msm_pip_*; round 6).  Rows go through in groups that keep the scratch (sorted pairs 84 B per column, bucket sums 288 KB per row) near 1.2 GB
  // (LASSO_MSM_PIP_SCRATCH_MB).  From 256 rows of 512 columns on (measured, profiles/r06_full_width_commit_ab.txt: 512 x 512 0.69 against 1.12 ms, 1024 x 1024 1.86 against 3.70,
  // 4096 x 4096 23.5 against 47.9).  LASSO_MSM_PIP=0: the bucket kernel (A/B switch).  A refused allocation falls back to it as well.
  if (s.bps == 32 && sw.pip && !full8 && p.K == 1 && s.rows >= 256 && s.n_cols >= sw.pip_min_cols && s.n_cols < ((size_t)1 << 26) && have.n * MSM_WINDOWS < ((size_t)1 << 31) && have.pip_scratch) {
    p.pip_items = s.n_cols * MSM_PIP_WINDOWS;
    p.pip_row_bytes = ((p.pip_items * 4 + (MSM_PIP_BUCKETS + 1) * 4 + MSM_PIP_BUCKETS * 2 + (size_t)MSM_PIP_BUCKETS * MSM_PT29_BYTES + s.n_cols) + 255) & ~(size_t)255;
    p.pip_group = (sw.pip_scratch_mb << 20) / p.pip_row_bytes; if (p.pip_group < 64) p.pip_group = 64; if (p.pip_group > s.rows) p.pip_group = s.rows;
  }
  // many SHORT rows: one wave per row (k_msm_rows8w: 64 additions per lane and a 6-level tree inside the wave instead of 16 per thread and a 256-point tree).  Measured
  // (profiles/r04_ab_rows8w.txt): -9 % on the headline's E (4096 one-byte columns), -8 % on BN254 configs[1], +2 % on configs[2]'s 16384-column rows, where a thread of the
  // 256-lane kernel already runs 64 additions — hence the column bound.  Several rows per wave (round 6 experiment, NOT the default: LASSO_MSM_ROWS8W_WAVES=2048 caps a launch at
  // two waves per SIMD, all resident at once) measured 0.966 ms against 0.896 ms at one row per wave on the headline's E, profiles/r06_madd_bench_curve25519.txt section C: two
  // waves per SIMD hide less than three, the tail of the three-wave schedule costs less than that.
  p.kernel = tab8 ? (sw.rows8w && p.K == 1 && s.rows >= 1024 && s.n_cols * p.W8 <= 8192 ? MSM_K_ROWS8W : MSM_K_ROWS8) : p.pip_group ? MSM_K_PIP : full8 ? MSM_K_FULL8 : MSM_K_BUCKETS;
  p.ref_adds = msm_ref_adds(s.rows, s.n_cols, s.bps == 32 ? FR_MODULUS_BITS : 4 * s.W);
  p.adds = (double)s.rows * s.n_cols * (tab8 ? p.W8 : full8 ? 32 : p.pip_group ? MSM_PIP_WINDOWS : s.W);
  return p;
}

// ------------------------------------------------------------------ the MLE of caller-defined tables (lasso_tables_mle, mle_kernels.cuh)
// Entry i of a table of 2^log_m entries is (row i_hi, column i_lo), i = i_hi 2^lo_bits + i_lo, with the FIRST ceil(log_m / 2) coordinates of the point in the row factor:
// log_m = 1 and 2 leave the column factor with zero and one variable (a one-entry table [1] is a legal factor table).  A lane's task is one column i_lo over a run of
// rows_per_task rows, so a workgroup tile is 256 tasks; entries [e0, e1) of the table — a strip, or all of it — touch rows e0 >> lo_bits .. (e1 - 1) >> lo_bits.
// MLE_ROWS_PER_TASK rows per task where that fills at most MLE_MAX_NX workgroups per table; above that the runs grow instead, so the block sums stay within 2 MiB for 32 tables.
#define MLE_ROWS_PER_TASK 64u
#define MLE_MAX_NX 2048u
#define MLE_MAX_TABLES 32u
#define MLE_STRIP_BYTES ((size_t)64 << 20)   // the host form's strips, all tables together, unless LASSO_MLE_STRIP names a length
struct MlePlan { uint32_t hi_bits, lo_bits, row_first, rows, rows_per_task; uint64_t tasks; unsigned nx; };
static inline MlePlan mle_plan_rows(uint32_t log_m, uint32_t row_first, uint32_t rows) {
  MlePlan p; p.hi_bits = (log_m + 1) / 2; p.lo_bits = log_m - p.hi_bits;
  p.row_first = row_first; p.rows = rows;
  p.rows_per_task = MLE_ROWS_PER_TASK;
  const uint64_t max_runs = ((uint64_t)MLE_MAX_NX * LASSO_BLOCK) >> p.lo_bits;   // >= 16: lo_bits <= 15
  if (((uint64_t)p.rows + p.rows_per_task - 1) / p.rows_per_task > max_runs) p.rows_per_task = (uint32_t)(((uint64_t)p.rows + max_runs - 1) / max_runs);
  const uint64_t runs = ((uint64_t)p.rows + p.rows_per_task - 1) / p.rows_per_task;
  p.tasks = runs << p.lo_bits; p.nx = (unsigned)((p.tasks + LASSO_BLOCK - 1) / LASSO_BLOCK);
  return p;
}
static inline MlePlan mle_plan(uint32_t log_m, uint64_t e0, uint64_t e1) {
  const uint32_t lo_bits = log_m - (log_m + 1) / 2, row_first = (uint32_t)(e0 >> lo_bits);
  return mle_plan_rows(log_m, row_first, (uint32_t)((e1 - 1) >> lo_bits) + 1 - row_first);
}
// the widest grid any strip of `strip_len` entries can ask for: a strip that starts inside a row touches one row more than one that starts on a row boundary (nx grows with rows)
static inline unsigned mle_max_nx(uint32_t log_m, uint64_t strip_len) {
  const uint32_t hi_bits = (log_m + 1) / 2, lo_bits = log_m - hi_bits;
  uint64_t rows = ((strip_len + (((uint64_t)1 << lo_bits) - 1)) >> lo_bits) + 1; if (rows > ((uint64_t)1 << hi_bits)) rows = (uint64_t)1 << hi_bits;
  return mle_plan_rows(log_m, 0, (uint32_t)rows).nx;
}
// entries of every table per strip of the host form: strip_sw > 0 (LASSO_MLE_STRIP) as given, else what MLE_STRIP_BYTES holds for all tables, a multiple of 256, at least 256
static inline uint64_t mle_strip_len(uint32_t num_tables, size_t elem_bytes, long long strip_sw) {
  if (strip_sw > 0) return (uint64_t)strip_sw;
  uint64_t n = MLE_STRIP_BYTES / ((size_t)num_tables * elem_bytes); n &= ~(uint64_t)255; return n < 256 ? 256 : n;
}

// ------------------------------------------------------------------ the lookup values (lasso_lookup_values, values_kernels.cuh)
// A lane's item is TWO consecutive lookups in the integer kernels (`pair`: one 16-byte store in the 64-bit form, an odd n leaves the last item with one lookup) and one
// lookup in the term-list kernel.  Lanes walk the items grid-stride; VALUES_MAX_NX workgroups are 16 per compute unit, above that a lane takes several passes.
// values_nx_sw = LASSO_VALUES_NX (tests: a few workgroups bring several passes per lane within reach of small arrays).
#define VALUES_MAX_NX 4096u
struct ValuesPlan { uint32_t per_item; uint64_t items; unsigned nx; uint64_t passes, last_block_items; };
static inline ValuesPlan values_plan(size_t n, bool pair, long values_nx_sw) {
  ValuesPlan p; p.per_item = pair ? 2u : 1u;
  p.items = pair ? ((uint64_t)n + 1) / 2 : (uint64_t)n;
  p.nx = grid_for((size_t)p.items, values_nx_sw > 0 ? (unsigned)values_nx_sw : VALUES_MAX_NX);
  const uint64_t stride = (uint64_t)p.nx * LASSO_BLOCK;
  p.passes = (p.items + stride - 1) / stride;                      // of the busiest lane (lane 0 of workgroup 0)
  p.last_block_items = p.items % LASSO_BLOCK;                      // non-zero: the last tile of 256 items is ragged
  return p;
}

// ------------------------------------------------------------------ the guard behind the context's own buffers (LASSO_SCRATCH_GUARD, tests)
// Every request of the scratch, the sort buffer of the 12-bit-window kernels and the big-result buffer names its size as a hand-written sum of sub-buffers, and the buffers'
// floors (4 MiB of scratch) hide a sum that is too small at every shape a test runs.  With the switch on a buffer of capacity `cap` is allocated with SCRATCH_GUARD_BYTES more,
// and each request of `bytes` <= cap has the pattern at [bytes, bytes + SCRATCH_GUARD_BYTES): directly behind what was ASKED for, wherever the capacity ends.
#define SCRATCH_GUARD_BYTES ((size_t)64 << 10)
#define SCRATCH_GUARD_BYTE 0xA5
static inline size_t guard_alloc_bytes(size_t cap, bool guard) { return guard ? cap + SCRATCH_GUARD_BYTES : cap; }
// the first byte of a guard read back that no longer holds the pattern, or SCRATCH_GUARD_BYTES: intact
static inline size_t guard_first_damage(const uint8_t* g) { size_t i = 0; while (i < SCRATCH_GUARD_BYTES && g[i] == SCRATCH_GUARD_BYTE) i++; return i; }

// ------------------------------------------------------------------ the fill in front of a call's own data (LASSO_POISON, tests; device_switches.cuh POISON_WORD)
// A request a public call makes of the scratch, the sort buffer or the big-result buffer fills what it ASKED for and this call has not asked for before, [done, req), with the
// word in stream order: whatever the call reads from there it must have stored itself.  done = 0 at the call's first request of the buffer (all of [0, req) is filled); a later
// request of the same call leaves [0, done) alone — the call's own data may live there — and fills only what lies beyond (hyrax_commit_impl asks for 4 bytes per scalar first
// and for 32 when a scalar turns out wide).  The fill is issued as whole 32-bit words plus a tail of single bytes, every byte the one its position in the repeated word gives it.
// It starts at the first word boundary at or behind `done` (the bytes in front of it went out with the word that held the earlier request's last byte), and the word that
// holds this request's last bytes is written whole where it still lies inside the allocation (cap bytes, SCRATCH_GUARD_BYTES more with the guard on: guard_place then puts the
// guard over its last 1..3 bytes); where it does not — a request of an odd size that is the capacity itself, guard off — the tail goes out as bytes.  A request above the
// capacity fills nothing: the buffer grows first, and dmalloc has filled the new allocation.
struct PoisonRange { size_t begin, words, tail_bytes; };   // [begin, begin + 4 * words) as words, then tail_bytes (0..3) single bytes
static inline PoisonRange poison_range(size_t req, size_t cap, bool guard, size_t done) {
  PoisonRange r = {0, 0, 0};
  if (req > cap || req <= done) return r;
  const size_t alloc = guard_alloc_bytes(cap, guard), whole = (req + 3) & ~(size_t)3;
  r.begin = (done + 3) & ~(size_t)3;
  if (r.begin > alloc) { r.begin = done; r.tail_bytes = req - done; return r; }   // both requests end in the allocation's last, partial word: its remaining bytes one by one
  if (r.begin >= req) { r.begin = 0; return r; }                                 // ... in a word the earlier request's fill wrote whole
  if (whole <= alloc) r.words = (whole - r.begin) / 4;
  else { r.words = ((req & ~(size_t)3) - r.begin) / 4; r.tail_bytes = req & 3; }
  return r;
}
