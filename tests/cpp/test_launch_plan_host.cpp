// lasso_amd/csrc/launch_plan.cuh: which kernel serves a shape, its grid and its scratch.  The plan functions against a LITERAL restatement of the conditions lasso_hip.hip carried
// inline before the plans existed — the `if` chain of run_msm, the branches of cubic_eqw_launch_t, both parsers of LASSO_MSM_DIRECT_WGS — field for field, on both sides of every
// boundary those conditions hold: 16/17, 31/32, 255/256, 1023/1024 rows; W <= 4; n_cols * W8 <= 8192; 511/512 columns; K == 1; 64 indices per circuit; ell 14/15; nx <= DIRECT_NX.
// And the invariants the kernels rely on: chunks cover the columns, waves cover the rows, the point scratch covers whichever plan is chosen, the round scratch covers partials
// plus factor tables.  (The restatements below are frozen: they are what the plans must keep computing, not a second implementation to be kept in step.)
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "../../lasso_amd/csrc/device_switches.cuh"
#include "../../lasso_amd/csrc/launch_plan.cuh"

static long checks = 0;
#define CHECK(c) do { checks++; if (!(c)) { printf("FAIL line %d: %s\n", __LINE__, #c); return 1; } } while (0)

// ------------------------------------------------------------------ the MSMs as run_msm / run_msm_direct / bullet_round_fused had them
static size_t old_direct_wgs(const char* v) { const long x = v ? atol(v) : 0; return (size_t)(x >= 1 && x <= 4096 ? x : 256); }    // msm_direct_chunks' parser
static size_t old_bullet_wgs(const char* v) { const long x = v ? atol(v) : 0; return (size_t)(x >= 4 && x <= 4096 ? x : 256); }    // bullet_round_fused's
static size_t old_msm_chunks(size_t rows, size_t n_cols, uint32_t W) {
  size_t pairs = n_cols * W, K = 1;
  if (rows < 256) { K = 256 / rows; size_t kmax = (pairs + 1023) / 1024; if (kmax < 1) kmax = 1; if (K > kmax) K = kmax; }
  size_t cols_per_chunk = (n_cols + K - 1) / K;
  return (n_cols + cols_per_chunk - 1) / cols_per_chunk;
}
static size_t old_msm_direct_chunks(size_t rows, size_t n_cols, uint32_t* items_per_chunk, size_t wgs, size_t windows = 64) {
  const size_t total = n_cols * windows;
  size_t K = wgs / rows; if (K < 1) K = 1;
  size_t ipc = ((total + K - 1) / K + 255) / 256 * 256;
  const size_t ipc_max = windows * 128;
  if (ipc > ipc_max) ipc = ipc_max;
  *items_per_chunk = (uint32_t)ipc;
  return (total + ipc - 1) / ipc;
}
static size_t old_msm_pts_bytes(size_t rows, size_t n_cols, size_t wgs) {
  uint32_t ipc; const size_t kd = rows <= 16 ? old_msm_direct_chunks(rows, n_cols, &ipc, wgs) : 0, kb = old_msm_chunks(rows, n_cols, 64);
  return (rows * (kd > kb ? kd : kb) + 2 * rows + 4) * 144 + 512;
}
struct Env { bool direct, rows8, rows8w, full8, pip; size_t waves, min_cols, mb; };
struct OldMsm { MsmKernel kernel; MsmResult result; size_t K, cpc; uint32_t W8; size_t rpw, waves, pip_items, pip_row_bytes, pip_group; double adds; };
// tab8_builds / pip_allocs: what ensure_tab8 / ensure_pip answer
static OldMsm old_run_msm(uint32_t bps, uint32_t W, size_t rows, size_t n_cols, bool compressed, bool d_rows_out, size_t bn, bool d_mult, bool d_mult8, bool tab8_builds, bool pip_allocs, const Env& e) {
  OldMsm o = {};
  bool out_compressed = compressed;
  if (d_rows_out) out_compressed = true;
  o.result = d_rows_out ? MSM_R_DEVICE_ROWS : out_compressed ? (rows <= ((size_t)1 << 16) ? MSM_R_COMPRESSED_MAPPED : MSM_R_COMPRESSED_MEMCPY) : rows <= 16 ? MSM_R_FLAG : MSM_R_MEMCPY;
  if (bps == 32 && rows <= 16 && !out_compressed && d_mult && e.direct) { o.kernel = MSM_K_DIRECT; return o; }
  const size_t K = old_msm_chunks(rows, n_cols, W);
  const size_t cols_per_chunk = (n_cols + K - 1) / K;
  bool t8[2] = {false, false};
  const uint32_t W8 = (W + 1) / 2;
  if (bps == 4 && W <= 4 && rows >= 32 && e.rows8) { t8[0] = tab8_builds; t8[1] = W8 > 1 && t8[0] ? tab8_builds : t8[0]; if (!t8[1]) t8[0] = false; }
  const bool full8 = bps == 32 && d_mult8 && e.full8 && !t8[0];
  size_t pip_group = 0, pip_row_bytes = 0, pip_items = 0;
  if (bps == 32 && e.pip && !full8 && K == 1 && rows >= 256 && n_cols >= e.min_cols && n_cols < ((size_t)1 << 26) && bn * 64 < ((size_t)1 << 31)) {
    pip_items = n_cols * 21;
    pip_row_bytes = ((pip_items * 4 + (2048 + 1) * 4 + 2048 * 2 + 2048 * (size_t)144 + n_cols) + 255) & ~(size_t)255;
    pip_group = (e.mb << 20) / pip_row_bytes; if (pip_group < 64) pip_group = 64; if (pip_group > rows) pip_group = rows;
    if (!pip_allocs) pip_group = 0;
  }
  o.adds = (double)rows * n_cols * (t8[0] ? W8 : full8 ? 32 : pip_group ? 21 : W);
  const size_t rpw = e.waves ? (rows + e.waves - 1) / e.waves : 1, waves = (rows + rpw - 1) / rpw;
  if (t8[0] && e.rows8w && K == 1 && rows >= 1024 && n_cols * W8 <= 8192) o.kernel = MSM_K_ROWS8W;
  else if (t8[0]) o.kernel = MSM_K_ROWS8;
  else if (pip_group) o.kernel = MSM_K_PIP;
  else if (full8) o.kernel = MSM_K_FULL8;
  else o.kernel = MSM_K_BUCKETS;
  o.K = K; o.cpc = cols_per_chunk; o.W8 = W8; o.rpw = rpw; o.waves = waves; o.pip_items = pip_items; o.pip_row_bytes = pip_row_bytes; o.pip_group = pip_group;
  return o;
}
// run_msm's use of the plan: the two wishes, plan again where one is refused
static MsmPlan plan_as_run_msm(const MsmShape& s, MsmHave have, const MsmSwitches& sw, bool tab8_builds, bool pip_allocs) {
  MsmPlan p = msm_plan(s, have, sw);
  if (p.kernel == MSM_K_ROWS8W || p.kernel == MSM_K_ROWS8) { if (!tab8_builds) { have.tab8 = false; p = msm_plan(s, have, sw); } }
  else if (p.kernel == MSM_K_PIP && !pip_allocs) { have.pip_scratch = false; p = msm_plan(s, have, sw); }
  return p;
}
static int test_msm() {
  const size_t ROWS[] = {1, 2, 16, 17, 31, 32, 255, 256, 1023, 1024, 2049}, COLS[] = {1, 5, 64, 128, 129, 511, 512, 2048, 4096, 8192, 8193, 16384};
  const uint32_t WS[] = {1, 2, 4, 5, 64};
  for (size_t rows : ROWS) for (size_t n_cols : COLS) for (uint32_t bps : {4u, 32u}) for (uint32_t W : WS)
  for (int tables = 0; tables < 16; tables++) for (int bools = 0; bools < 32; bools++) for (size_t min_cols : {(size_t)32, (size_t)512}) for (size_t mb : {(size_t)16, (size_t)1200})
  for (size_t wv : {(size_t)0, (size_t)2048}) for (int outm = 0; outm < 3; outm++) for (size_t bn : {(size_t)16386, (size_t)1 << 25}) {
    if (bn != 16386 && !(bps == 32 && (bools & 16) && rows >= 256)) continue;   // the generator count only enters through the 12-bit-window kernels' index bound
    const bool d_mult = tables & 1, d_mult8 = tables & 2, tab8_builds = tables & 4, pip_allocs = tables & 8, compressed = outm & 1, dev_rows = outm & 2;
    const Env e = {(bools & 1) != 0, (bools & 2) != 0, (bools & 4) != 0, (bools & 8) != 0, (bools & 16) != 0, wv, min_cols, mb};
    const MsmSwitches sw = {e.direct, e.rows8, e.rows8w, e.full8, e.pip, wv, min_cols, mb, 0};
    const MsmShape s = {bps, W, rows, n_cols, compressed, dev_rows};
    const MsmHave have = {bn, d_mult, d_mult8, true, true};
    const OldMsm o = old_run_msm(bps, W, rows, n_cols, compressed, dev_rows, bn, d_mult, d_mult8, tab8_builds, pip_allocs, e);
    const MsmPlan p = plan_as_run_msm(s, have, sw, tab8_builds, pip_allocs);
    CHECK(p.kernel == o.kernel); CHECK(p.result == o.result);
    if (o.kernel == MSM_K_DIRECT) continue;
    CHECK(p.K == o.K); CHECK(p.cols_per_chunk == o.cpc); CHECK(p.W8 == o.W8); CHECK(p.rpw == o.rpw); CHECK(p.waves == o.waves); CHECK(p.pip_group == o.pip_group); CHECK(p.adds == o.adds);
    if (o.kernel == MSM_K_PIP) { CHECK(p.pip_items == o.pip_items); CHECK(p.pip_row_bytes == o.pip_row_bytes); CHECK(p.pip_group >= (rows < 64 ? rows : 64) && p.pip_group <= rows); }
    CHECK(p.K * p.cols_per_chunk >= n_cols); CHECK(p.rpw * p.waves >= rows);
    // the scratch the callers reserve behind the scalars (they pass W <= MSM_WINDOWS): chunk partials, 16-byte-aligned row sums as pt29, 16-byte-aligned wire bytes
    if (W <= 64) CHECK(msm_pts_bytes(rows, n_cols, 256) >= rows * p.K * 144 + 15 + rows * 144 + 15 + rows * 32);
  }
  // the latency-shaped forms, with every spelling of LASSO_MSM_DIRECT_WGS
  const char* WGS[] = {nullptr, "1", "3", "4", "64", "4096", "4097"};
  for (const char* v : WGS) {
    const long parsed = v ? atol(v) : 0L;   // dsw::msm_direct_wgs()
    CHECK(msm_direct_wgs(parsed) == old_direct_wgs(v)); CHECK(bullet_wgs(parsed) == old_bullet_wgs(v));
    for (size_t rows : {(size_t)1, (size_t)2, (size_t)16}) for (size_t n_cols : COLS) for (bool mult8 : {false, true}) {
      const size_t windows = mult8 ? 32 : 64; uint32_t ipc = 0;
      const size_t K = old_msm_direct_chunks(rows, n_cols, &ipc, old_direct_wgs(v), windows);
      const MsmDirectPlan d = msm_direct_plan(rows, n_cols, mult8, parsed);
      CHECK(d.K == K); CHECK(d.ipc == ipc); CHECK(d.windows == windows); CHECK(d.w8 == mult8); CHECK(d.adds == (double)rows * n_cols * windows); CHECK(d.ref_adds == msm_ref_adds(rows, n_cols, FR_MODULUS_BITS));
      CHECK(d.ipc % 256 == 0 && d.ipc <= windows * 128 && d.K * d.ipc >= n_cols * windows);
      CHECK(msm_pts_bytes(rows, n_cols, msm_direct_wgs(parsed)) == old_msm_pts_bytes(rows, n_cols, old_direct_wgs(v)));
      CHECK(msm_pts_bytes(rows, n_cols, msm_direct_wgs(parsed)) >= rows * d.K * 144);   // k_msm_direct's partial points
    }
    for (size_t n = 2; n <= ((size_t)1 << 20); n *= 2) for (size_t nk = 2; nk <= n; nk *= 2) for (uint32_t world : {1u, 2u, 8u}) for (bool w8 : {false, true}) {
      if (world > n) continue;
      // bullet_round_fused's chunking
      const size_t wgs = old_bullet_wgs(v);
      const size_t n_loc = n / world, cols = (nk / 2 >= world) ? n_loc / 2 : n_loc;
      const size_t windows = w8 ? 32 : 64;
      const size_t total = cols * windows, kmax = (wgs - 2) / 2;
      size_t ipc_ = (total + kmax - 1) / kmax; ipc_ = (ipc_ + windows - 1) / windows * windows; if (ipc_ < 256) ipc_ = 256; if (ipc_ > windows * 128) ipc_ = windows * 128;
      const uint32_t ipc = (uint32_t)ipc_; const size_t K = (total + ipc_ - 1) / ipc_;
      const BulletPlan b = bullet_plan(n, nk, world, w8, parsed);
      CHECK(b.K == K); CHECK(b.ipc == ipc); CHECK(b.windows == windows); CHECK(b.n_loc == n_loc); CHECK(b.w8 == w8);
      CHECK(b.ipc % windows == 0 && b.ipc >= 256 && b.ipc <= windows * 128 && b.K * b.ipc >= total);   // whole columns per chunk (a multiple of 256 only where the window count divides it)
    }
  }
  for (size_t rows : ROWS) for (size_t n_cols : COLS) for (uint32_t W : WS) CHECK(msm_chunks(rows, n_cols, W) == old_msm_chunks(rows, n_cols, W));
  return 0;
}

// ------------------------------------------------------------------ one cubic round as cubic_eqw_launch_t had it: what each of its launch sites passed
struct OldCubic {
  CubicForm form; const char* refusal; bool bind; size_t items; unsigned nx, ny; size_t part_elems, scratch_elems; bool direct, wide, gate, inkernel;
  CubicEq eq; bool gate_point, factors, factors_gated, eq_outer; uint32_t g_ell, g_hi, g_lo, pipe; bool nt;
};
static unsigned old_grid_for(size_t n, unsigned cap = 2048) { size_t g = (n + 256 - 1) / 256; if (g < 1) g = 1; if (g > cap) g = cap; return (unsigned)g; }
static unsigned old_cubic_nx_cap(unsigned ny, long e) { if (e > 0) return (unsigned)e; unsigned c = 512 / (ny ? ny : 1); return c < 64 ? 64 : c; }
static OldCubic old_cubic(size_t n, uint32_t ncirc, int NT, bool ahead, bool r, bool eqi, bool eqg, uint32_t eqg_ell, int gate_ell, uint32_t prof_mask, bool groups_out, bool tagged, const CubicSwitches& sw) {
  OldCubic o = {}; o.ny = ncirc; o.nx = 1;
  const unsigned direct_nx_max = sw.direct_nx;
#define OLD_RESULT_ARGS(nx_) o.direct = groups_out && tagged && (nx_) > 1 && (nx_) <= direct_nx_max
  if (ahead && (NT != 2 || n / 4 <= 64)) { o.form = CUBIC_REFUSED; o.refusal = "a round launched ahead of its challenge: two-sum streaming rounds only (more than 64 index quadruples per circuit)"; return o; }
  if (!r && !ahead) {
    const size_t half = n / 2; o.items = half;
    if (half <= 64) { o.form = CUBIC_SMALL; }   // k_cubic_eqw_small<false, NT>
    else {
      o.form = CUBIC_LB;
      const unsigned ny = ncirc, nx = old_grid_for(half, old_cubic_nx_cap(ny, sw.cubic_nx));
      const bool big_inline = sw.eq_inline_big;
      const bool gated = gate_ell >= 0, gbig = gated && gate_ell > 14;
      const uint32_t g_ell = gbig ? (uint32_t)gate_ell : eqg ? eqg_ell : 0, g_lo = g_ell / 2, g_hi = g_ell - g_lo;
      const size_t part_elems = (size_t)nx * ny * 3;
      o.nx = nx; o.part_elems = part_elems; o.scratch_elems = part_elems + ((eqg || gbig) ? ((size_t)1 << g_hi) + ((size_t)1 << g_lo) : 0);
      o.g_ell = g_ell; o.g_lo = g_lo; o.g_hi = g_hi;
      OLD_RESULT_ARGS(nx);
      const uint32_t pipe = sw.lb_pipeline ? 1u : 0u;
      if (gated && NT == 2) o.gate_point = true;   // k_gate_point
      if ((gbig || eqg) && NT == 2) { o.factors = true; o.factors_gated = gbig; /* k_eq_small2_mem : k_eq_small2 */ if (!big_inline) o.eq_outer = true; }
      if ((gbig || eqg) && NT == 2 && !big_inline) { o.eq = CUBIC_EQ_TABLE; o.pipe = pipe; }          // <2, false, TP, EqNone>, EN.gp = gate_gp
      else if (gated && NT == 2) {
        if (gbig) { o.eq = CUBIC_EQ_FACTORS; o.pipe = 1u; }                                            // <2, true, TP, EqGlobal>, G.gp = d_gpoint
        else { o.eq = CUBIC_EQ_GATED; o.pipe = 1u; }                                                   // <2, true, TP, EqInlineMem>
      } else if (eqg && NT == 2) { o.eq = CUBIC_EQ_FACTORS; o.pipe = 1u; }                             // <2, true, TP, EqGlobal>, G.gp = nullptr
      else if (NT == 3) { o.eq = CUBIC_EQ_TABLE; o.pipe = 0u; }                                        // <3, false, TP, EqNone>
      else if (eqi) { o.eq = CUBIC_EQ_LDS; o.pipe = 1u; }                                              // <2, true, TP, EqInline>
      else { o.eq = CUBIC_EQ_TABLE; o.pipe = pipe; o.nt = sw.lb_nt && pipe; }                          // <2, false, TP, EqNone, true> : <2, false, TP, EqNone>
    }
  } else if (ahead) {
    const size_t q = n / 4; o.form = CUBIC_FUSED; o.bind = true; o.items = q;
    const unsigned ny = ncirc, nx = old_grid_for(q, old_cubic_nx_cap(ny, sw.cubic_nx));
    o.nx = nx; o.part_elems = o.scratch_elems = (size_t)nx * ny * 3;
    OLD_RESULT_ARGS(nx);
    const unsigned inkernel_max = sw.ahead_inkernel_wgs;
    const bool bracketed = ((prof_mask >> LASSO_K_CUBIC) & 1u) && !(prof_mask & 0x40000000u);
    const bool inkernel = nx * ny <= inkernel_max && !bracketed;
    o.inkernel = inkernel; o.gate = !inkernel;   // k_gate
    o.wide = sw.wide;                             // k_cubic_eqw_fused<2, wide, TM, true>
  } else {
    const size_t q = n / 4; o.bind = true; o.items = q;
    if (q <= 64) { o.form = CUBIC_SMALL; }       // k_cubic_eqw_small<true, NT>
    else {
      o.form = CUBIC_FUSED;
      const unsigned ny = ncirc, nx = old_grid_for(q, old_cubic_nx_cap(ny, sw.cubic_nx));
      o.nx = nx; o.part_elems = o.scratch_elems = (size_t)nx * ny * 3;
      OLD_RESULT_ARGS(nx);
      o.wide = NT == 3 ? false : sw.wide;         // <3, false> : <2, true> : <2, false>
    }
  }
  return o;
}
static int test_cubic() {
  for (size_t n = 2; n <= ((size_t)1 << 20); n *= 2) for (uint32_t ncirc : {1u, 8u, 9u, 136u}) for (int NT : {2, 3}) for (int pres = 0; pres < 32; pres++) for (uint32_t ell : {0u, 9u, 14u, 15u, 32u})
  for (uint32_t prof_mask : {0u, 1u << LASSO_K_CUBIC, (1u << LASSO_K_CUBIC) | 0x40000000u}) for (long cnx : {0L, 64L}) for (unsigned dnx : {0u, 16u}) for (unsigned ik : {0u, 32u}) for (int sb = 0; sb < 16; sb++)
  for (int res = 0; res < 4; res++) {
    const bool r = pres & 1, eqi = pres & 2, eqg = pres & 4, ahead = pres & 8, gated = pres & 16, groups_out = res & 1, tagged = res & 2;
    const CubicSwitches sw = {cnx, (sb & 1) != 0, dnx, (sb & 2) != 0, (sb & 4) != 0, (sb & 8) != 0, ik};
    const OldCubic o = old_cubic(n, ncirc, NT, ahead, r, eqi, eqg, ell, gated ? (int)ell : -1, prof_mask, groups_out, tagged, sw);
    const CubicShape s = {n, ncirc, NT, ahead, r, eqi, eqg, eqg ? ell : 0u, gated ? (int)ell : -1, prof_mask, groups_out && tagged};
    const CubicPlan p = cubic_plan(s, sw);
    CHECK(p.form == o.form);
    if (o.form == CUBIC_REFUSED) { CHECK(p.refusal && !strcmp(p.refusal, o.refusal)); continue; }
    CHECK(p.bind == o.bind); CHECK(p.items == o.items); CHECK(p.nx == o.nx); CHECK(p.ny == o.ny); CHECK(p.part_elems == o.part_elems); CHECK(p.scratch_elems == o.scratch_elems);
    CHECK(p.direct == o.direct); CHECK(p.wide == o.wide); CHECK(p.gate == o.gate); CHECK(p.inkernel == o.inkernel);
    CHECK(p.lb.eq == o.eq); CHECK(p.lb.gate == o.gate_point); CHECK(p.lb.factors == o.factors); CHECK(p.lb.factors_gated == o.factors_gated); CHECK(p.lb.eq_outer == o.eq_outer);
    CHECK(p.lb.g_ell == o.g_ell); CHECK(p.lb.g_hi == o.g_hi); CHECK(p.lb.g_lo == o.g_lo); CHECK(p.lb.pipe == o.pipe); CHECK(p.lb.nt == o.nt);
    CHECK(p.scratch_elems >= (size_t)p.nx * p.ny * 3 * (p.form != CUBIC_SMALL) + (p.lb.factors ? ((size_t)1 << p.lb.g_hi) + ((size_t)1 << p.lb.g_lo) : 0));
    CHECK(p.nx >= 1);
    if (p.direct) CHECK(p.nx > 1 && p.nx <= dnx);
  }
  // the x-extent of the linear rounds (cubic_nx_cap / grid_for) and the resident tails' workgroup
  for (size_t items = 1; items <= ((size_t)1 << 22); items = items * 2 + (items & 1 ? 0 : 1)) for (unsigned ny : {0u, 1u, 2u, 8u, 9u, 32u, 136u}) for (long cnx : {-1L, 0L, 64L, 1000L})
    CHECK(round_nx(items, ny, cnx) == old_grid_for(items, old_cubic_nx_cap(ny, cnx)));
  // the reduction launches outside the round grids: grid_for(items, 1024 / 512 / 256) as each launch site had it, LASSO_REDUCE_NX in the cap's place where it is above 0
  for (size_t items = 1; items <= ((size_t)1 << 26); items = items * 2 + (items & 1 ? 0 : 1)) for (unsigned cap : {256u, 512u, 1024u}) for (long rnx : {-1L, 0L, 1L, 3L, 2000L})
    CHECK(reduce_nx(items, cap, rnx) == old_grid_for(items, rnx > 0 ? (unsigned)rnx : cap));
  // the row chunks of lasso_matvec_left / lasso_matvec_left_dev, as both had them
  for (size_t l_size : {(size_t)1, (size_t)2, (size_t)3, (size_t)320, (size_t)512, (size_t)1000, (size_t)4096, (size_t)5000}) for (size_t r_size : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)1024, (size_t)4096, (size_t)300000}) {
    size_t col_blocks = (r_size + 256 - 1) / 256;
    size_t nchunks = (1024 + col_blocks - 1) / col_blocks; if (nchunks > l_size) nchunks = l_size; if (nchunks < 1) nchunks = 1;
    size_t rows_per_chunk = (l_size + nchunks - 1) / nchunks; nchunks = (l_size + rows_per_chunk - 1) / rows_per_chunk;
    const MatvecPlan mp = matvec_plan(l_size, r_size);
    CHECK(mp.col_blocks == col_blocks && mp.nchunks == nchunks && mp.rows_per_chunk == rows_per_chunk);
    CHECK(mp.nchunks * mp.rows_per_chunk >= l_size && (mp.nchunks - 1) * mp.rows_per_chunk < l_size);
  }
  for (size_t q : {(size_t)1, (size_t)255, (size_t)256, (size_t)257, (size_t)512}) CHECK(tail_threads(q) == (q <= 256 ? 256u : 512u));
  CHECK(grid_for(0) == 1 && grid_for(257) == 2 && grid_for((size_t)1 << 40) == 2048 && grid_for(1 << 20, 4096) == 4096);
  return 0;
}

int main() {
  if (test_msm()) return 1;
  if (test_cubic()) return 1;
  // the switch table's helpers
  CHECK(lasso::dsw::unless0(nullptr) && lasso::dsw::unless0("1") && !lasso::dsw::unless0("0") && !lasso::dsw::if1(nullptr) && lasso::dsw::if1("1") && !lasso::dsw::if1("0"));
  // LASSO_SCRATCH_GUARD: default off; the guard's room is added to a capacity only with the switch on; the first damaged byte of a guard read back
  CHECK(!lasso::dsw::scratch_guard());   // the test runs without the variable
  CHECK(guard_alloc_bytes((size_t)1 << 22, false) == ((size_t)1 << 22) && guard_alloc_bytes((size_t)1 << 22, true) == ((size_t)1 << 22) + SCRATCH_GUARD_BYTES && SCRATCH_GUARD_BYTES >= ((size_t)64 << 10));
  {
    static uint8_t g[SCRATCH_GUARD_BYTES];
    memset(g, SCRATCH_GUARD_BYTE, sizeof(g)); CHECK(guard_first_damage(g) == SCRATCH_GUARD_BYTES);
    for (size_t at : {(size_t)0, (size_t)1, (size_t)4095, SCRATCH_GUARD_BYTES - 1}) { g[at] ^= 1; CHECK(guard_first_damage(g) == at); g[at] ^= 1; }
    g[7] = 0; g[9] = 0; CHECK(guard_first_damage(g) == 7);
  }
  // LASSO_POISON: default off; the word; the host fill (whole words, then the word's first bytes in memory order); which range a request fills
  CHECK(!lasso::dsw::poison());   // the test runs without the variable
  CHECK(lasso::dsw::POISON_WORD == 1u);   // non-zero as a value, a counter and a flag; as an index inside any table of two or more entries
  {
    alignas(4) uint8_t m[24];
    for (size_t bytes = 0; bytes <= 19; bytes++) {
      memset(m, 0xEE, sizeof(m)); lasso::dsw::poison_fill_host(m, bytes, lasso::dsw::POISON_WORD);
      for (size_t i = 0; i < sizeof(m); i++) CHECK(m[i] == (i >= bytes ? 0xEE : (i & 3) == 0 ? 1 : 0));
    }
    memset(m, 0xEE, sizeof(m)); lasso::dsw::poison_fill_host(m, 7, 0x04030201u);
    for (size_t i = 0; i < 7; i++) CHECK(m[i] == 1 + (i & 3)); CHECK(m[7] == 0xEE);
  }
  {
    const size_t cap = (size_t)1 << 22;
    for (int guard = 0; guard < 2; guard++) {
      // inside the capacity: the word that holds the request's last bytes is written whole, nothing beyond it
      for (size_t req : {(size_t)0, (size_t)1, (size_t)3, (size_t)4, (size_t)5, (size_t)129 * 7, (size_t)98 * 3, cap - 5, cap - 4, cap - 3, cap}) {
        const PoisonRange r = poison_range(req, cap, guard != 0, 0);
        CHECK(r.begin == 0 && r.tail_bytes == 0 && r.words == (req + 3) / 4 && 4 * r.words >= req && 4 * r.words < req + 4 && 4 * r.words <= cap);
      }
      // above the capacity: nothing (the buffer grows first, and its new allocation is filled as a whole)
      for (size_t req : {cap + 1, cap + 4, 2 * cap}) { const PoisonRange r = poison_range(req, cap, guard != 0, 0); CHECK(r.words == 0 && r.tail_bytes == 0); }
    }
    // a capacity of an odd size asked for whole (the scratch grows to exactly the request above its floor: 129 n and 98 n bytes): without the guard's room behind it the last
    // 1..3 bytes go out as bytes, with it as one more word, which the guard then overwrites
    for (size_t odd : {((size_t)1 << 22) + 1, ((size_t)1 << 22) + 2, ((size_t)1 << 22) + 3, (size_t)129 * 40001, (size_t)98 * 50001}) {
      const PoisonRange a = poison_range(odd, odd, false, 0), b = poison_range(odd, odd, true, 0);
      CHECK(a.words == odd / 4 && a.tail_bytes == (odd & 3) && 4 * a.words + a.tail_bytes == odd);
      CHECK(b.tail_bytes == 0 && b.words == (odd + 3) / 4 && 4 * b.words <= guard_alloc_bytes(odd, true) && 4 * b.words - odd < SCRATCH_GUARD_BYTES);
      const PoisonRange below = poison_range(odd - 4, odd, false, 0);   // ... and a request whose last word ends inside that capacity keeps the whole word
      CHECK(below.tail_bytes == 0 && 4 * below.words == ((odd - 4 + 3) & ~(size_t)3) && 4 * below.words <= odd);
    }
    // a later request of the same call (done > 0): nothing in front of `done` is touched, everything from the first word boundary at or behind it to the request's end is filled
    // (the bytes between `done` and that boundary went out with the earlier request's last word), and a request that is not larger fills nothing
    {
      const PoisonRange same = poison_range(4096, cap, false, 4096), smaller = poison_range(100, cap, true, 4096); CHECK(same.words == 0 && same.tail_bytes == 0 && smaller.words == 0 && smaller.tail_bytes == 0);
      const PoisonRange r = poison_range((size_t)32 * 1000 + 7, cap, false, (size_t)4 * 1000 + 256 + 3);   // 4 bytes per scalar, then 32: hyrax_commit_impl's two requests
      CHECK(r.begin == 4260 && r.tail_bytes == 0 && r.begin + 4 * r.words == 32008);
      const PoisonRange within = poison_range(4099, cap, false, 4097); CHECK(within.words == 0 && within.tail_bytes == 0);   // inside the word the earlier fill wrote whole
    }
    for (size_t c2 : {(size_t)8, (size_t)9, (size_t)10, (size_t)11, (size_t)131}) for (size_t done = 0; done <= c2; done++) for (size_t req = 0; req <= c2; req++) for (int guard = 0; guard < 2; guard++) {
      const size_t alloc = guard_alloc_bytes(c2, guard != 0);
      const PoisonRange first = poison_range(done, c2, guard != 0, 0), r = poison_range(req, c2, guard != 0, done);
      const size_t covered = done ? first.begin + 4 * first.words + first.tail_bytes : 0, end = r.begin + 4 * r.words + r.tail_bytes;   // where the earlier request's fill ended
      if (req <= done) { CHECK(r.words == 0 && r.tail_bytes == 0); continue; }
      if (r.words == 0 && r.tail_bytes == 0) { CHECK(covered >= req); continue; }       // nothing to do: the earlier fill reached past this request
      CHECK(r.begin >= done && r.begin <= covered && (r.words == 0 || r.begin % 4 == 0) && r.tail_bytes < 4 && end >= req && end <= alloc && (r.tail_bytes == 0 || end == req));
    }
    // every filled byte lies inside the allocation, and every requested byte is filled
    for (size_t c2 : {(size_t)1, (size_t)2, (size_t)7, (size_t)8, (size_t)4097}) for (size_t req = 0; req <= c2; req++) for (int guard = 0; guard < 2; guard++) {
      const PoisonRange r = poison_range(req, c2, guard != 0, 0);
      CHECK(r.tail_bytes < 4 && 4 * r.words + r.tail_bytes >= req && 4 * r.words + r.tail_bytes <= guard_alloc_bytes(c2, guard != 0) && (r.tail_bytes == 0 || 4 * r.words + r.tail_bytes == req));
    }
  }
  printf("OK %ld checks\n", checks);
  return 0;
}
