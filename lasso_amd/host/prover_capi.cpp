// liblasso_prover.so — include/lasso_prover.h over lasso_amd/host/prover.hpp.  Nothing unwinds across the ABI.
#include "prover.hpp"
#include "verifier.hpp"
#include "shm_comm.hpp"
#include <atomic>
#include "../../include/lasso_prover.h"
#include "../../include/lasso_hip_wire.h"
#include "../../include/lasso_hip_msm.h"
#include "../../include/lasso_hip_operands.h"
#include "../../include/lasso_hip_gens.h"
#include "../../include/lasso_hip_mle.h"
#include "../../include/lasso_prover_mle.h"
#include "../../include/lasso_hip_values.h"
#include "../../include/lasso_prover_values.h"
#include "../csrc/values_combine.cuh"
#include "../../include/lasso_hip_poly.h"
#include "../../include/lasso_prover_poly.h"
#include "../../include/lasso_prover_polys.h"
#include "../../include/lasso_prover_blind.h"

using namespace lasso;

// ---- The optional parts of the device ABI, stated once.  Each is a header beside include/lasso_hip.h whose entry points are WEAK references here: null when these sources are
// linked against an implementation of lasso_hip.h alone.  The host then takes the route it had before the entry existed (named per line below), and a call that cannot do
// without the entry refuses in ext_unavailable's words.  Where the entry exists a switch (switches.hpp) can still keep the earlier route: the A/B handle.
// wire: the verifier decodes on the host.  LASSO_VERIFY_DEVICE_POINTS=0 keeps that; LASSO_WIRE_DEVICE_MIN = the smallest batch handed over (default: the smallest MEASURED ahead, profiles/verify_device_points.json)
extern "C" int32_t lasso_points_decompress(lasso_ctx*, const uint8_t*, size_t, lasso_affine*, uint8_t*, uint8_t*) __attribute__((weak));
// msm: the verifier's MSMs over commitment rows build a lasso_bases per call.  LASSO_VERIFY_MSM_POINTS=0 keeps that; no size threshold yet (tools/verify_bench.py --ab msm_points is what one would be set from)
extern "C" int32_t lasso_msm_points(lasso_ctx*, const lasso_affine*, const lasso_fr*, size_t, lasso_point*) __attribute__((weak));
// operands: lasso_host_densify_operands expands the operands to indices on the host and takes lasso_host_densify's path.  LASSO_DENSIFY_OPERANDS=0 does the same
extern "C" int32_t lasso_densify_dim_operands(lasso_ctx*, const uint64_t*, const uint64_t*, size_t, const lasso_operand_layout*, size_t, size_t, size_t, uint32_t, uint32_t, uint32_t, uint32_t*, lasso_fr*,
                                              lasso_fr*, lasso_fr*) __attribute__((weak));
// gens: lasso_host_gens_new builds every point on the host.  LASSO_GENS_DEVICE=0 keeps that; LASSO_GENS_DEVICE_MIN = the smallest set that goes over, LASSO_GENS_DEVICE_BATCH caps the candidates per call
extern "C" int32_t lasso_points_from_candidates(lasso_ctx*, const uint64_t*, const uint8_t*, size_t, lasso_affine*, uint8_t*) __attribute__((weak));
// mle: the verifier keeps its host loop (2^log_m products per subtable).  LASSO_VERIFY_DEVICE_MLE=0 keeps that; LASSO_MLE_DEVICE_MIN = the smallest num_subtables * 2^log_m that goes over
extern "C" int32_t lasso_tables_mle(lasso_ctx*, const uint32_t* const*, const lasso_fr* const*, uint32_t, uint32_t, const lasso_fr*, lasso_fr*) __attribute__((weak));
extern "C" int32_t lasso_tables_mle_dev(lasso_ctx*, const uint32_t* const*, const lasso_fr* const*, uint32_t, uint32_t, const lasso_fr*, lasso_fr*) __attribute__((weak));
// values: lasso_host_lookup_values refuses (lasso_host_lookup_values_ref needs no device); lasso_host_values_evaluate takes mle's entry for where its vector lives
extern "C" int32_t lasso_lookup_values(lasso_ctx*, const lasso_strategy*, const uint32_t* const*, const uint32_t* const*, const lasso_fr* const*, size_t, int32_t, void*) __attribute__((weak));
// poly: lasso_host_poly_commit / lasso_host_poly_open lift the integers on the host and take lasso_hyrax_commit_compressed / lasso_matvec_left_dev: the same bytes.  The three are used together or not at all
extern "C" int32_t lasso_u64_or(lasso_ctx*, const uint64_t*, size_t, uint64_t*) __attribute__((weak));
extern "C" int32_t lasso_hyrax_commit_compressed_u64(lasso_ctx*, const uint64_t*, uint64_t, size_t, size_t, const lasso_bases*, uint8_t*) __attribute__((weak));
extern "C" int32_t lasso_matvec_left_u64_dev(lasso_ctx*, const uint64_t*, const lasso_fr*, size_t, size_t, lasso_fr*) __attribute__((weak));

// One row per extension, under the name lasso_amd/_abi.py EXTENSIONS and the tests' mock (-DMOCK_EXT_<NAME>) know it by: its header, what a refusal calls the entry, whether
// the device library has it, and (lasso_host::ext_count) up to two counters that its lasso_host_*_stats reports.
enum Ext { EXT_WIRE, EXT_MSM_POINTS, EXT_OPERANDS, EXT_GENS, EXT_MLE, EXT_VALUES, EXT_POLY, EXT_COUNT };
static const struct { const char *name, *header, *what, *entry; bool (*available)(); } EXTS[EXT_COUNT] = {
  {"wire", "lasso_hip_wire.h", "the device decoder", "lasso_points_decompress", [] { return lasso_points_decompress != nullptr; }},                 // [0]: compressed points decoded on the device
  {"msm_points", "lasso_hip_msm.h", "the MSM over caller points", "lasso_msm_points", [] { return lasso_msm_points != nullptr; }},                // [0]: Verifier::msm_points calls that took it
  {"operands", "lasso_hip_operands.h", "the device entry", "lasso_densify_dim_operands", [] { return lasso_densify_dim_operands != nullptr; }},   // [0]: dimensions densified by it
  {"gens", "lasso_hip_gens.h", "the device entry", "lasso_points_from_candidates", [] { return lasso_points_from_candidates != nullptr; }},       // [0]: candidates handed to it
  {"mle", "lasso_hip_mle.h", "the device entry", "lasso_tables_mle", [] { return lasso_tables_mle != nullptr; }},                                 // [0]: caller-defined tables evaluated by it
  {"values", "lasso_hip_values.h", "the device entry", "lasso_lookup_values", [] { return lasso_lookup_values != nullptr; }},                     // [0]: elements it wrote
  {"poly", "lasso_hip_poly.h", "the device entry", "lasso_matvec_left_u64_dev", [] { return lasso_u64_or && lasso_hyrax_commit_compressed_u64 && lasso_matvec_left_u64_dev; }},   // [0], [1]: 64-bit elements committed to / opened
};
static Error ext_unavailable(const char* who, Ext e, const char* entry = nullptr) {
  return Error(std::string(who) + ": " + EXTS[e].what + " (" + (entry ? entry : EXTS[e].entry) + ", include/" + EXTS[e].header + ") is not available in the device library this host was linked against");
}

// Generator and dense-representation objects hold device buffers that belong to their host's context (DBuf keeps a `const Dev*`), so the host
// must outlive them: it is reference-counted by its children, and lasso_host_destroy only drops the caller's reference — the context goes away
// with the last child (Python's GC may release the three in any order).
struct lasso_host {
  Dev dev; std::atomic<int> refs{1};
  std::unique_ptr<ShmComm> shm;   // slab mode's native intra-node exchange (lasso_host_set_comm_shm); outlives every proof of this host
  uint64_t ext_count[EXT_COUNT][2] = {};   // the counters of EXTS' rows, for this host
  uint64_t polys_count[2] = {};            // lasso_host_polys_stats: vectors committed to / opened (no device entry of their own, so no row of EXTS)
  uint64_t blind_count[2] = {};            // lasso_host_blind_stats: rows blinded on the device / on the host (likewise)
  TablesMle tables_mle() { TablesMle m; if (lasso_tables_mle && sw::verify_device_mle()) { m.fn = &lasso_tables_mle; m.min_entries = sw::mle_device_min(); m.counter = ext_count[EXT_MLE]; } return m; }
  GensDevice gens_device() { GensDevice g; if (lasso_points_from_candidates && sw::gens_device()) { g.fn = &lasso_points_from_candidates; g.min_points = sw::gens_device_min(); g.batch = sw::gens_device_batch(); g.counter = ext_count[EXT_GENS]; } return g; }
  PointsMsm points_msm() { PointsMsm m; if (lasso_msm_points && sw::verify_msm_points()) { m.fn = &lasso_msm_points; m.counter = ext_count[EXT_MSM_POINTS]; } return m; }
  WireDecoder wire_decoder() { WireDecoder w; if (lasso_points_decompress && sw::verify_device_points()) { w.fn = &lasso_points_decompress; w.min_points = sw::wire_device_min(); w.counter = ext_count[EXT_WIRE]; } return w; }
  explicit lasso_host(int device) : dev(device) {}
  void retain() { refs.fetch_add(1, std::memory_order_relaxed); }
  void release() { if (refs.fetch_sub(1, std::memory_order_acq_rel) == 1) delete this; }
};
struct lasso_host_gens {
  lasso_host* owner; std::unique_ptr<SparsePolyCommitmentGens> g;
  lasso_host_gens(lasso_host* h, const char* label, size_t c, size_t s, size_t nm, size_t log_m) : owner(h) { g.reset(new SparsePolyCommitmentGens(h->dev, label, c, s, nm, log_m, h->gens_device())); h->retain(); }
  lasso_host_gens(lasso_host* h, size_t c, size_t s, size_t nm, size_t log_m, const lasso_affine* p1, size_t n1, const lasso_affine* p2, size_t n2, const lasso_affine* p3, size_t n3) : owner(h) {
    g.reset(new SparsePolyCommitmentGens(h->dev, c, s, nm, log_m, p1, n1, p2, n2, p3, n3)); h->retain();
  }
  ~lasso_host_gens() { g.reset(); owner->release(); }
};
struct lasso_host_dense {
  lasso_host* owner; std::unique_ptr<DensifiedRepresentation> d;
  explicit lasso_host_dense(lasso_host* h) : owner(h) { h->retain(); }
  ~lasso_host_dense() { d.reset(); owner->release(); }
};
struct lasso_host_poly_gens {
  lasso_host* owner; std::unique_ptr<PolyCommitmentGens> g; size_t num_vars;
  lasso_host_poly_gens(lasso_host* h, size_t nv) : owner(h), num_vars(nv) { h->retain(); }
  ~lasso_host_poly_gens() { g.reset(); owner->release(); }
};

static thread_local std::string g_err;
#define GUARD(...) try { __VA_ARGS__ } catch (const std::exception& e) { g_err = e.what(); return -1; } catch (...) { g_err = "unknown error"; return -1; }
static int32_t emit(const std::vector<uint8_t>& b, uint8_t* out, size_t cap, size_t* len) { if (len) *len = b.size(); if (!out || b.size() > cap) { g_err = "output buffer too small"; return -2; } memcpy(out, b.data(), b.size()); return 0; }
// `n` scalars of the caller's, memory form, any representative -> Sc
static ScVec scalars_in(const lasso_fr* v, size_t n) { ScVec out; out.reserve(n); for (size_t i = 0; i < n; i++) out.push_back(Sc::from_abi(v[i])); return out; }
// every lasso_host_*_stats: a pair of this host's counters (c1 only where the call reports two) and the reset; e != EXT_COUNT: whether the device library has that extension
static int32_t pair_stats(const char* who, lasso_host* h, uint64_t (lasso_host::*pair)[2], Ext e, uint64_t* c0, uint64_t* c1, int32_t* available, int32_t reset) {
  GUARD(
    if (!h) throw Error(std::string(who) + ": null host");
    uint64_t* c = pair ? h->*pair : h->ext_count[e];
    if (c0) *c0 = c[0];
    if (c1) *c1 = c[1];
    if (available) *available = EXTS[e].available() ? 1 : 0;
    if (reset) c[0] = c[1] = 0;
    return 0;)
}
static int32_t ext_stats(const char* who, lasso_host* h, Ext e, uint64_t* c0, uint64_t* c1, int32_t* available, int32_t reset) { return pair_stats(who, h, nullptr, e, c0, c1, available, reset); }

extern "C" {
const char* lasso_host_last_error(void) { return g_err.c_str(); }
// The library may have been built with -march=x86-64-v3 (lasso_amd/build.py host_march_flags): refuse, with a message, to run on a CPU without those extensions — the alternative
// is a SIGILL somewhere inside the first Keccak permutation.  This function itself must not need them: it is compiled for the baseline ISA.
#if defined(LASSO_HOST_V3) && defined(__x86_64__)
__attribute__((target("arch=x86-64"))) static bool host_cpu_ok() { __builtin_cpu_init(); return __builtin_cpu_supports("avx2") && __builtin_cpu_supports("bmi2") && __builtin_cpu_supports("fma"); }
#else
static bool host_cpu_ok() { return true; }
#endif
int32_t lasso_host_create(int32_t device, lasso_host** out) {
  if (!host_cpu_ok()) { g_err = "liblasso_prover was built with -march=x86-64-v3 (AVX2 / BMI2 / FMA) and this CPU lacks them: rebuild with LASSO_HOST_MARCH=none"; return -1; }
  GUARD(*out = new lasso_host(device); return 0;)
}
void lasso_host_destroy(lasso_host* h) { if (h) h->release(); }
lasso_ctx* lasso_host_ctx(lasso_host* h) { return h ? h->dev.ctx : nullptr; }
int32_t lasso_host_mem_stats(lasso_host* h, uint64_t* live_bytes, uint64_t* peak_bytes, uint64_t* prover_peak_bytes, int32_t reset) {
  GUARD(if (!h) throw Error("lasso_host_mem_stats: null host"); h->dev.mem_stats(live_bytes, peak_bytes, prover_peak_bytes, reset != 0); return 0;)
}
int32_t lasso_host_set_capacity(lasso_host* h, int32_t on) { GUARD(if (!h) throw Error("lasso_host_set_capacity: null host"); h->dev.capacity = on != 0; if (on) h->dev.trim(); return 0;) }
int32_t lasso_host_set_throughput_mode(lasso_host* h, int32_t on) { GUARD(if (!h) throw Error("lasso_host_set_throughput_mode: null host"); h->dev.throughput = on != 0; return 0;) }
int32_t lasso_host_set_comm(lasso_host* h, int32_t rank, int32_t world, lasso_host_allgather_fn fn, void* user) {
  GUARD(
    if (!h || world < 1 || (world & (world - 1)) || rank < 0 || rank >= world || (world > 1 && !fn)) throw Error("lasso_host_set_comm: world must be a power of two, 0 <= rank < world, and a collective is needed when world > 1");
    h->dev.comm.rank = (size_t)rank; h->dev.comm.world = (size_t)world; h->dev.comm.fn = fn; h->dev.comm.user = user; return 0;)
}
// Slab mode with the library's own exchange: the ranks of one node meet in a POSIX shared-memory segment `name` (same on every rank, e.g. derived from
// MASTER_PORT) and all-gather their per-round partial sums there (shm_comm.hpp) — no callback into the embedding language per round.
int32_t lasso_host_set_comm_shm(lasso_host* h, int32_t rank, int32_t world, const char* name) {
  GUARD(
    if (!h || !name || world < 1 || (world & (world - 1)) || rank < 0 || rank >= world) throw Error("lasso_host_set_comm_shm: world must be a power of two and 0 <= rank < world");
    h->shm.reset(new ShmComm(name, rank, world));
    h->dev.comm.rank = (size_t)rank; h->dev.comm.world = (size_t)world; h->dev.comm.fn = &ShmComm::trampoline; h->dev.comm.user = h->shm.get();
    // The bulk exchange (partial row commitments) goes over RCCL on the device stream when every rank can join one communicator: rank 0 draws the
    // unique id and publishes it through the segment; the ranks then agree (an all-gather of one status byte) — all use RCCL or none does.
    // Agreement protocol (every step an all-gather through the segment, so no rank can be left inside a collective its peers never enter):
    //   1. every rank publishes whether IT can use RCCL at all (librccl loads, LASSO_SLAB_RCCL != 0) — ncclCommInitRank is only entered if ALL can;
    //   2. rank 0 draws the unique id and publishes it with its status — the others read it, and all enter ncclCommInitRank or none does;
    //   3. every rank publishes its ncclCommInitRank outcome — the communicator is kept only if it came up on every rank.
    const bool rccl_on = sw::slab_rccl();
    if (world > 1) {
      auto all_ok = [&](uint8_t mine, const char* what) {
        std::vector<uint8_t> all((size_t)world, 0);
        if (h->shm->allgather(&mine, all.data(), 1) != 0) throw Error(std::string("lasso_host_set_comm_shm: ranks did not agree on ") + what);
        bool every = true; for (uint8_t v : all) every = every && v; return every;
      };
      const uint8_t can = (rccl_on && lasso_rccl_available() == 1) ? 1 : 0;
      if (all_ok(can, "RCCL availability")) {
        uint8_t blob[129] = {0};
        if (rank == 0) blob[128] = lasso_rccl_unique_id(blob) == 0 ? 1 : 0;
        h->shm->broadcast_blob(blob, sizeof(blob));
        if (blob[128]) {     // the same byte on every rank: all enter the collective init, or none
          const uint8_t mine = lasso_rccl_init(h->dev.ctx, rank, world, blob) == 0 ? 1 : 0;
          if (!all_ok(mine, "the device-side exchange")) { if (mine) (void)lasso_rccl_shutdown(h->dev.ctx); }
          else {
            //   4. first contact: every rank all-gathers 1 KB through the new communicator and checks every slot (lasso_rccl_selftest, bounded wait); the communicator is kept only
            //      if that worked on EVERY rank — otherwise the fall-back is announced on stderr, not silent (a node where xGMI / RCCL is half-configured must say so once)
            const uint8_t st = lasso_rccl_selftest(h->dev.ctx) == 0 ? 1 : 0;
            if (!st) fprintf(stderr, "[lasso] rank %d: RCCL self-test failed (%s) — slab mode falls back to the shared-memory exchange of partial row commitments\n", rank, lasso_last_error(h->dev.ctx));
            if (!all_ok(st, "the RCCL self-test")) { if (lasso_rccl_ready(h->dev.ctx)) (void)lasso_rccl_shutdown(h->dev.ctx); if (st) fprintf(stderr, "[lasso] rank %d: a peer's RCCL self-test failed — shared-memory exchange on every rank\n", rank); }
          }
        }
      }
    }
    return 0;)
}
int32_t lasso_host_gens_new(lasso_host* h, const char* label, size_t c, size_t s, size_t nm, size_t log_m, lasso_host_gens** out) { GUARD(*out = new lasso_host_gens(h, label, c, s, nm, log_m); return 0;) }
int32_t lasso_host_gens_from_points(lasso_host* h, size_t c, size_t s, size_t nm, size_t log_m, const lasso_affine* l_variate, size_t n_l, const lasso_affine* log_m_variate, size_t n_m,
                                    const lasso_affine* derefs, size_t n_d, lasso_host_gens** out) {
  GUARD(if (!h || !out) throw Error("lasso_host_gens_from_points: null argument"); *out = new lasso_host_gens(h, c, s, nm, log_m, l_variate, n_l, log_m_variate, n_m, derefs, n_d); return 0;)
}
int32_t lasso_host_gens_points(lasso_host_gens* g, int32_t which, lasso_affine* out, size_t cap, size_t* count) {
  GUARD(
    if (!g || !count) throw Error("lasso_host_gens_points: null argument");
    const PolyCommitmentGens& pg = g->g->set(which);
    *count = pg.affine.size();
    if (!out || cap < pg.affine.size()) { g_err = "output buffer too small"; return -2; }
    memcpy(out, pg.affine.data(), pg.affine.size() * sizeof(lasso_affine)); return 0;)
}
// every table a proof over these generators reads, built now: the byte-multiple tables of the small-scalar commitments (dim / read / final: two byte windows; E: one) are otherwise
// built by the first lasso_host_commit / lasso_host_prove that meets the object — inside whatever span the caller times
int32_t lasso_host_gens_prepare(lasso_host_gens* g) {
  GUARD(
    if (!g) throw Error("lasso_host_gens_prepare: null argument");
    for (int which = 0; which < 3; which++) {
      const PolyCommitmentGens& pg = g->g->set(which);
      if (pg.bases) pg.dev->chk(lasso_bases_prepare(pg.dev->ctx, pg.bases, 2), "lasso_bases_prepare");
      if (pg.bases_slab) pg.dev->chk(lasso_bases_prepare(pg.dev->ctx, pg.bases_slab, 2), "lasso_bases_prepare");
    }
    return 0;)
}
void lasso_host_gens_free(lasso_host_gens* g) { delete g; }
int32_t lasso_host_densify(lasso_host* h, const uint64_t* indices, size_t n, size_t c, size_t log_m, lasso_host_dense** out) {
  GUARD(std::unique_ptr<lasso_host_dense> d(new lasso_host_dense(h)); d->d = DensifiedRepresentation::from_lookup_indices(h->dev, indices, n, c, log_m); *out = d.release(); return 0;)
}
void lasso_host_dense_free(lasso_host_dense* d) { delete d; }
// ---- densify from operand columns (include/lasso_hip_operands.h, lasso_amd/csrc/operand_layout.cuh)
static void check_operand_args(const char* who, const lasso_operand_layout* L, const uint64_t* x, const uint64_t* y, size_t n, size_t c, size_t log_m) {
  if (const int bad = operand_layout_check(L, c, log_m)) throw Error(std::string(who) + ": " + operand_layout_error(bad));
  if ((y != nullptr) != (L->operands == 2u)) throw Error(std::string(who) + ": " OPL_MSG_Y);
  if (!x && n) throw Error(std::string(who) + ": null operand column");
}
// an operand that does not fit, in the words the device path reports it with (Dev::chk of lasso_densify_dim_operands' LASSO_ERR_INVALID): one text whichever path ran
static Error operand_unfit() { return Error("lasso_densify_dim_operands failed (" + std::to_string((int)LASSO_ERR_INVALID) + "): lasso_densify_dim_operands: " OPL_MSG_FIT); }
static void expand_operands(const lasso_operand_layout& L, const uint64_t* x, const uint64_t* y, size_t n, size_t c, uint64_t* indices) {
  for (size_t k = 0; k < n; k++) {
    const uint64_t vx = x[k], vy = y ? y[k] : 0;
    if (!operand_fits(vx, c, L.chunk_bits) || !operand_fits(vy, c, L.chunk_bits)) throw operand_unfit();
    for (size_t i = 0; i < c; i++) indices[k * c + i] = operand_index(L, vx, vy, c, i);
  }
}
int32_t lasso_host_operand_layout(const lasso_strategy* st, lasso_operand_layout* out) {
  GUARD(
    if (!st || !out) throw Error("lasso_host_operand_layout: null argument");
    const bool two = st->kind == LASSO_AND || st->kind == LASSO_OR || st->kind == LASSO_XOR || st->kind == LASSO_LT;
    if (!two && st->kind != LASSO_RANGE) throw Error("lasso_host_operand_layout: this strategy kind has no built-in operand layout (the caller passes its own)");
    if (st->log_m < 1 || st->log_m > 32) throw Error("lasso_host_operand_layout: log_m must be 1 .. 32");
    if (two && (st->log_m & 1u)) throw Error("lasso_host_operand_layout: a two-operand strategy splits log_m evenly between its operands: log_m must be even");
    out->operands = two ? 2u : 1u; out->chunk_bits = two ? st->log_m / 2 : st->log_m; out->msb_first = st->kind == LASSO_LT ? 1u : 0u;   // lt.rs:60-69: LT[0] is the top chunk
    return 0;)
}
int32_t lasso_host_operand_indices(const lasso_operand_layout* L, const uint64_t* x, const uint64_t* y, size_t n, size_t c, size_t log_m, uint64_t* indices) {
  GUARD(
    check_operand_args("lasso_host_operand_indices", L, x, y, n, c, log_m);
    if (!indices && n) throw Error("lasso_host_operand_indices: null output");
    expand_operands(*L, x, y, n, c, indices);
    return 0;)
}
int32_t lasso_host_densify_operands(lasso_host* h, const lasso_operand_layout* L, const uint64_t* x, const uint64_t* y, size_t n, size_t c, size_t log_m, int32_t where, lasso_host_dense** out) {
  GUARD(
    if (!h || !out || (where != 0 && where != 1)) throw Error("lasso_host_densify_operands: null argument, or `where` is neither 0 (host pointers) nor 1 (device pointers)");
    check_operand_args("lasso_host_densify_operands", L, x, y, n, c, log_m);
    const bool device = lasso_densify_dim_operands && sw::densify_operands();
    if (where == 1 && !device)
      throw Error("lasso_host_densify_operands: device-resident operands need lasso_densify_dim_operands (include/lasso_hip_operands.h), which the device library this host was linked against does not have (or LASSO_DENSIFY_OPERANDS=0 keeps out)");
    std::unique_ptr<lasso_host_dense> d(new lasso_host_dense(h));
    if (device) d->d = DensifiedRepresentation::from_operands(h->dev, &lasso_densify_dim_operands, *L, x, y, where == 1, n, c, log_m, h->ext_count[EXT_OPERANDS]);
    else { std::vector<uint64_t> idx(n * c); expand_operands(*L, x, y, n, c, idx.data()); d->d = DensifiedRepresentation::from_lookup_indices(h->dev, idx.data(), n, c, log_m); }
    *out = d.release(); return 0;)
}
int32_t lasso_host_densify_stats(lasso_host* h, uint64_t* operand_dims_on_device, int32_t* available, int32_t reset) { return ext_stats("lasso_host_densify_stats", h, EXT_OPERANDS, operand_dims_on_device, nullptr, available, reset); }
int32_t lasso_host_dense_info(lasso_host_dense* d, uint64_t* device_bytes, int32_t* compact) {
  if (!d || !d->d) return LASSO_ERR_INVALID;
  const DensifiedRepresentation& D = *d->d;
  uint64_t b = (uint64_t)(D.combined_l_variate_polys.n + D.combined_log_m_variate_polys.n) * sizeof(lasso_fr);
  for (auto& x : D.dim_u32) b += 4 * (uint64_t)x.n;
  for (auto& x : D.read_u32) b += 4 * (uint64_t)x.n;
  if (device_bytes) *device_bytes = b;
  if (compact) *compact = D.compact ? 1 : 0;
  return 0;
}
int32_t lasso_host_commit(lasso_host_dense* d, lasso_host_gens* g, uint8_t* out, size_t cap, size_t* len) {
  GUARD(SparsePolynomialCommitment c = d->d->commit(*g->g); ProofWriter w; w.pts_vec(c.l_variate_polys_commitment.compressed); w.pts_vec(c.log_m_variate_polys_commitment.compressed); return emit(w.b, out, cap, len);)
}
// one proof (capacity mode's bound on what stays parked between proofs is in Dev::alloc_bytes: returning everything to the driver here was measured at 1.4 s per proof
// of hipFree / hipMalloc at configs[3])
// A caller-defined strategy states its own NUM_MEMORIES: the derefs generators must have been made for it (surge.rs:39-47) — found here, before anything is launched,
// instead of at batch_commit's assert in the middle of the proof
static void check_custom_gens(const Strategy& S, const SparsePolyCommitmentGens& G, size_t s) {
  if (!S.custom()) return;
  const size_t nv = ceil_log2(next_pow2(S.num_memories() * next_pow2(s)));
  if (G.gens_derefs.n != ((size_t)1 << (nv - nv / 2))) throw Error("custom strategy: num_memories does not match the generators (gens_derefs was made for another number of memories or lookups)");
}
// lasso_host_prove / lasso_host_prove_cb behind their transcripts, lasso_host_verify / lasso_host_verify_cb behind theirs
static int32_t run_prover(lasso_host* h, const Strategy& S, DensifiedRepresentation& D, const SparsePolyCommitmentGens& G, ProofTranscript& t, RandomTape& tape, const lasso_fr* r, size_t r_len,
                          uint8_t* out, size_t cap, size_t* len) {
  std::vector<uint8_t> bytes;
  {
    if (S.custom() && (S.C() != D.C || S.M() != D.m)) throw Error("custom strategy: c / log_m do not match the densified representation");
    check_custom_gens(S, G, D.s);
    Prover P(h->dev, S, D, G, t, tape);
    try { P.prove(scalars_in(r, r_len)); } catch (...) { h->dev.abort_all(); throw; }
    bytes.swap(P.proof_bytes);
  }
  return emit(bytes, out, cap, len);
}
static void run_verifier(lasso_host* h, const Strategy& S, const SparsePolyCommitmentGens& G, ProofTranscript& t, size_t s, size_t log_m, const lasso_fr* r, size_t r_len,
                         const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  check_custom_gens(S, G, s);
  Verifier V(h->dev, S, G, t, h->wire_decoder(), h->points_msm(), h->tables_mle());
  *ok = V.verify(proof, proof_len, commitment, commitment_len, s, log_m, scalars_in(r, r_len)) ? 1 : 0;
  HostClock::dump();
}
int32_t lasso_host_prove(lasso_host* h, lasso_host_dense* d, lasso_host_gens* g, const lasso_strategy* st, const lasso_fr* r, size_t r_len, const char* tl, const char* pl,
                         uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    Strategy S = Strategy::from_abi(st);
    ProofTranscript t(tl); RandomTape tape(pl);
    return run_prover(h, S, *d->d, *g->g, t, tape, r, r_len, out, cap, len);)
}
// ---- live transcripts (include/lasso_prover.h lasso_transcript_vtbl)
struct lasso_merlin { Merlin m; explicit lasso_merlin(const char* label) : m(label) {} };
static void merlin_append(void* u, const uint8_t* label, size_t ll, const uint8_t* msg, size_t n) { ((lasso_merlin*)u)->m.append_message_l(label, ll, msg, n); }
static void merlin_challenge(void* u, const uint8_t* label, size_t ll, uint8_t* dest, size_t n) { ((lasso_merlin*)u)->m.challenge_bytes_l(label, ll, dest, n); }
static const lasso_transcript_vtbl g_merlin_vtbl = {merlin_append, merlin_challenge};
const lasso_transcript_vtbl* lasso_host_merlin_vtbl(void) { return &g_merlin_vtbl; }
lasso_merlin* lasso_host_merlin_new(const char* label) { try { return label ? new lasso_merlin(label) : nullptr; } catch (...) { return nullptr; } }
lasso_merlin* lasso_host_random_tape_new(const char* name) {
  try {
    if (!name) return nullptr;
    lasso_merlin* t = new lasso_merlin(name);
    ChaChaRng prng = ChaChaRng::test_rng(); uint8_t b[32]; fr_rand(prng).to_bytes(b);
    t->m.append_message("init_randomness", b, 32);   // RandomTape::new (utils/random.rs:15-31)
    return t;
  } catch (...) { return nullptr; }
}
void lasso_host_merlin_free(lasso_merlin* m) { delete m; }
int32_t lasso_host_prove_cb(lasso_host* h, lasso_host_dense* d, lasso_host_gens* g, const lasso_strategy* st, const lasso_fr* r, size_t r_len,
                            const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu, uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    if (!h || !d || !g || !st || !r || !tv || !pv) throw Error("lasso_host_prove_cb: null argument");
    Strategy S = Strategy::from_abi(st);
    ProofTranscript t(tv, tu); RandomTape tape(pv, pu);
    return run_prover(h, S, *d->d, *g->g, t, tape, r, r_len, out, cap, len);)
}
int32_t lasso_host_verify_cb(lasso_host* h, lasso_host_gens* g, const lasso_strategy* st, size_t s, const lasso_fr* r, size_t r_len, const lasso_transcript_vtbl* tv, void* tu,
                             const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  GUARD(
    if (!h || !g || !st || !r || !proof || !commitment || !ok || !tv) throw Error("lasso_host_verify_cb: null argument");
    Strategy S = Strategy::from_abi(st);
    ProofTranscript t(tv, tu);
    run_verifier(h, S, *g->g, t, s, st->log_m, r, r_len, proof, proof_len, commitment, commitment_len, ok);
    return 0;)
}
int32_t lasso_host_verify(lasso_host* h, lasso_host_gens* g, const lasso_strategy* st, size_t s, const lasso_fr* r, size_t r_len, const char* tl,
                          const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  GUARD(
    if (!h || !g || !st || !r || !proof || !commitment || !ok) throw Error("lasso_host_verify: null argument");
    Strategy S = Strategy::from_abi(st);
    ProofTranscript t(tl);
    run_verifier(h, S, *g->g, t, s, st->log_m, r, r_len, proof, proof_len, commitment, commitment_len, ok);
    return 0;)
}
// Test support: Prover::prove_cubic_batched (sumcheck.rs:27-135 with C = EqPolynomial(rand).evals(), grand_product.rs:122-128) on caller-supplied
// arrays with a SCRIPTED eq point, so that the eq points a transcript never produces (rand_t = 0: the claim-derived evaluation is unavailable;
// rand_t = 1: the table prefix vanishes) can be driven through the device path.  A, B: k arrays of 2^ell elements each, contiguous.
// out = per round the three compressed coefficients, then the ell challenges, then the k final claims of A and the k of B (32-byte scalars).
int32_t lasso_host_debug_cubic_batched(lasso_host* h, lasso_host_dense* dn, lasso_host_gens* g, const lasso_strategy* st, size_t k, size_t ell, const lasso_fr* A, const lasso_fr* B,
                                       const lasso_fr* rand, const lasso_fr* coeffs, const lasso_fr* claim, const char* tl, uint8_t* out, size_t cap, size_t* len) {
  try {
    Strategy S = Strategy::from_abi(st);
    ProofTranscript t(tl); RandomTape tape("unused");
    Prover P(h->dev, S, *dn->d, *g->g, t, tape);
    const size_t n = (size_t)1 << ell;
    std::vector<DBuf> bufs; std::vector<lasso_fr*> pa, pb;
    for (size_t c = 0; c < 2 * k; c++) {
      bufs.emplace_back(h->dev, n);
      h->dev.chk(lasso_upload(h->dev.ctx, bufs.back().p, (c < k ? A + c * n : B + (c - k) * n), n * sizeof(lasso_fr)), "lasso_upload");
      (c < k ? pa : pb).push_back(bufs.back().p);
    }
    ScVec rv = scalars_in(rand, ell), cv = scalars_in(coeffs, k);
    {   // read per call: the tests drive the HOST rounds (Prover::host_cubic_rounds: the tree tops' layers) through the same scripted points
      if (sw::debug_cubic_host()) {
        std::vector<ScVec> ha(k, ScVec(n)), hb(k, ScVec(n));
        for (size_t c = 0; c < k; c++) for (size_t i = 0; i < n; i++) { ha[c][i] = Sc::from_abi(A[c * n + i]); hb[c][i] = Sc::from_abi(B[c * n + i]); }
        SumcheckProof sp; ScVec r_out; std::vector<lasso_fr> heads; Sc e0 = Sc::from_abi(*claim);
        P.host_cubic_rounds(ha, hb, ell, rv, 0, cv, Sc::one(), e0, sp, r_out, heads);
        ProofWriter w;
        for (auto& c : sp.compressed_polys) w.sc_arr(c);
        w.sc_arr(r_out); for (auto& x : heads) w.sc(Sc::from_abi(x));
        return emit(w.b, out, cap, len);
      } }
    DBuf eq(h->dev, n / 2 ? n / 2 : 1);
    P.eq_half_local(rv, eq.p);
    ScVec r_out, ca, cb;
    SumcheckProof sp = P.prove_cubic_batched(Sc::from_abi(*claim), ell, false, pa, pb, eq.p, rv, cv, r_out, ca, cb);
    ProofWriter w;
    for (auto& c : sp.compressed_polys) w.sc_arr(c);
    w.sc_arr(r_out); w.sc_arr(ca); w.sc_arr(cb);
    return emit(w.b, out, cap, len);
  } catch (const std::exception& e) { g_err = e.what(); return -1; } catch (...) { g_err = "unknown error"; return -1; }
}
int32_t lasso_host_points_decompress(lasso_host* h, const uint8_t* wire32, size_t n, int32_t where, lasso_affine* out, uint8_t* canon32, uint8_t* status) {
  GUARD(
    if (!h || !status || (!wire32 && n) || (where != 0 && where != 1)) throw Error("lasso_host_points_decompress: null argument, or `where` is neither 0 (host) nor 1 (device)");
    if (where == 1) {
      if (!lasso_points_decompress) throw ext_unavailable("lasso_host_points_decompress", EXT_WIRE);
      h->dev.chk(lasso_points_decompress(h->dev.ctx, wire32, n, out, canon32, status), "lasso_points_decompress");
      h->ext_count[EXT_WIRE][0] += n;
      return 0;
    }
    for (size_t i = 0; i < n; i++) status[i] = decompress_point_abi(wire32 + 32 * i, out ? out + i : nullptr, canon32 ? canon32 + 32 * i : nullptr);
    return 0;)
}
int32_t lasso_host_wire_stats(lasso_host* h, uint64_t* device_points, int32_t* device_available, int32_t reset) { return ext_stats("lasso_host_wire_stats", h, EXT_WIRE, device_points, nullptr, device_available, reset); }
int32_t lasso_host_msm_points(lasso_host* h, const lasso_affine* points, const lasso_fr* scalars, size_t n, uint8_t* out_compressed32) {
  GUARD(
    if (!h || !out_compressed32 || (n && (!points || !scalars))) throw Error("lasso_host_msm_points: null argument");
    if (!lasso_msm_points) throw ext_unavailable("lasso_host_msm_points", EXT_MSM_POINTS);
    lasso_point out;
    h->dev.chk(lasso_msm_points(h->dev.ctx, points, scalars, n, &out), "lasso_msm_points");
    compress_one(Pt::from_abi(out), out_compressed32);
    return 0;)
}
int32_t lasso_host_msm_stats(lasso_host* h, uint64_t* points_calls, int32_t* available, int32_t reset) { return ext_stats("lasso_host_msm_stats", h, EXT_MSM_POINTS, points_calls, nullptr, available, reset); }
int32_t lasso_host_points_from_candidates(lasso_host* h, const uint64_t* limbs, const uint8_t* greatest, size_t n, int32_t where, lasso_affine* out, uint8_t* status) {
  GUARD(
    if (!h || !status || ((!limbs || !greatest) && n) || (where != 0 && where != 1)) throw Error("lasso_host_points_from_candidates: null argument, or `where` is neither 0 (host) nor 1 (device)");
    if (where == 1) {
      if (!lasso_points_from_candidates) throw ext_unavailable("lasso_host_points_from_candidates", EXT_GENS);
      h->dev.chk(lasso_points_from_candidates(h->dev.ctx, limbs, greatest, n, out, status), "lasso_points_from_candidates");
      h->ext_count[EXT_GENS][0] += n;
      return 0;
    }
    for (size_t i = 0; i < n; i++) {
      Pt p; lasso_affine a; memset(&a, 0, sizeof a);
      status[i] = (uint8_t)point_from_candidate(limbs + 4 * i, greatest[i] != 0, p);
      if (status[i] == LASSO_CAND_OK) normalize_points(&p, 1, &a);
      if (out) out[i] = a;
    }
    return 0;)
}
int32_t lasso_host_gens_stats(lasso_host* h, uint64_t* device_candidates, int32_t* available, int32_t reset) { return ext_stats("lasso_host_gens_stats", h, EXT_GENS, device_candidates, nullptr, available, reset); }
// include/lasso_prover_mle.h: SubtableStrategy::evaluate_subtable_mle for every subtable of a strategy of any kind
int32_t lasso_host_tables_mle(lasso_host* h, const lasso_strategy* st, const lasso_fr* point, size_t point_len, int32_t where, lasso_fr* out) {
  GUARD(
    if (!h || !st || !out || (!point && point_len) || (where != 0 && where != 1)) throw Error("lasso_host_tables_mle: null argument, or `where` is neither 0 (host) nor 1 (device)");
    const Strategy S = Strategy::from_abi(st);
    if (point_len != S.abi.log_m) throw Error("lasso_host_tables_mle: the point must have log_m coordinates");
    const ScVec pt = scalars_in(point, point_len);
    const size_t n = S.num_subtables();
    if (S.custom() && where == 1) {
      if (!lasso_tables_mle) throw ext_unavailable("lasso_host_tables_mle", EXT_MLE);
      TablesMle m; m.fn = &lasso_tables_mle; m.counter = h->ext_count[EXT_MLE];
      std::vector<size_t> ks(n); for (size_t k = 0; k < n; k++) ks[k] = k;
      const ScVec v = custom_subtable_mles_device(h->dev, S, m, ks, pt);
      for (size_t k = 0; k < n; k++) out[k] = v[k].abi();
      return 0;
    }
    for (size_t k = 0; k < n; k++) out[k] = evaluate_subtable_mle(S, k, pt).abi();
    return 0;)
}
int32_t lasso_host_mle_stats(lasso_host* h, uint64_t* device_tables, int32_t* available, int32_t reset) { return ext_stats("lasso_host_mle_stats", h, EXT_MLE, device_tables, nullptr, available, reset); }
// ---- include/lasso_prover_values.h: the lookup results as a vector, a vector's evaluation at r, the claim inside the proof bytes
// the refusal of the 64-bit form in the words the device entry reports it with (Dev::chk of lasso_lookup_values' LASSO_ERR_UNSUPPORTED): one text whichever route ran
static void values_check_form(const Strategy& S, int32_t form) {
  if (form != LASSO_VALUES_FR && form != LASSO_VALUES_U64) throw Error("lookup values: form is neither LASSO_VALUES_FR (0) nor LASSO_VALUES_U64 (1)");
  if (form == LASSO_VALUES_U64 && (S.custom() || S.spark() || !S.integer_tables() || !values_u64_offered(S.abi.kind, S.abi.c, S.abi.log_m)))
    throw Error("lasso_lookup_values failed (" + std::to_string((int)LASSO_ERR_UNSUPPORTED) + "): lasso_lookup_values: " VALUES_MSG_U64);
}
int32_t lasso_host_lookup_values_ref(const lasso_strategy* st, const uint64_t* indices, size_t n, int32_t form, void* out, size_t cap, size_t* count) {
  GUARD(
    const Strategy S = Strategy::from_abi(st);
    if (!indices || n < 1) throw Error("lasso_host_lookup_values_ref: null indices, or no lookups");
    if (S.abi.kind < LASSO_AND || S.abi.kind > LASSO_CUSTOM || S.C() < 1 || S.abi.log_m < 1 || S.abi.log_m > 32) throw Error("lasso_host_lookup_values_ref: unknown strategy kind, c = 0, or log_m outside 1..32");
    values_check_form(S, form);
    const size_t s = next_pow2(n), C = S.C(), alpha = S.num_memories(); const uint64_t m = (uint64_t)1 << S.abi.log_m;
    if (count) *count = s;
    if (!out || cap < s) { g_err = "output buffer too small"; return -2; }
    for (size_t k = 0; k < n * C; k++) if (indices[k] >= m) throw Error("lasso_host_lookup_values_ref: an index is not below 2^log_m");
    // materialize_subtables (subtables/*.rs), or the caller's
    std::vector<std::vector<uint32_t>> ti; std::vector<ScVec> tf; const bool ints = S.integer_tables();
    if (S.custom()) {
      for (size_t i = 0; i < S.num_subtables(); i++) {
        if (ints) ti.emplace_back(S.cabi.tables_u32[i], S.cabi.tables_u32[i] + m);
        else { ScVec t(m); for (uint64_t j = 0; j < m; j++) t[j] = Sc::from_abi(S.cabi.tables_fr[i][j]); tf.push_back(std::move(t)); }
      }
    } else if (ints) ti = S.materialize_subtables();
    else { const std::vector<ScVec> tau = S.spark_point(); for (size_t i = 0; i < S.num_subtables(); i++) tf.push_back(eq_evals_host(tau[i].data(), tau[i].size())); }
    const ScVec w = S.linear() ? S.weights() : ScVec();
    const uint32_t inc = values_inc(S.abi.kind, S.abi.log_m);
    ScVec vals(alpha); std::vector<uint32_t> iv(alpha);
    for (size_t k = 0; k < s; k++) {
      for (size_t i = 0; i < alpha; i++) {
        const uint64_t a = k < n ? indices[k * C + S.memory_to_dimension_index(i)] : 0;   // access_sequence.resize(s, 0): densified.rs:38
        const size_t sub = S.memory_to_subtable_index(i);
        if (ints) { iv[i] = ti[sub][a]; vals[i] = Sc::from_u64(iv[i]); } else vals[i] = tf[sub][a];
      }
      if (form == LASSO_VALUES_U64) {   // values_check_form: a built-in integer kind whose result fits
        uint64_t g;
        if (S.abi.kind == LASSO_LT) { g = iv[2 * (C - 1)]; for (size_t c = C - 1; c-- > 0;) g = values_lt_step(iv[2 * c], iv[2 * c + 1], g); }
        else { values_u128 acc = 0; for (size_t i = 0; i < alpha; i++) values_linear_add(acc, iv[i], (uint32_t)i * inc); g = (uint64_t)acc; }
        ((uint64_t*)out)[k] = g;
        continue;
      }
      Sc g = Sc::zero();   // combine_lookups as the strategies state it
      if (S.custom()) {
        for (uint32_t t = 0; t < S.cabi.num_terms; t++) { Sc term = Sc::from_abi(S.cabi.coeff[t]); for (uint32_t j = S.cabi.term_start[t]; j < S.cabi.term_start[t + 1]; j++) term *= vals[S.cabi.term_mem[j]]; g += term; }
      } else if (S.spark()) { g = Sc::one(); for (size_t i = 0; i < alpha; i++) g *= vals[i]; }
      else if (S.abi.kind == LASSO_LT) { Sc eq_prod = Sc::one(); for (size_t c = 0; c < C; c++) { g += vals[2 * c] * eq_prod; eq_prod *= vals[2 * c + 1]; } }   // lt.rs:62-71
      else for (size_t i = 0; i < alpha; i++) g += w[i] * vals[i];
      ((lasso_fr*)out)[k] = (g * Sc::one()).abi();
    }
    return 0;)
}
int32_t lasso_host_lookup_values(lasso_host* h, lasso_host_dense* dn, const lasso_strategy* st, int32_t form, int32_t out_on_device, void* out) {
  GUARD(
    if (!h || !dn || !dn->d || !out || (out_on_device != 0 && out_on_device != 1)) throw Error("lasso_host_lookup_values: null argument, or `out_on_device` is neither 0 (host) nor 1 (device)");
    const Strategy S = Strategy::from_abi(st);
    const DensifiedRepresentation& D = *dn->d; const Dev& d = h->dev;
    if (S.C() != D.C || S.abi.log_m != D.log_m) throw Error("lasso_host_lookup_values: the strategy's c / log_m do not match the densified representation");
    if (d.comm.sharded() || D.s_loc != D.s) throw Error("lasso_host_lookup_values: a slab-mode representation holds one residue class of the lookups per rank; the values of a sharded proof are not offered");
    values_check_form(S, form);
    if (!lasso_lookup_values) throw ext_unavailable("lasso_host_lookup_values", EXT_VALUES);
    // the tables on the device, as Prover::prove makes them (materialised by the device, Spark's eq tables, or the caller's uploaded); they go back to the pool on return
    const size_t m = D.m, s = D.s; const bool ints = S.integer_tables();
    std::vector<DBufU32> tu; std::vector<DBuf> tf; std::vector<const uint32_t*> pu; std::vector<const lasso_fr*> pf;
    for (size_t i = 0; i < S.num_subtables(); i++) {
      if (ints) {
        tu.emplace_back(d, m);
        if (S.custom()) d.chk(lasso_upload(d.ctx, tu.back().p, S.cabi.tables_u32[i], m * sizeof(uint32_t)), "lasso_upload");
        else d.chk(lasso_materialize_subtable_u32(d.ctx, &S.abi, (uint32_t)i, tu.back().p), "lasso_materialize_subtable_u32");
        pu.push_back(tu.back().p);
      } else {
        tf.emplace_back(d, m);
        if (S.custom()) d.chk(lasso_upload(d.ctx, tf.back().p, S.cabi.tables_fr[i], m * sizeof(lasso_fr)), "lasso_upload");
        else { const std::vector<ScVec> tau = S.spark_point(); std::vector<lasso_fr> tv; for (auto& x : tau[i]) tv.push_back(x.abi()); d.chk(lasso_eq_evals(d.ctx, tv.data(), (uint32_t)tv.size(), tf.back().p), "lasso_eq_evals"); }
        pf.push_back(tf.back().p);
      }
    }
    std::vector<const uint32_t*> dims; for (size_t i = 0; i < D.C; i++) dims.push_back(D.dim_u32[i].p);
    const size_t bytes = s * (form == LASSO_VALUES_U64 ? sizeof(uint64_t) : sizeof(lasso_fr));
    void* d_out = out_on_device ? out : d.alloc_bytes(bytes);
    try {
      d.chk(lasso_lookup_values(d.ctx, S.abi_ptr(), dims.data(), ints ? pu.data() : nullptr, ints ? nullptr : pf.data(), s, form, d_out), "lasso_lookup_values");
      if (out_on_device) d.chk(lasso_sync(d.ctx), "lasso_sync"); else d.chk(lasso_download(d.ctx, out, d_out, bytes), "lasso_download");
    } catch (...) { if (!out_on_device) d.free(d_out); throw; }
    if (!out_on_device) d.free(d_out);
    h->ext_count[EXT_VALUES][0] += s;
    return 0;)
}
int32_t lasso_host_dense_len(lasso_host_dense* dn, size_t* s) { GUARD(if (!dn || !dn->d || !s) throw Error("lasso_host_dense_len: null argument"); *s = dn->d->s; return 0;) }
int32_t lasso_host_values_evaluate(lasso_host* h, const lasso_fr* values, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len, lasso_fr* out) {
  GUARD(
    if (!h || !values || !out || (!r && r_len) || (on_device != 0 && on_device != 1)) throw Error("lasso_host_values_evaluate: null argument, or `values_on_device` is neither 0 (host) nor 1 (device)");
    if (r_len > 30 || s != ((size_t)1 << r_len)) throw Error("lasso_host_values_evaluate: the vector must have 2^r_len elements, r_len at most 30");
    if (r_len == 0) {   // the polynomial in no variables is its one value
      lasso_fr v; if (on_device) h->dev.chk(lasso_download(h->dev.ctx, &v, values, sizeof v), "lasso_download"); else v = values[0];
      *out = (Sc::from_abi(v) * Sc::one()).abi(); return 0;
    }
    auto fn = on_device ? lasso_tables_mle_dev : lasso_tables_mle;
    if (!fn) throw ext_unavailable("lasso_host_values_evaluate", EXT_MLE, "lasso_tables_mle / lasso_tables_mle_dev");
    const lasso_fr* one[1] = {values};
    h->dev.chk(fn(h->dev.ctx, nullptr, one, 1, (uint32_t)r_len, r, out), on_device ? "lasso_tables_mle_dev" : "lasso_tables_mle");
    return 0;)
}
int32_t lasso_host_proof_claimed_evaluation(const uint8_t* proof, size_t proof_len, lasso_fr* out) {
  GUARD(
    if (!proof || !out) throw Error("lasso_host_proof_claimed_evaluation: null argument");
    ProofReader r(proof, proof_len);
    std::vector<const uint8_t*> skipped; r.collect = &skipped;   // comm_derefs' points are stepped over, not decoded (read_proof's structural pass)
    (void)r.pts_vec(); (void)r.sumcheck();                       // surge.rs:92-104: comm_derefs, the primary sumcheck, then the scalar
    *out = r.sc().abi();
    return 0;)
}
int32_t lasso_host_values_stats(lasso_host* h, uint64_t* device_lookups, int32_t* available, int32_t reset) { return ext_stats("lasso_host_values_stats", h, EXT_VALUES, device_lookups, nullptr, available, reset); }
// ---- include/lasso_prover_poly.h: a commitment to the caller's vector and its opening at a point
}  // extern "C"
// The caller's vector where the device calls read it: 64-bit integers as they are when the device library has include/lasso_hip_poly.h, field elements otherwise (lifted on
// the host); host memory is uploaded.  A buffer made here goes back to the pool with the object.
struct PolyOperand {
  const Dev* dev = nullptr; const void* d = nullptr; bool u64 = false; void* own = nullptr;
  PolyOperand() {}
  PolyOperand(const PolyOperand&) = delete; PolyOperand& operator=(const PolyOperand&) = delete;
  ~PolyOperand() { try { if (own && dev) dev->free(own); } catch (...) {} }
};
// what is refused of one vector, whoever takes it: `w` names the call and, where the call takes several (include/lasso_prover_polys.h), the vector
static void poly_vec_check(const std::string& w, const void* values, int32_t form, int32_t on_device) {
  if (!values) throw Error(w + ": null argument");
  if (form != LASSO_VALUES_FR && form != LASSO_VALUES_U64) throw Error(w + ": form is neither LASSO_VALUES_FR (0) nor LASSO_VALUES_U64 (1)");
  if (on_device != 0 && on_device != 1) throw Error(w + ": `on_device` is neither 0 (host) nor 1 (device)");
  if ((uintptr_t)values & (on_device ? 15 : 7)) throw Error(w + ": the values pointer is misaligned for its form (host memory: 8 bytes, device memory: 16 bytes)");
}
// slab mode's refusal, of the calls that take one vector and of those that take several
static const char* const POLY_SLAB = ": a slab-mode host (world > 1) holds one residue class of every polynomial per rank; commitments to and openings of a caller's vector are not offered there";
static const char* const POLYS_SLAB = ": a slab-mode host (world > 1) holds one residue class of every polynomial per rank; commitments to and openings of a caller's vectors are not offered there";
static void poly_check(const char* who, lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s) {
  const std::string w(who);
  if (!h || !g || !g->g) throw Error(w + ": null argument");
  if (g->owner != h) throw Error(w + ": the generators belong to another host");
  poly_vec_check(w, values, form, on_device);
  if (h->dev.comm.sharded()) throw Error(w + POLY_SLAB);
  if (s == 0 || (s & (s - 1))) throw Error(w + ": the number of values must be a power of two");
  if (s != ((size_t)1 << g->num_vars)) throw Error(w + ": the generators were made for 2^" + std::to_string(g->num_vars) + " values, got " + std::to_string(s));
}
static void poly_operand(lasso_host* h, const void* values, int32_t form, int32_t on_device, size_t s, PolyOperand& o) {
  const Dev& d = h->dev; o.dev = &d;
  const size_t elem = form == LASSO_VALUES_U64 ? sizeof(uint64_t) : sizeof(lasso_fr);
  if (form == LASSO_VALUES_U64 && !EXTS[EXT_POLY].available()) {   // the device library is an implementation of lasso_hip.h alone: F::from on the host, the 32-byte entries from there on
    std::vector<uint64_t> v(s);
    if (on_device) d.chk(lasso_download(d.ctx, v.data(), values, s * 8), "lasso_download"); else memcpy(v.data(), values, s * 8);
    std::vector<lasso_fr> f(s); for (size_t i = 0; i < s; i++) f[i] = Sc::from_u64(v[i]).abi();
    o.own = d.alloc_bytes(s * sizeof(lasso_fr)); o.d = o.own;
    d.chk(lasso_upload(d.ctx, o.own, f.data(), s * sizeof(lasso_fr)), "lasso_upload");
    return;
  }
  o.u64 = form == LASSO_VALUES_U64;
  if (on_device) { o.d = values; return; }
  o.own = d.alloc_bytes(s * elem); o.d = o.own;
  d.chk(lasso_upload(d.ctx, o.own, values, s * elem), "lasso_upload");
}
static void poly_gens_check(const char* who, lasso_host* h, size_t num_vars, const void* out) {
  const std::string w(who);
  if (!h || !out) throw Error(w + ": null argument");
  if (num_vars < 1 || num_vars > 30) throw Error(w + ": num_vars must be 1 .. 30");
  if (h->dev.comm.sharded()) throw Error(w + POLY_SLAB);
}
// what the verify calls refuse before they read anything: `rest` = the call's other pointers are all there; k == SIZE_MAX: one vector at a point of num_vars coordinates,
// otherwise k evaluations at a point of r_len coordinates
static void verify_check(const char* who, lasso_host* h, lasso_host_poly_gens* g, bool rest, size_t r_len, size_t k = SIZE_MAX) {
  const std::string w(who);
  if (!h || !g || !g->g || !rest) throw Error(w + ": null argument");
  if (g->owner != h) throw Error(w + ": the generators belong to another host");
  if (h->dev.comm.sharded()) throw Error(w + (k == SIZE_MAX ? POLY_SLAB : POLYS_SLAB));
  if (k == SIZE_MAX) { if (r_len != g->num_vars) throw Error(w + ": the point must have num_vars coordinates"); return; }
  if (k == 0) throw Error(w + ": no vectors (k = 0)");
  if (r_len + ceil_log2(k) != g->num_vars) throw Error(w + ": the generators were made for " + std::to_string(g->num_vars) + " variables, but " + std::to_string(k) + " evaluations at a point of " +
                                                       std::to_string(r_len) + " coordinates are an opening in " + std::to_string(r_len + ceil_log2(k)));
}
// an opening and the commitment it is about, each read to its last byte
static WireDotProductProofLog read_opening(const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, std::vector<WirePoint>& comm) {
  ProofReader pr(proof, proof_len);
  const WireDotProductProofLog P = read_dpl(pr);
  if (!pr.done()) throw Error("proof bytes: trailing data");
  ProofReader cr(commitment, commitment_len);
  comm = cr.pts_vec();
  if (!cr.done()) throw Error("commitment bytes: trailing data");
  return P;
}
// ---- commitments, plain and hiding (include/lasso_prover_blind.h: the hiding form is composed of the device entries the plain one uses and of slab mode's two)
static void blinds_check(const std::string& w, const void* blinds) {
  if ((uintptr_t)blinds & 7) throw Error(w + ": the blinds pointer is misaligned (host memory: 8 bytes)");
}
// tape.random_vector("poly_blinds", count) (dense_mlpoly.rs:166-170) into the caller's array
static ScVec blinds_draw(const lasso_transcript_vtbl* pv, void* pu, size_t count, lasso_fr* out) {
  RandomTape tape(pv, pu);
  const ScVec b = tape.random_vector("poly_blinds", count);
  for (size_t i = 0; i < count; i++) out[i] = (b[i] * Sc::one()).abi();
  return b;
}
// rows[i] += blinds[i] * h on the host: `rows` wire rows are decoded as the verifier would decode them, the sums compressed in one batch
static void blind_rows_host(lasso_host* h, const PolyCommitmentGens& g, const Sc* blinds, size_t rows, uint8_t* wire) {
  const std::vector<WirePoint> pts = decode_points(h->dev, h->wire_decoder(), wire, rows, "commitment rows");
  std::vector<Pt> sum(rows);
  for (size_t i = 0; i < rows; i++) { const Pt b = g.hmul.mul(blinds[i]); sum[i] = pts[i].infinity ? b : pts[i].p + b; }
  std::vector<uint8_t> out; compress_batch(sum, out);
  memcpy(wire, out.data(), 32 * rows);
  h->blind_count[1] += rows;
}
// `rows` whole rows of R values of one vector as wire bytes at `wire`: row i = <Z_i, G>, + blinds[i] * h where there are blinds (commitments.rs:84-93).  hb: the one-point
// base [h], made by the first vector that is blinded on the device and destroyed by the caller
static void commit_rows(lasso_host* h, const PolyCommitmentGens& g, const PolyOperand& o, size_t s, size_t rows, size_t R, const Sc* blinds, lasso_bases** hb, uint8_t* wire) {
  const Dev& d = h->dev;
  if (o.u64) {   // read as 8-byte integers; the populated bits bound the scalars: the width of the MSM's windows, and below 2^32 the 4-byte route.  The rows come back in wire form
    uint64_t bits = 0;
    d.chk(lasso_u64_or(d.ctx, (const uint64_t*)o.d, s, &bits), "lasso_u64_or");
    d.chk(lasso_hyrax_commit_compressed_u64(d.ctx, (const uint64_t*)o.d, bits, rows, R, g.bases, wire), "lasso_hyrax_commit_compressed_u64");
    h->ext_count[EXT_POLY][0] += s;
    if (blinds) blind_rows_host(h, g, blinds, rows, wire);
    return;
  }
  if (!blinds) { const PolyCommitment c = hyrax_commit_rows(d, (const lasso_fr*)o.d, rows, R, g); memcpy(wire, c.compressed.data(), 32 * rows); return; }
  // field elements: data rows and blind rows as the kernels' own points, side by side, added and compressed by slab mode's reduction
  const size_t rb = lasso_point_row_bytes();
  struct Bytes { const Dev& d; void* p; ~Bytes() { try { if (p) d.free(p); } catch (...) {} } } parts{d, d.alloc_bytes(2 * rows * rb)};
  int32_t rc = lasso_hyrax_commit_rows_dev(d.ctx, (const lasso_fr*)o.d, rows, R, g.bases, parts.p);
  if (rc == LASSO_ERR_UNSUPPORTED) {   // a device library without row sums on the device: wire rows, blinded on the host
    d.chk(lasso_hyrax_commit_compressed(d.ctx, (const lasso_fr*)o.d, rows, R, g.bases, wire), "lasso_hyrax_commit_compressed");
    blind_rows_host(h, g, blinds, rows, wire);
    return;
  }
  d.chk(rc, "lasso_hyrax_commit_rows_dev");
  if (!*hb) d.chk(lasso_bases_create(d.ctx, &g.affine[g.n + 1], 1, hb), "lasso_bases_create");
  DBuf d_bl(d, rows);
  std::vector<lasso_fr> bl(rows); for (size_t i = 0; i < rows; i++) bl[i] = blinds[i].abi();
  d.chk(lasso_upload(d.ctx, d_bl.p, bl.data(), rows * sizeof(lasso_fr)), "lasso_upload");
  d.chk(lasso_hyrax_commit_rows_dev(d.ctx, d_bl.p, rows, 1, *hb, (uint8_t*)parts.p + rows * rb), "lasso_hyrax_commit_rows_dev");
  d.chk(lasso_points_reduce_compress(d.ctx, parts.p, 2, rows, wire), "lasso_points_reduce_compress");
  h->blind_count[0] += rows;
}
struct BlindBase { const Dev& d; lasso_bases* b = nullptr; explicit BlindBase(const Dev& d_) : d(d_) {} ~BlindBase() { if (b) lasso_bases_destroy(d.ctx, b); } };
// DensePolynomial::merge(vecs[0 .. k)).commit(gens, blinds) in wire form, the merge never made: L rows of R values, vector b in the rows [b * rows_per, (b + 1) * rows_per)
// (one vector: k = 1, rows_per = L).  blinds: null = None, else L of them, one draw for the whole merge
static std::vector<uint8_t> commit_vectors(lasso_host* h, const PolyCommitmentGens& g, const lasso_host_poly_vec* vecs, size_t k, size_t s, size_t L, size_t R, size_t rows_per, const ScVec* blinds) {
  std::vector<uint8_t> rows(32 * L);
  BlindBase hb(h->dev);
  for (size_t b = 0; b < k; b++) {   // one vector at a time: an uploaded one is released before the next
    PolyOperand o; poly_operand(h, vecs[b].values, vecs[b].form, vecs[b].on_device, s, o);
    try { commit_rows(h, g, o, s, rows_per, R, blinds ? blinds->data() + b * rows_per : nullptr, &hb.b, rows.data() + 32 * b * rows_per); } catch (...) { h->dev.abort_all(); throw; }
  }
  if (k * rows_per < L && blinds) {   // the zero blocks behind k commit to blinds[i] * h, row by row
    std::vector<Pt> tail; for (size_t i = k * rows_per; i < L; i++) tail.push_back(g.hmul.mul((*blinds)[i]));
    std::vector<uint8_t> tb; compress_batch(tail, tb);
    memcpy(rows.data() + 32 * k * rows_per, tb.data(), tb.size());
    h->blind_count[1] += tail.size();
  } else if (k * rows_per < L) {      // without blinds, to the identity
    uint8_t id[32]; compress_one(Pt::identity(), id);
    for (size_t i = k * rows_per; i < L; i++) memcpy(rows.data() + 32 * i, id, 32);
  }
  ProofWriter w; w.pts_vec(rows);
  return w.b;
}
// lasso_host_poly_open_blinded, and lasso_host_poly_open (no blinds, no C_Zr) in its own name
static int32_t poly_open(const char* who, lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len,
                         const lasso_fr* blinds, const lasso_fr* blind_Zr, const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu,
                         lasso_fr* Zr, uint8_t* C_Zr, uint8_t* proof, size_t cap, size_t* len) {
  const std::string w(who);
  poly_check(who, h, g, values, form, on_device, s);
  if (!r || !tv || !pv) throw Error(w + ": null argument");
  if (r_len != g->num_vars) throw Error(w + ": the point must have num_vars coordinates");
  blinds_check(w, blinds); blinds_check(w, blind_Zr);
  ProofTranscript t(tv, tu); RandomTape tape(pv, pu);
  const ScVec rv = scalars_in(r, r_len), bl = scalars_in(blinds, blinds ? (size_t)1 << (g->num_vars / 2) : 0);
  Sc bz; if (blind_Zr) bz = Sc::from_abi(*blind_Zr);
  PolyOperand o; poly_operand(h, values, form, on_device, s, o);
  Sc y; DotProductProofLog P; uint8_t cy[32];
  try {
    P = Prover::poly_eval_prove_resident(h->dev, t, tape, o.d, o.u64 ? lasso_matvec_left_u64_dev : nullptr, g->num_vars, rv, nullptr, &y, *g->g, blinds ? &bl : nullptr, blind_Zr ? &bz : nullptr, cy);
  } catch (...) { h->dev.abort_all(); throw; }
  if (o.u64) h->ext_count[EXT_POLY][1] += s;
  if (Zr) *Zr = (y * Sc::one()).abi();
  if (C_Zr) memcpy(C_Zr, cy, 32);
  ProofWriter pw; P.write(pw);
  return emit(pw.b, proof, cap, len);
}
extern "C" {
int32_t lasso_host_poly_gens_new(lasso_host* h, const char* label, size_t num_vars, lasso_host_poly_gens** out) {
  GUARD(
    poly_gens_check("lasso_host_poly_gens_new", h, num_vars, out);
    if (!label) throw Error("lasso_host_poly_gens_new: null label");
    std::unique_ptr<lasso_host_poly_gens> g(new lasso_host_poly_gens(h, num_vars));
    const GenStream gs(h->dev, label, ((size_t)1 << (num_vars - num_vars / 2)) + 2, h->gens_device());
    g->g.reset(new PolyCommitmentGens(h->dev, gs, num_vars));
    *out = g.release(); return 0;)
}
int32_t lasso_host_poly_gens_from_points(lasso_host* h, size_t num_vars, const lasso_affine* points, size_t n_points, lasso_host_poly_gens** out) {
  GUARD(
    poly_gens_check("lasso_host_poly_gens_from_points", h, num_vars, out);
    std::unique_ptr<lasso_host_poly_gens> g(new lasso_host_poly_gens(h, num_vars));
    g->g.reset(new PolyCommitmentGens(h->dev, points, n_points, num_vars));
    *out = g.release(); return 0;)
}
void lasso_host_poly_gens_free(lasso_host_poly_gens* g) { delete g; }
int32_t lasso_host_poly_commit(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    poly_check("lasso_host_poly_commit", h, g, values, form, on_device, s);
    const size_t nv = g->num_vars, L = (size_t)1 << (nv / 2), R = (size_t)1 << (nv - nv / 2);
    const lasso_host_poly_vec v = {values, form, on_device};
    return emit(commit_vectors(h, *g->g, &v, 1, s, L, R, L, nullptr), out, cap, len);)
}
int32_t lasso_host_poly_commitment_append(const lasso_transcript_vtbl* tv, void* tu, const char* label, const uint8_t* commitment, size_t len) {
  GUARD(
    if (!tv || !label || !commitment) throw Error("lasso_host_poly_commitment_append: null argument");
    ProofReader r(commitment, len);
    PolyCommitment c; c.rows = r.len(32);
    if (len != 8 + 32 * c.rows) throw Error("commitment bytes: trailing data");
    c.compressed.assign(commitment + 8, commitment + len);
    ProofTranscript t(tv, tu);
    append_poly_commitment(t, label, c);
    return 0;)
}
int32_t lasso_host_poly_open(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len,
                             const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu, lasso_fr* Zr, uint8_t* proof, size_t cap, size_t* len) {
  GUARD(return poly_open("lasso_host_poly_open", h, g, values, form, on_device, s, r, r_len, nullptr, nullptr, tv, tu, pv, pu, Zr, nullptr, proof, cap, len);)
}
int32_t lasso_host_poly_verify(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const lasso_fr* Zr, const lasso_transcript_vtbl* tv, void* tu,
                               const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  GUARD(
    verify_check("lasso_host_poly_verify", h, g, r && Zr && tv && proof && commitment && ok, r_len);
    std::vector<WirePoint> comm;
    const WireDotProductProofLog P = read_opening(proof, proof_len, commitment, commitment_len, comm);
    ProofTranscript t(tv, tu);
    *ok = Verifier::poly_eval_verify_plain(h->dev, t, h->points_msm(), P, *g->g, scalars_in(r, r_len), Sc::from_abi(*Zr), comm) ? 1 : 0;
    return 0;)
}
int32_t lasso_host_poly_stats(lasso_host* h, uint64_t* u64_commit_elements, uint64_t* u64_open_elements, int32_t* available, int32_t reset) { return ext_stats("lasso_host_poly_stats", h, EXT_POLY, u64_commit_elements, u64_open_elements, available, reset); }
// ---- include/lasso_prover_polys.h: k vectors under one commitment, opened at r in one proof
}  // extern "C"
// The merge of k vectors of s = 2^nv values as a matrix: 2^left rows of 2^right values, vector b in the rows [b * rows_per, (b + 1) * rows_per)
struct PolysShape { size_t nv = 0, kappa = 0, left = 0, right = 0, rows_per = 0; };
// every refusal of the calls that take vectors, before anything is uploaded or launched.  g == null: a call without generators; r_len == SIZE_MAX: a call without a point
static PolysShape polys_check(const char* who, lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, size_t r_len) {
  const std::string w(who);
  if (!h || (!vecs && k)) throw Error(w + ": null argument");
  if (g && g->owner != h) throw Error(w + ": the generators belong to another host");
  if (h->dev.comm.sharded()) throw Error(w + POLYS_SLAB);
  if (k == 0) throw Error(w + ": no vectors (k = 0)");
  if (s == 0 || (s & (s - 1))) throw Error(w + ": the number of values per vector must be a power of two");
  PolysShape sh; while (((size_t)1 << sh.nv) < s) sh.nv++;
  sh.kappa = ceil_log2(k);
  const std::string merge = std::to_string(k) + " vectors of 2^" + std::to_string(sh.nv) + " values merge into a polynomial of " + std::to_string(sh.nv + sh.kappa) + " variables";
  if (sh.nv + sh.kappa > 30) throw Error(w + ": " + merge + "; at most 30 are offered");
  if (g && g->num_vars != sh.nv + sh.kappa) throw Error(w + ": the generators were made for " + std::to_string(g->num_vars) + " variables, but " + merge);
  if (r_len != SIZE_MAX && r_len != sh.nv) throw Error(w + ": the point must have log2(s) = " + std::to_string(sh.nv) + " coordinates (the " + std::to_string(sh.kappa) + " above them are challenges), got " + std::to_string(r_len));
  sh.left = (sh.nv + sh.kappa) / 2; sh.right = sh.nv + sh.kappa - sh.left;
  if (sh.right > sh.nv) throw Error(w + ": a row of the merged matrix (2^" + std::to_string(sh.right) + " values) would span several vectors of " + std::to_string(s) + " values; " + merge);
  sh.rows_per = (size_t)1 << (sh.left - sh.kappa);
  for (size_t b = 0; b < k; b++) poly_vec_check(w + ": vector " + std::to_string(b), vecs[b].values, vecs[b].form, vecs[b].on_device);
  return sh;
}
// the block pass over the k vectors where the device reads them, and evals[b] = MLE(vecs[b])(r), fully reduced; host vectors are uploaded for its duration
static Prover::BlockPass polys_pass(lasso_host* h, const lasso_host_poly_vec* vecs, size_t k, size_t s, const PolysShape& sh, const ScVec& rv, ScVec& ev, lasso_fr* evals, size_t* u64_vectors) {
  std::vector<PolyOperand> ops(k); std::vector<Prover::PolyBlock> blocks(k);
  size_t wide = 0;
  for (size_t b = 0; b < k; b++) { poly_operand(h, vecs[b].values, vecs[b].form, vecs[b].on_device, s, ops[b]); blocks[b] = {ops[b].d, ops[b].u64}; wide += ops[b].u64 ? 1 : 0; }
  if (u64_vectors) *u64_vectors = wide;
  try {
    Prover::BlockPass bp = Prover::block_pass(h->dev, h->dev.ctx, &Dev::chk, blocks, lasso_matvec_left_u64_dev, sh.nv, rv);
    ev = Prover::block_evals(h->dev, bp, rv);
    for (size_t b = 0; b < k; b++) evals[b] = (ev[b] * Sc::one()).abi();
    return bp;
  } catch (...) { h->dev.abort_all(); throw; }
}
// lasso_host_polys_open_blinded, and lasso_host_polys_open (blinds == null) in its own name
static int32_t polys_open(const char* who, lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len, const lasso_fr* blinds,
                          const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu, lasso_fr* evals, uint8_t* proof, size_t cap, size_t* len) {
  if (!g || !g->g || !r || !tv || !pv || !evals) throw Error(std::string(who) + ": null argument");
  const PolysShape sh = polys_check(who, h, g, vecs, k, s, r_len);
  blinds_check(who, blinds);
  ProofTranscript t(tv, tu); RandomTape tape(pv, pu);
  const ScVec rv = scalars_in(r, r_len), bl = scalars_in(blinds, blinds ? (size_t)1 << sh.left : 0);
  size_t wide = 0; ScVec ev;
  Prover::BlockPass bp = polys_pass(h, vecs, k, s, sh, rv, ev, evals, &wide);
  DotProductProofLog P;
  try { P = Prover::polys_eval_prove(h->dev, t, tape, bp, ev, *g->g, blinds ? &bl : nullptr); } catch (...) { h->dev.abort_all(); throw; }
  h->ext_count[EXT_POLY][1] += wide * s; h->polys_count[1] += k;
  ProofWriter w; P.write(w);
  return emit(w.b, proof, cap, len);
}
extern "C" {
int32_t lasso_host_polys_commit(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    if (!g || !g->g) throw Error("lasso_host_polys_commit: null argument");
    const PolysShape sh = polys_check("lasso_host_polys_commit", h, g, vecs, k, s, SIZE_MAX);
    const std::vector<uint8_t> bytes = commit_vectors(h, *g->g, vecs, k, s, (size_t)1 << sh.left, (size_t)1 << sh.right, sh.rows_per, nullptr);
    h->polys_count[0] += k;
    return emit(bytes, out, cap, len);)
}
int32_t lasso_host_polys_open(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len,
                              const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu, lasso_fr* evals, uint8_t* proof, size_t cap, size_t* len) {
  GUARD(return polys_open("lasso_host_polys_open", h, g, vecs, k, s, r, r_len, nullptr, tv, tu, pv, pu, evals, proof, cap, len);)
}
int32_t lasso_host_polys_verify(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const lasso_fr* evals, size_t k, const lasso_transcript_vtbl* tv, void* tu,
                                const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  GUARD(
    verify_check("lasso_host_polys_verify", h, g, (r || !r_len) && evals && tv && proof && commitment && ok, r_len, k);
    std::vector<WirePoint> comm;
    const WireDotProductProofLog P = read_opening(proof, proof_len, commitment, commitment_len, comm);
    ProofTranscript t(tv, tu);
    *ok = Verifier::combined_table_eval_verify_plain(h->dev, t, h->points_msm(), P, *g->g, scalars_in(r, r_len), scalars_in(evals, k), comm) ? 1 : 0;
    return 0;)
}
int32_t lasso_host_polys_evaluate(lasso_host* h, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len, lasso_fr* evals) {
  GUARD(
    if ((!r && r_len) || !evals) throw Error("lasso_host_polys_evaluate: null argument");
    const PolysShape sh = polys_check("lasso_host_polys_evaluate", h, nullptr, vecs, k, s, r_len);
    ScVec ev;
    (void)polys_pass(h, vecs, k, s, sh, scalars_in(r, r_len), ev, evals, nullptr);
    return 0;)
}
int32_t lasso_host_polys_stats(lasso_host* h, uint64_t* vectors_committed, uint64_t* vectors_opened, int32_t reset) {
  return pair_stats("lasso_host_polys_stats", h, &lasso_host::polys_count, EXT_COUNT, vectors_committed, vectors_opened, nullptr, reset);
}
// ---- include/lasso_prover_blind.h: the hiding form of the two headers above
int32_t lasso_host_poly_commit_blinded(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s,
                                       const lasso_transcript_vtbl* pv, void* pu, lasso_fr* blinds_out, uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    poly_check("lasso_host_poly_commit_blinded", h, g, values, form, on_device, s);
    if (!pv || !blinds_out) throw Error("lasso_host_poly_commit_blinded: null argument");
    blinds_check("lasso_host_poly_commit_blinded", blinds_out);
    const size_t nv = g->num_vars, L = (size_t)1 << (nv / 2), R = (size_t)1 << (nv - nv / 2);
    const ScVec blinds = blinds_draw(pv, pu, L, blinds_out);
    const lasso_host_poly_vec v = {values, form, on_device};
    return emit(commit_vectors(h, *g->g, &v, 1, s, L, R, L, &blinds), out, cap, len);)
}
int32_t lasso_host_poly_open_blinded(lasso_host* h, lasso_host_poly_gens* g, const void* values, int32_t form, int32_t on_device, size_t s, const lasso_fr* r, size_t r_len,
                                     const lasso_fr* blinds, const lasso_fr* blind_Zr, const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu,
                                     lasso_fr* Zr, uint8_t C_Zr[32], uint8_t* proof, size_t cap, size_t* len) {
  GUARD(return poly_open("lasso_host_poly_open_blinded", h, g, values, form, on_device, s, r, r_len, blinds, blind_Zr, tv, tu, pv, pu, Zr, C_Zr, proof, cap, len);)
}
int32_t lasso_host_poly_verify_committed(lasso_host* h, lasso_host_poly_gens* g, const lasso_fr* r, size_t r_len, const uint8_t C_Zr[32], const lasso_transcript_vtbl* tv, void* tu,
                                         const uint8_t* proof, size_t proof_len, const uint8_t* commitment, size_t commitment_len, int32_t* ok) {
  GUARD(
    verify_check("lasso_host_poly_verify_committed", h, g, r && C_Zr && tv && proof && commitment && ok, r_len);
    std::vector<WirePoint> comm;
    const WireDotProductProofLog P = read_opening(proof, proof_len, commitment, commitment_len, comm);
    WirePoint cz;
    if (!decompress_point(C_Zr, cz.p, cz.infinity)) throw Error("C_Zr bytes: invalid point encoding");
    if (cz.infinity) cz.p = Pt::identity();
    compress_affine_pt(cz.p, cz.infinity, cz.bytes);
    ProofTranscript t(tv, tu);
    *ok = Verifier::poly_eval_verify(h->dev, t, h->points_msm(), P, *g->g, scalars_in(r, r_len), cz, comm) ? 1 : 0;
    return 0;)
}
int32_t lasso_host_polys_commit_blinded(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s,
                                        const lasso_transcript_vtbl* pv, void* pu, lasso_fr* blinds_out, uint8_t* out, size_t cap, size_t* len) {
  GUARD(
    if (!g || !g->g) throw Error("lasso_host_polys_commit_blinded: null argument");
    const PolysShape sh = polys_check("lasso_host_polys_commit_blinded", h, g, vecs, k, s, SIZE_MAX);
    if (!pv || !blinds_out) throw Error("lasso_host_polys_commit_blinded: null argument");
    blinds_check("lasso_host_polys_commit_blinded", blinds_out);
    const size_t L = (size_t)1 << sh.left, R = (size_t)1 << sh.right;
    const ScVec blinds = blinds_draw(pv, pu, L, blinds_out);   // one draw for the whole merge, as merge(polys).commit(gens, Some(tape)) makes it
    const std::vector<uint8_t> bytes = commit_vectors(h, *g->g, vecs, k, s, L, R, sh.rows_per, &blinds);
    h->polys_count[0] += k;
    return emit(bytes, out, cap, len);)
}
int32_t lasso_host_polys_open_blinded(lasso_host* h, lasso_host_poly_gens* g, const lasso_host_poly_vec* vecs, size_t k, size_t s, const lasso_fr* r, size_t r_len,
                                      const lasso_fr* blinds, const lasso_transcript_vtbl* tv, void* tu, const lasso_transcript_vtbl* pv, void* pu,
                                      lasso_fr* evals, uint8_t* proof, size_t cap, size_t* len) {
  GUARD(return polys_open("lasso_host_polys_open_blinded", h, g, vecs, k, s, r, r_len, blinds, tv, tu, pv, pu, evals, proof, cap, len);)
}
int32_t lasso_host_blind_stats(lasso_host* h, uint64_t* rows_device, uint64_t* rows_host, int32_t reset) {
  return pair_stats("lasso_host_blind_stats", h, &lasso_host::blind_count, EXT_COUNT, rows_device, rows_host, nullptr, reset);
}
int32_t lasso_host_strategy_check(const lasso_strategy* st) {
  GUARD(const Strategy S = Strategy::from_abi(st); (void)S; return 0;)
}
void lasso_host_gen_indices(size_t sparsity, size_t memory_size, uint64_t* out) { ChaChaRng rng = ChaChaRng::test_rng(); for (size_t i = 0; i < sparsity; i++) out[i] = rng.next_u64() % memory_size; }
void lasso_host_gen_random_point(size_t bits, lasso_fr* out) { ChaChaRng rng = ChaChaRng::test_rng(); for (size_t i = 0; i < bits; i++) out[i] = fr_rand(rng).abi(); }
}
