// Which MSM kernel serves a call of the device library, as lasso_hip.hip decides it: the plan functions of lasso_amd/csrc/launch_plan.cuh over the switches of
// lasso_amd/csrc/device_switches.cuh, both included as they are (as tests/cpp/test_launch_plan_host.cpp includes them).  tests/msmvariants.py runs this program once per switch
// setting, as a child process with that environment (the switches are read once per process), and tests/test_msm_reach_cpu.py holds every row of its table to the plan printed here.
// stdin, one call per line:   <id> <entry> <rows> <cols> <bps> <W> <ngens> <world>
//   entry: hyrax_commit | hyrax_commit_compressed | hyrax_commit_compressed_u32 | hyrax_commit_rows_dev | msm | msm_dev_scaled | bullet_round | bullet_round_slab | msm_dev_slab
//   rows x cols: the matrix of a commitment; msm / msm_dev_scaled / msm_dev_slab: rows = 1, cols = n; bullet_round(_slab): rows = n, cols = nk
//   bps, W: bytes per scalar and populated nibbles as hyrax_commit_impl finds them in the data (4 and (bits + 3) / 4, or 32 and 64); ignored by the last three entries
//   ngens: points the bases object was created from (lasso_bases_create); the slab entries: the rank's n / world generators, then Q and H
//   world: ranks of slab mode (the two slab entries; 1 everywhere else)
// stdout, one JSON object per line: {"id", "msm": MsmPlan | null, "direct": MsmDirectPlan | null, "bullet": BulletPlan | null} — the plans the call goes through.
#include <cstdio>
#include <cstring>
#include "../../lasso_amd/csrc/device_switches.cuh"
#include "../../lasso_amd/csrc/launch_plan.cuh"

namespace dsw = lasso::dsw;

static const char* kernel_name(MsmKernel k) {
  switch (k) {
    case MSM_K_DIRECT: return "DIRECT"; case MSM_K_ROWS8W: return "ROWS8W"; case MSM_K_ROWS8: return "ROWS8";
    case MSM_K_PIP: return "PIP"; case MSM_K_FULL8: return "FULL8"; case MSM_K_BUCKETS: return "BUCKETS";
  }
  return "?";
}
static const char* result_name(MsmResult r) {
  switch (r) {
    case MSM_R_FLAG: return "FLAG"; case MSM_R_COMPRESSED_MAPPED: return "COMPRESSED_MAPPED"; case MSM_R_COMPRESSED_MEMCPY: return "COMPRESSED_MEMCPY";
    case MSM_R_DEVICE_ROWS: return "DEVICE_ROWS"; case MSM_R_MEMCPY: return "MEMCPY";
  }
  return "?";
}

// lasso_bases_create: the digit-multiple table for sets of up to LASSO_MSM_DIRECT_MAX_N points, the byte-multiple table beside it for sets of up to
// LASSO_MSM_DIRECT8_MAX_N (0 under LASSO_MSM_DIRECT8=0); every allocation granted (tab8, pip_scratch: run_msm's first plan)
static MsmHave have_of(size_t ngens) {
  const bool mult = ngens <= dsw::msm_direct_max_n();
  const bool mult8 = mult && ngens <= dsw::msm_direct8_max_n();
  return MsmHave{ngens, mult, mult8, true, true};
}

static void print_bullet(const BulletPlan& b, size_t nk, size_t world) {   // wide: both rows get n_loc / 2 local columns (half >= P); else one row of the rank gets all n_loc, the other none
  const bool wide = nk / 2 >= world;
  printf("{\"w8\": %s, \"windows\": %zu, \"n_loc\": %zu, \"K\": %zu, \"ipc\": %u, \"ipc_cap\": %zu, \"world\": %zu, \"half\": %zu, \"wide\": %s, \"cols\": %zu, \"weights\": %zu}", b.w8 ? "true" : "false", b.windows, b.n_loc, b.K,
         b.ipc, b.windows * 128, world, nk / 2, wide ? "true" : "false", wide ? b.n_loc / 2 : b.n_loc, b.n_loc * world / nk);
}
static void print_direct(const MsmDirectPlan& d) {
  printf("{\"w8\": %s, \"windows\": %zu, \"K\": %zu, \"ipc\": %u, \"ipc_cap\": %zu}", d.w8 ? "true" : "false", d.windows, d.K, d.ipc, d.windows * 128);
}
// run_msm: its plan, and run_msm_direct's where the plan hands the call over
static void print_run_msm(const MsmShape& s, const MsmHave& have) {
  const MsmSwitches sw = {dsw::msm_direct(), dsw::msm_rows8(), dsw::msm_rows8w(), dsw::msm_full8(), dsw::msm_pip(), dsw::msm_rows8w_waves(), dsw::msm_pip_min_cols(), dsw::msm_pip_scratch_mb(), dsw::msm_direct_wgs()};
  const MsmPlan p = msm_plan(s, have, sw);
  printf("\"msm\": {\"kernel\": \"%s\", \"result\": \"%s\", \"bps\": %u, \"rows\": %zu, \"n_cols\": %zu", kernel_name(p.kernel), result_name(p.result), s.bps, s.rows, s.n_cols);
  if (p.kernel != MSM_K_DIRECT)
    printf(", \"K\": %zu, \"cols_per_chunk\": %zu, \"W8\": %u, \"rpw\": %zu, \"waves\": %zu, \"pip_items\": %zu, \"pip_row_bytes\": %zu, \"pip_group\": %zu, \"pts_bytes\": %zu",
           p.K, p.cols_per_chunk, p.W8, p.rpw, p.waves, p.pip_items, p.pip_row_bytes, p.pip_group, msm_pts_bytes(s.rows, s.n_cols, msm_direct_wgs(dsw::msm_direct_wgs())));
  printf("}, \"direct\": ");
  if (p.kernel == MSM_K_DIRECT) print_direct(msm_direct_plan(s.rows, s.n_cols, have.mult8, dsw::msm_direct_wgs())); else printf("null");
  printf(", \"bullet\": null");
}

int main() {
  char id[128], entry[64];
  size_t rows, cols, ngens, world; unsigned bps, W;
  while (scanf("%127s %63s %zu %zu %u %u %zu %zu", id, entry, &rows, &cols, &bps, &W, &ngens, &world) == 8) {
    const MsmHave have = have_of(ngens);
    const bool direct = have.mult && dsw::msm_direct();   // the entry points that choose the latency-shaped launch themselves ask this
    printf("{\"id\": \"%s\", ", id);
    if (!strcmp(entry, "hyrax_commit")) print_run_msm(MsmShape{bps, W, rows, cols, false, false}, have);
    else if (!strcmp(entry, "hyrax_commit_compressed") || !strcmp(entry, "hyrax_commit_compressed_u32")) print_run_msm(MsmShape{bps, W, rows, cols, true, false}, have);
    else if (!strcmp(entry, "hyrax_commit_rows_dev")) print_run_msm(MsmShape{bps, W, rows, cols, false, true}, have);
    else if (!strcmp(entry, "msm")) print_run_msm(MsmShape{32, MSM_WINDOWS, 1, cols, false, false}, have);
    else if (!strcmp(entry, "msm_dev_scaled")) {   // lasso_msm_dev_scaled: a row of n + 2 columns; scaling inside the latency-shaped launch, else k_scale_to_integers + run_msm
      const size_t row = cols + 2;
      if (direct && dsw::msm_fused()) { printf("\"msm\": null, \"direct\": "); print_direct(msm_direct_plan(1, row, have.mult8, dsw::msm_direct_wgs())); printf(", \"bullet\": null"); }
      else print_run_msm(MsmShape{32, MSM_WINDOWS, 1, row, false, false}, have);
    } else if (!strcmp(entry, "bullet_round")) {   // lasso_bullet_round (n = rows, nk = cols): the fused launch, else k_bullet_step + two compact rows by k_msm_direct, else two whole rows by run_msm
      const size_t n = rows, nk = cols;
      if (direct && dsw::msm_fused()) {
        printf("\"msm\": null, \"direct\": null, \"bullet\": "); print_bullet(bullet_plan(n, nk, 1, have.mult8, dsw::msm_direct_wgs()), nk, 1);
      } else if (direct) { printf("\"msm\": null, \"direct\": "); print_direct(msm_direct_plan(2, n / 2 + 2, have.mult8, dsw::msm_direct_wgs())); printf(", \"bullet\": null"); }
      else print_run_msm(MsmShape{32, MSM_WINDOWS, 2, n + 2, false, false}, have);
    } else if (!strcmp(entry, "bullet_round_slab")) {   // lasso_bullet_round_slab: always the fused launch (no switch takes it elsewhere), chunked over the rank's local columns
      if (!have.mult || world < 1 || rows % world) { fprintf(stderr, "%s: lasso_bullet_round_slab refuses this call\n", id); return 2; }
      printf("\"msm\": null, \"direct\": null, \"bullet\": "); print_bullet(bullet_plan(rows, cols, (uint32_t)world, have.mult8, dsw::msm_direct_wgs()), cols, world);
    } else if (!strcmp(entry, "msm_dev_slab")) {   // lasso_msm_dev_slab: always run_msm_direct, one row of the rank's n / world columns and the two tail columns
      if (!have.mult || world < 1 || cols % world) { fprintf(stderr, "%s: lasso_msm_dev_slab refuses this call\n", id); return 2; }
      printf("\"msm\": null, \"direct\": "); print_direct(msm_direct_plan(1, cols / world + 2, have.mult8, dsw::msm_direct_wgs())); printf(", \"bullet\": null");
    } else { fprintf(stderr, "unknown entry %s\n", entry); return 2; }
    printf("}\n");
  }
  return 0;
}
