// The grid a summing launch of the device library gets, as lasso_hip.hip decides it: round_nx, cubic_plan, reduce_nx and matvec_plan of lasso_amd/csrc/launch_plan.cuh over the
// switches of lasso_amd/csrc/device_switches.cuh, both included as they are (as tests/cpp/cubic_plan_dump.cpp includes them).  tests/passvariants.py runs this program once per
// switch setting, as a child process with that environment (the switches are read once per process), and tests/test_pass_reach_cpu.py works out from the grids printed here how
// many passes of its loop every workgroup of a row makes.
// stdin, one launch per line:   <id> <kind> <a> <b> <c>
//   round  <items> <ny> 0        the linear rounds and lasso_sumcheck_cubic_round: round_nx(items, ny, LASSO_CUBIC_NX)
//   eqw_round | eqw_round_fused | eqw2_begin | eqw2_begin_r  <n> <ncirc> 0      the lasso_sumcheck_cubic_* entry point of that name (eqw2_begin_r: with a challenge to bind first)
//   reduce <items> <cap> 0       a reduction launch outside the round grids with its own cap: reduce_nx(items, cap, LASSO_REDUCE_NX)
//   matvec <l_size> <r_size> 0   lasso_matvec_left / lasso_matvec_left_dev: matvec_plan
// stdout, one JSON object per line.
#include <cstdio>
#include <cstring>
#include "../../lasso_amd/csrc/device_switches.cuh"
#include "../../lasso_amd/csrc/launch_plan.cuh"

namespace dsw = lasso::dsw;

int main() {
  char id[192], kind[64];
  size_t a, b, c;
  const CubicSwitches sw = {dsw::cubic_nx(), dsw::cubic_wide(), dsw::direct_nx(), dsw::eq_inline_big(), dsw::lb_pipeline(), dsw::lb_nt(), dsw::ahead_inkernel_wgs()};
  while (scanf("%191s %63s %zu %zu %zu", id, kind, &a, &b, &c) == 5) {
    printf("{\"id\": \"%s\", \"kind\": \"%s\", \"sw\": {\"cubic_nx\": %ld, \"reduce_nx\": %ld, \"wide\": %s}, ", id, kind, dsw::cubic_nx(), dsw::reduce_nx(), sw.wide ? "true" : "false");
    if (!strcmp(kind, "round")) printf("\"items\": %zu, \"nx\": %u, \"ny\": %zu}\n", a, round_nx(a, (unsigned)b, dsw::cubic_nx()), b);
    else if (!strcmp(kind, "reduce")) printf("\"items\": %zu, \"nx\": %u, \"ny\": 1}\n", a, reduce_nx(a, (unsigned)b, dsw::reduce_nx()));
    else if (!strcmp(kind, "matvec")) { const MatvecPlan p = matvec_plan(a, b); printf("\"col_blocks\": %zu, \"nchunks\": %zu, \"rows_per_chunk\": %zu}\n", p.col_blocks, p.nchunks, p.rows_per_chunk); }
    else {
      int NT = 2; bool has_r = false;
      if (!strcmp(kind, "eqw_round")) NT = 3;
      else if (!strcmp(kind, "eqw_round_fused")) { NT = 3; has_r = true; }
      else if (!strcmp(kind, "eqw2_begin")) { }
      else if (!strcmp(kind, "eqw2_begin_r")) has_r = true;
      else { fprintf(stderr, "unknown kind %s\n", kind); return 2; }
      const CubicShape s = {a, (uint32_t)b, NT, false, has_r, false, false, 0u, -1, 0u, dsw::tagged_results()};
      const CubicPlan p = cubic_plan(s, sw);
      printf("\"form\": \"%s\", \"NT\": %d, \"is_wide\": %s, \"items\": %zu, \"nx\": %u, \"ny\": %u}\n",
             p.form == CUBIC_LB ? "LB" : p.form == CUBIC_FUSED ? "FUSED" : p.form == CUBIC_SMALL ? "SMALL" : "REFUSED", NT, p.wide ? "true" : "false", p.items, p.nx, p.ny);
    }
  }
  return 0;
}
