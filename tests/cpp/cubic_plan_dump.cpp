// Which kernel serves an eq-weighted cubic round of the device library, as lasso_hip.hip decides it: cubic_plan of lasso_amd/csrc/launch_plan.cuh over the switches of
// lasso_amd/csrc/device_switches.cuh, both included as they are (as tests/cpp/test_launch_plan_host.cpp and tests/cpp/msm_plan_dump.cpp include them).  tests/roundvariants.py runs
// this program once per switch setting, as a child process with that environment (the switches are read once per process), and tests/test_round_reach_cpu.py holds every row of its
// table to the plan printed here.
// stdin, one call per line:   <id> <entry> <n> <ncirc> <ell> <prof>
//   entry: eqw_round | eqw_round_fused | eqw2_begin | eqw2_begin_r | eqw2_begin_ahead | eqw2_begin_eq | eqw2_begin_eq_ahead — the lasso_sumcheck_cubic_* entry point of that name
//          (eqw2_begin_r: lasso_sumcheck_cubic_eqw2_begin with a challenge to bind first)
//   n, ncirc: length of every array, number of circuits; ell: the eq point's length (2^ell = n / 2; read by the last two entries only)
//   prof: the context's profiling mask (lasso_prof_enable)
// stdout, one JSON object per line: the CubicPlan, the CubicLbPlan in "lb" for an evaluation-only round (null otherwise), the pointer-table width cubic_eqw_launch picks, and the
// switch values the plan was made under.
#include <cstdio>
#include <cstring>
#include "../../lasso_amd/csrc/device_switches.cuh"
#include "../../lasso_amd/csrc/launch_plan.cuh"

namespace dsw = lasso::dsw;

static const char* form_name(CubicForm f) {
  switch (f) { case CUBIC_REFUSED: return "REFUSED"; case CUBIC_SMALL: return "SMALL"; case CUBIC_LB: return "LB"; case CUBIC_FUSED: return "FUSED"; }
  return "?";
}
static const char* eq_name(CubicEq e) {
  switch (e) { case CUBIC_EQ_TABLE: return "TABLE"; case CUBIC_EQ_LDS: return "LDS"; case CUBIC_EQ_GATED: return "GATED"; case CUBIC_EQ_FACTORS: return "FACTORS"; }
  return "?";
}
static const char* tf(bool b) { return b ? "true" : "false"; }

int main() {
  char id[128], entry[64];
  size_t n; unsigned ncirc, ell, prof;
  const CubicSwitches sw = {dsw::cubic_nx(), dsw::cubic_wide(), dsw::direct_nx(), dsw::eq_inline_big(), dsw::lb_pipeline(), dsw::lb_nt(), dsw::ahead_inkernel_wgs()};
  const bool tagged = dsw::tagged_results();   // lasso_ctx_create: c->tagged
  while (scanf("%127s %63s %zu %u %u %u", id, entry, &n, &ncirc, &ell, &prof) == 6) {
    // cubic_plan_for(c, ncirc, n, has_r, NT, has_eqi, want_groups, ahead, eqg, gate_ell) as each entry point calls it; every one of them passes groups_out
    int NT = 2; bool has_r = false, ahead = false, has_eqi = false, has_eqg = false; int gate_ell = -1;
    if (!strcmp(entry, "eqw_round")) NT = 3;
    else if (!strcmp(entry, "eqw_round_fused")) { NT = 3; has_r = true; }
    else if (!strcmp(entry, "eqw2_begin")) { }
    else if (!strcmp(entry, "eqw2_begin_r")) has_r = true;
    else if (!strcmp(entry, "eqw2_begin_ahead")) ahead = true;
    else if (!strcmp(entry, "eqw2_begin_eq")) { if (ell <= 14) has_eqi = true; else has_eqg = true; }   // make_eq_inline takes points of up to 14 coordinates
    else if (!strcmp(entry, "eqw2_begin_eq_ahead")) gate_ell = (int)ell;
    else { fprintf(stderr, "unknown entry %s\n", entry); return 2; }
    const CubicShape s = {n, ncirc, NT, ahead, has_r, has_eqi, has_eqg, has_eqg ? ell : 0u, gate_ell, prof, /* groups_out passed */ true && tagged};
    const CubicPlan p = cubic_plan(s, sw);
    printf("{\"id\": \"%s\", \"form\": \"%s\", \"NT\": %d, \"bind\": %s, \"items\": %zu, \"nx\": %u, \"ny\": %u, \"direct\": %s, \"wide\": %s, \"gate\": %s, \"inkernel\": %s, \"refusal\": ",
           id, form_name(p.form), NT, tf(p.bind), p.items, p.nx, p.ny, tf(p.direct), tf(p.wide), tf(p.gate), tf(p.inkernel));
    if (p.refusal) printf("\"%s\"", p.refusal); else printf("null");
    printf(", \"part_elems\": %zu, \"scratch_elems\": %zu, \"lb\": ", p.part_elems, p.scratch_elems);
    if (p.form == CUBIC_LB) {
      const CubicLbPlan& l = p.lb;
      printf("{\"eq\": \"%s\", \"gate\": %s, \"factors\": %s, \"factors_gated\": %s, \"eq_outer\": %s, \"g_ell\": %u, \"g_hi\": %u, \"g_lo\": %u, \"pipe\": %u, \"nt\": %s}",
             eq_name(l.eq), tf(l.gate), tf(l.factors), tf(l.factors_gated), tf(l.eq_outer), l.g_ell, l.g_hi, l.g_lo, l.pipe, tf(l.nt));
    } else printf("null");
    // cubic_eqw_launch: MutPtrTable8 / PtrTable8 up to 8 circuits, the full tables above
    printf(", \"ptr_table\": \"%s\", \"ell\": %u, \"sw\": {\"cubic_nx\": %ld, \"direct_nx\": %u, \"ahead_inkernel_wgs\": %u, \"tagged\": %s}}\n",
           ncirc <= 8 ? "8" : "full", ell, sw.cubic_nx, sw.direct_nx, sw.ahead_inkernel_wgs, tf(tagged));
  }
  return 0;
}
