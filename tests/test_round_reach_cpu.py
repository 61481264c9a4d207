"""Every row of tests/roundvariants.py reaches the kernel instantiation it names — checked on the CPU, before any of it runs on a GPU.

tests/cpp/cubic_plan_dump.cpp is the device library's own decision (cubic_plan of launch_plan.cuh over device_switches.cuh, with the CubicShape each lasso_sumcheck_cubic_* entry
point builds), run once per switch setting as a child process with that environment, for both curve builds.  Two statements:

  1. each row's plan is the row's `expect`;
  2. the union of the table's plans holds every instantiation and loop shape cubic_eqw_launch_t selects among: k_cubic_eqw_small<BIND, NT> over both pointer tables, at 64 indices
     per circuit and at one; k_cubic_eqw_fused with three sums, two wide and two narrow, launched ahead wide and narrow with the wait behind k_gate and inside the kernel, at the
     boundary of LASSO_AHEAD_INKERNEL_WGS, on one partly filled workgroup and on a grid at its cap, with block sums direct and through the second stage on both sides of
     LASSO_DIRECT_NX; k_cubic_eqw_lb with three sums, EqNone pipelined, plain and non-temporal, EqInline at 7 and 14 coordinates, EqInlineMem, EqGlobal ungated and gated with equal
     and unequal factor tables, k_eq_outer behind k_eq_small2 and behind k_eq_small2_mem; every CubicForm, every CubicEq, and the refusal.

And the shapes of the six cubic-round tests of tests/test_gpu_kernels.py (default switches) go through the same program: the form the comment beside each list names is the form
planned.  Move CUBIC_SMALL_Q, the 2^14-entry bound of the in-LDS table or a grid rule, and the row that lost its kernel fails here by name."""
import pytest

import roundvariants as V

CURVES = ["curve25519", "bn254"]


@pytest.fixture(scope="module", params=CURVES)
def planned(request):
    """{row id: plan} of the whole table on one curve build: one run of the plan program per switch setting"""
    out = {}
    for env in V.ENVS:
        out.update(V.plans(env, [(r.id, r.entry, r.shape) for r in V.rows_of(env)], request.param))
    return out


def test_every_row_gets_the_plan_it_expects(planned):
    bad = [f"{r.id} [{V.env_id(r.env)}] {r.entry} {tuple(r.shape)}: " + "; ".join(m) for r in V.TABLE for m in [V.plan_mismatches(planned[r.id], r.expect)] if m]
    assert not bad, "\n".join(bad)


def test_every_row_names_its_form_and_its_eq_source():
    """a row without an expectation about WHICH kernel serves it would be a shape, not a lock"""
    assert all("form" in r.expect for r in V.TABLE)
    assert all("lb.eq" in r.expect and "lb.nt" in r.expect and "lb.pipe" in r.expect for r in V.TABLE if r.expect["form"] == "LB")
    assert all("refusal" in r.expect for r in V.TABLE if r.expect["form"] == "REFUSED")


def test_the_settings_are_the_ones_the_switches_offer():
    ids = {V.env_id(e) for e in V.ENVS}
    assert ids >= {"default", "LASSO_CUBIC_WIDE=0", "LASSO_LB_NT=1", "LASSO_LB_PIPELINE=0", "LASSO_LB_NT=1,LASSO_LB_PIPELINE=0", "LASSO_EQ_INLINE_BIG=1", "LASSO_DIRECT_NX=0",
                   "LASSO_DIRECT_NX=64", "LASSO_AHEAD_INKERNEL_WGS=0", "LASSO_AHEAD_INKERNEL_WGS=4096", "LASSO_CUBIC_NX=64", "LASSO_TAGGED_RESULTS=0"}
    assert any(r.shape.prof & V.PROF_CUBIC and not r.env for r in V.TABLE)
    assert all(set(e) <= set(V.SWITCHES) for e in V.ENVS)


def _nx_cap(p):
    """round_nx's cap on the x-extent of the plan's grid"""
    return p["sw"]["cubic_nx"] if p["sw"]["cubic_nx"] > 0 else max(512 // p["ny"], 64)


def test_the_table_reaches_every_form_eq_source_and_loop_shape(planned):
    ps = list(planned.values())
    assert {p["form"] for p in ps} == {"REFUSED", "SMALL", "LB", "FUSED"}
    lb = [p for p in ps if p["form"] == "LB"]
    assert {p["lb"]["eq"] for p in lb} == {"TABLE", "LDS", "GATED", "FACTORS"}
    missing = []

    def need(what, found):
        if not found:
            missing.append(what)
    tables = ("8", "full")
    small = [p for p in ps if p["form"] == "SMALL"]
    for bind in (False, True):
        for nt in (2, 3):
            for t in tables:
                need(f"k_cubic_eqw_small<{str(bind).lower()}, {nt}> over the pointer table `{t}`", any(p["bind"] == bind and p["NT"] == nt and p["ptr_table"] == t for p in small))
    need("k_cubic_eqw_small at 64 indices per circuit, the last size it serves", any(p["items"] == 64 for p in small))
    need("k_cubic_eqw_small at one index per circuit", any(p["items"] == 1 for p in small))
    need("k_cubic_eqw_small with the bind at 64 and at one", {p["items"] for p in small if p["bind"]} >= {1, 64})

    fused = [p for p in ps if p["form"] == "FUSED"]
    now = [p for p in fused if not p["gate"] and not p["inkernel"]]
    ahead = [p for p in fused if p["gate"] or p["inkernel"]]
    for t in tables:
        need(f"k_cubic_eqw_fused<3> over the pointer table `{t}`", any(p["NT"] == 3 and p["ptr_table"] == t for p in now))
        need(f"k_cubic_eqw_fused<2, wide> over the pointer table `{t}`", any(p["NT"] == 2 and p["wide"] and p["ptr_table"] == t for p in now))
        need(f"k_cubic_eqw_fused<2, narrow> over the pointer table `{t}`", any(p["NT"] == 2 and not p["wide"] and p["ptr_table"] == t for p in now))
        need(f"k_cubic_eqw_fused launched ahead over the pointer table `{t}`", any(p["ptr_table"] == t for p in ahead))
    for wide in (True, False):
        for wait in ("gate", "inkernel"):
            need(f"k_cubic_eqw_fused launched ahead, {'wide' if wide else 'narrow'}, waiting by `{wait}`", any(p["wide"] == wide and p[wait] for p in ahead))
    need("a round launched ahead on exactly ahead_inkernel_wgs workgroups (inside the kernel)", any(p["inkernel"] and p["nx"] * p["ny"] == p["sw"]["ahead_inkernel_wgs"] for p in ahead))
    need("a round launched ahead on ahead_inkernel_wgs + 1 workgroups (behind the gate)", any(p["gate"] and p["nx"] * p["ny"] == p["sw"]["ahead_inkernel_wgs"] + 1 for p in ahead))
    need("a round launched ahead whose in-kernel wait profiling turned into the gate", any(p["gate"] and p["nx"] * p["ny"] <= p["sw"]["ahead_inkernel_wgs"] for p in ahead))
    need("k_cubic_eqw_fused on 128 indices: one partly filled workgroup", any(p["items"] == 128 and p["nx"] == 1 for p in fused))
    need("k_cubic_eqw_fused with nx at its cap and several passes per workgroup", any(p["nx"] == _nx_cap(p) and p["items"] > p["nx"] * 256 for p in fused))
    need("k_cubic_eqw_fused, direct block sums at nx == direct_nx", any(p["direct"] and p["nx"] == p["sw"]["direct_nx"] for p in fused))
    need("k_cubic_eqw_fused, the second stage at nx == direct_nx + 1", any(not p["direct"] and p["nx"] == p["sw"]["direct_nx"] + 1 for p in fused))
    need("k_cubic_eqw_fused, the second stage where nobody takes groups (flag protocol)", any(not p["direct"] and not p["sw"]["tagged"] and 1 < p["nx"] <= p["sw"]["direct_nx"] for p in fused))

    need("k_cubic_eqw_lb<3>", any(p["NT"] == 3 for p in lb))
    two = [p for p in lb if p["NT"] == 2]
    plain = [p for p in two if p["lb"]["eq"] == "TABLE" and not p["lb"]["eq_outer"]]
    need("k_cubic_eqw_lb<2, EqNone> pipelined", any(p["lb"]["pipe"] == 1 and not p["lb"]["nt"] for p in plain))
    need("k_cubic_eqw_lb<2, EqNone> with the plain loop (pipe == 0)", any(p["lb"]["pipe"] == 0 for p in plain))
    need("k_cubic_eqw_lb<2, EqNone, NTL>", any(p["lb"]["nt"] for p in plain))
    need("k_cubic_eqw_lb<2, EqNone, NTL> on one partly filled workgroup, at a capped grid with several passes, over both pointer tables",
         any(p["lb"]["nt"] and p["items"] == 128 for p in plain) and any(p["lb"]["nt"] and p["nx"] == _nx_cap(p) and p["items"] > p["nx"] * 256 for p in plain)
         and {p["ptr_table"] for p in plain if p["lb"]["nt"]} == set(tables))
    need("LASSO_LB_NT=1 without the pipeline: nt stays off", any(r.env == {"LASSO_LB_NT": "1", "LASSO_LB_PIPELINE": "0"} and not planned[r.id]["lb"]["nt"] and planned[r.id]["lb"]["pipe"] == 0
                                                              for r in V.TABLE if planned[r.id]["form"] == "LB"))
    lds = [p for p in two if p["lb"]["eq"] == "LDS"]
    need("k_cubic_eqw_lb<2, EqInline> at 7 and at 14 coordinates", {p["ell"] for p in lds} >= {7, 14})
    need("k_cubic_eqw_lb<2, EqInline> at an odd number of coordinates above 7 (factor tables of different sizes)", any(p["ell"] % 2 and p["ell"] > 7 for p in lds))
    gated = [p for p in two if p["lb"]["eq"] == "GATED"]
    need("k_cubic_eqw_lb<2, EqInlineMem> at up to 14 coordinates", any(p["ell"] <= 14 and p["lb"]["gate"] for p in gated))
    need("k_cubic_eqw_lb<2, EqInlineMem> at 7 and at 14 coordinates", {p["ell"] for p in gated} >= {7, 14})
    fac = [p for p in two if p["lb"]["eq"] == "FACTORS"]
    for is_gated in (False, True):
        g = [p for p in fac if p["lb"]["gate"] == is_gated and p["lb"]["factors_gated"] == is_gated]
        need(f"k_cubic_eqw_lb<2, EqGlobal> {'gated' if is_gated else 'ungated'}, g_hi != g_lo", any(p["lb"]["g_hi"] != p["lb"]["g_lo"] for p in g))
        need(f"k_cubic_eqw_lb<2, EqGlobal> {'gated' if is_gated else 'ungated'}, g_hi == g_lo", any(p["lb"]["g_hi"] == p["lb"]["g_lo"] for p in g))
    outer = [p for p in two if p["lb"]["eq_outer"]]
    need("k_eq_outer behind k_eq_small2", any(p["lb"]["factors"] and not p["lb"]["factors_gated"] and not p["lb"]["gate"] for p in outer))
    need("k_eq_outer behind k_eq_small2_mem", any(p["lb"]["factors_gated"] and p["lb"]["gate"] for p in outer))
    need("k_eq_outer in front of the plain loop (pipe == 0)", any(p["lb"]["pipe"] == 0 for p in outer))
    need("k_cubic_eqw_lb with direct block sums and through the second stage", {p["direct"] for p in lb} == {True, False})
    need("k_cubic_eqw_lb, direct block sums at nx == direct_nx and the second stage at direct_nx + 1",
         any(p["direct"] and p["nx"] == p["sw"]["direct_nx"] for p in lb) and any(not p["direct"] and p["nx"] == p["sw"]["direct_nx"] + 1 for p in lb))
    for eq in ("TABLE", "LDS", "GATED"):
        need(f"k_cubic_eqw_lb reading `{eq}` over both pointer tables", {p["ptr_table"] for p in lb if p["lb"]["eq"] == eq} == set(tables))
    need("k_cubic_eqw_lb<2, EqGlobal> and k_eq_outer's round over the full pointer table", any(p["ptr_table"] == "full" for p in fac) and any(p["ptr_table"] == "full" for p in outer))
    need("k_cubic_eqw_lb on one partly filled workgroup and at a capped grid with several passes",
         any(p["items"] == 128 and p["nx"] == 1 for p in lb) and any(p["nx"] == _nx_cap(p) and p["items"] > p["nx"] * 256 for p in lb))
    need("an x-extent that is no power of two (an uneven number of passes per workgroup)", any(p["nx"] & (p["nx"] - 1) for p in fused) and any(p["nx"] & (p["nx"] - 1) for p in lb))

    refused = [(r, planned[r.id]) for r in V.TABLE if planned[r.id]["form"] == "REFUSED"]
    need("a refused round: lasso_sumcheck_cubic_eqw2_begin_ahead at n / 4 <= 64, with its message",
         any(r.entry == "eqw2_begin_ahead" and r.shape.n // 4 <= 64 and p["refusal"] == V.REFUSAL_AHEAD for r, p in refused))
    assert not missing, "no row of tests/roundvariants.py TABLE reaches: " + "; ".join(missing)


_EQ = {"TABLE": "EqNone", "LDS": "EqInline", "GATED": "EqInlineMem", "FACTORS": "EqGlobal"}


def _kernel(p):
    """the instantiation cubic_eqw_launch_t launches for a plan, as the source spells it"""
    if p["form"] == "SMALL":
        return f"small<{str(p['bind']).lower()}, {p['NT']}>"
    if p["form"] == "FUSED":
        return f"fused<{p['NT']}, {'wide' if p['wide'] else 'narrow'}>" + ("/gate" if p["gate"] else "/inkernel" if p["inkernel"] else "")
    if p["form"] == "LB":
        l = p["lb"]
        front = ("/k_eq_small2_mem" if l["factors_gated"] else "/k_eq_small2" if l["factors"] else "") + ("+k_eq_outer" if l["eq_outer"] else "")
        return f"lb<{p['NT']}, {_EQ[l['eq']]}{', NTL' if l['nt'] else ''}>" + front
    return "refused"


def _per_setting_needs():
    """{setting: [(what the setting must reach, predicate over a plan)]}: what each child process of tests/test_gpu_round_variants.py is there for.  Every row of the table is
    the only one of its setting that meets one of these, so a row that goes — or moves to another kernel — is reported by what is no longer reached."""
    K = _kernel
    one_wg = lambda p: p["nx"] == 1 and p["items"] == 128                         # one workgroup, half of it idle
    stage2 = lambda p: p["nx"] > 1 and not p["direct"]                            # the in-launch second stage
    at_cap = lambda p: p["nx"] == _nx_cap(p) and p["items"] > p["nx"] * 256        # the grid at its cap, several passes per workgroup
    wgs = lambda p: p["nx"] * p["ny"]
    t8, full = (lambda p: p["ptr_table"] == "8"), (lambda p: p["ptr_table"] == "full")
    hi_ne_lo = lambda p: p["lb"]["g_hi"] != p["lb"]["g_lo"]
    plain_lb = "lb<2, EqNone>"
    needs = {
        "default": [(f"k_cubic_eqw_{k} over the pointer table `{t}`", lambda p, k=k, t=t: K(p) == k and p["ptr_table"] == t)
                    for k in ("small<false, 2>", "small<false, 3>", "small<true, 2>", "small<true, 3>") for t in ("8", "full")] + [
            ("fused<3> on one partly filled workgroup", lambda p: K(p) == "fused<3, narrow>" and one_wg(p)),
            ("fused<3> over the full pointer table, block sums direct", lambda p: K(p) == "fused<3, narrow>" and full(p) and p["direct"]),
            ("fused<2, wide> on one partly filled workgroup", lambda p: K(p) == "fused<2, wide>" and one_wg(p)),
            ("fused<2, wide> over the full pointer table", lambda p: K(p) == "fused<2, wide>" and full(p)),
            ("fused<2, wide>, block sums direct at nx == direct_nx", lambda p: K(p) == "fused<2, wide>" and p["direct"] and p["nx"] == p["sw"]["direct_nx"]),
            ("fused<2, wide> through the second stage", lambda p: K(p) == "fused<2, wide>" and stage2(p)),
            ("a round launched ahead on exactly ahead_inkernel_wgs workgroups, waiting inside its kernel", lambda p: K(p) == "fused<2, wide>/inkernel" and wgs(p) == p["sw"]["ahead_inkernel_wgs"]),
            ("a round launched ahead on ahead_inkernel_wgs + 1 workgroups, behind k_gate, full pointer table", lambda p: K(p) == "fused<2, wide>/gate" and wgs(p) == p["sw"]["ahead_inkernel_wgs"] + 1 and full(p)),
            ("a round launched ahead behind k_gate, through the second stage", lambda p: K(p) == "fused<2, wide>/gate" and stage2(p)),
            ("a profiled round launched ahead: the in-kernel wait turned into k_gate", lambda p: K(p) == "fused<2, wide>/gate" and wgs(p) <= p["sw"]["ahead_inkernel_wgs"]),
            ("the refusal of a round launched ahead", lambda p: K(p) == "refused" and p["refusal"] == V.REFUSAL_AHEAD),
            ("lb<3> on one workgroup", lambda p: K(p) == "lb<3, EqNone>" and p["nx"] == 1),
            ("lb<3> over the full pointer table, block sums direct", lambda p: K(p) == "lb<3, EqNone>" and full(p) and p["direct"]),
            ("lb<2, EqNone> pipelined, block sums direct at nx == direct_nx", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 1 and p["direct"] and p["nx"] == p["sw"]["direct_nx"]),
            ("lb<2, EqNone> pipelined over the full pointer table at a capped grid", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 1 and full(p) and at_cap(p)),
            ("lb<2, EqInline> at 7 coordinates", lambda p: K(p) == "lb<2, EqInline>" and p["ell"] == 7),
            ("lb<2, EqInline> at an odd number of coordinates above 7, full pointer table", lambda p: K(p) == "lb<2, EqInline>" and p["ell"] > 7 and p["ell"] % 2 and full(p)),
            ("lb<2, EqInline> at 14 coordinates", lambda p: K(p) == "lb<2, EqInline>" and p["ell"] == 14),
            ("lb<2, EqInlineMem> at 7 coordinates, full pointer table", lambda p: K(p) == "lb<2, EqInlineMem>" and p["ell"] == 7 and full(p)),
            ("lb<2, EqInlineMem> at an odd number of coordinates above 7, block sums direct", lambda p: K(p) == "lb<2, EqInlineMem>" and p["ell"] > 7 and p["ell"] % 2 and p["direct"]),
            ("lb<2, EqInlineMem> at 14 coordinates", lambda p: K(p) == "lb<2, EqInlineMem>" and p["ell"] == 14),
            ("k_eq_small2 + k_eq_outer in front of round 0, factor tables of different sizes", lambda p: K(p) == plain_lb + "/k_eq_small2+k_eq_outer" and hi_ne_lo(p) and t8(p)),
            ("k_eq_small2 + k_eq_outer in front of round 0, factor tables of equal size", lambda p: K(p) == plain_lb + "/k_eq_small2+k_eq_outer" and not hi_ne_lo(p)),
            ("k_eq_small2 + k_eq_outer in front of round 0 over the full pointer table", lambda p: K(p) == plain_lb + "/k_eq_small2+k_eq_outer" and full(p)),
            ("k_eq_small2_mem + k_eq_outer in front of round 0, factor tables of different sizes", lambda p: K(p) == plain_lb + "/k_eq_small2_mem+k_eq_outer" and hi_ne_lo(p)),
            ("k_eq_small2_mem + k_eq_outer in front of round 0, factor tables of equal size", lambda p: K(p) == plain_lb + "/k_eq_small2_mem+k_eq_outer" and not hi_ne_lo(p))],
        "LASSO_CUBIC_WIDE=0": [
            ("fused<2, narrow> on one partly filled workgroup", lambda p: K(p) == "fused<2, narrow>" and one_wg(p)),
            ("fused<2, narrow> over the full pointer table, block sums direct", lambda p: K(p) == "fused<2, narrow>" and full(p) and p["direct"]),
            ("fused<2, narrow> through the second stage", lambda p: K(p) == "fused<2, narrow>" and stage2(p)),
            ("fused<2, narrow> launched ahead, waiting inside its kernel", lambda p: K(p) == "fused<2, narrow>/inkernel"),
            ("fused<2, narrow> launched ahead behind k_gate", lambda p: K(p) == "fused<2, narrow>/gate")],
        "LASSO_LB_NT=1": [
            ("lb<2, EqNone, NTL> on one partly filled workgroup", lambda p: K(p) == "lb<2, EqNone, NTL>" and one_wg(p)),
            ("lb<2, EqNone, NTL>, block sums direct", lambda p: K(p) == "lb<2, EqNone, NTL>" and p["direct"]),
            ("lb<2, EqNone, NTL> over the full pointer table at a capped grid", lambda p: K(p) == "lb<2, EqNone, NTL>" and full(p) and at_cap(p)),
            ("a round launched ahead behind a non-temporal round 0", lambda p: K(p).startswith("fused<2, wide>/")),
            ("lb<3> stays as it is", lambda p: K(p) == "lb<3, EqNone>"),
            ("lb<2, EqInline> stays as it is", lambda p: K(p) == "lb<2, EqInline>"),
            ("the round behind k_eq_outer stays as it is", lambda p: K(p) == plain_lb + "/k_eq_small2+k_eq_outer")],
        "LASSO_LB_PIPELINE=0": [
            ("lb<2, EqNone>, plain loop, on one partly filled workgroup", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 0 and one_wg(p)),
            ("lb<2, EqNone>, plain loop, block sums direct", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 0 and p["direct"]),
            ("lb<2, EqNone>, plain loop, over the full pointer table at a capped grid", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 0 and full(p) and at_cap(p)),
            ("lb<2, EqInline> stays pipelined", lambda p: K(p) == "lb<2, EqInline>" and p["lb"]["pipe"] == 1),
            ("the plain loop behind k_eq_small2 + k_eq_outer", lambda p: K(p) == plain_lb + "/k_eq_small2+k_eq_outer" and p["lb"]["pipe"] == 0),
            ("the plain loop behind k_eq_small2_mem + k_eq_outer", lambda p: K(p) == plain_lb + "/k_eq_small2_mem+k_eq_outer" and p["lb"]["pipe"] == 0)],
        "LASSO_LB_NT=1,LASSO_LB_PIPELINE=0": [
            ("nt stays off without the pipeline, one partly filled workgroup", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 0 and one_wg(p)),
            ("nt stays off without the pipeline, block sums direct", lambda p: K(p) == plain_lb and p["lb"]["pipe"] == 0 and p["direct"])],
        "LASSO_EQ_INLINE_BIG=1": [
            ("lb<2, EqGlobal> ungated, factor tables of different sizes", lambda p: K(p) == "lb<2, EqGlobal>/k_eq_small2" and hi_ne_lo(p) and t8(p)),
            ("lb<2, EqGlobal> ungated, factor tables of equal size", lambda p: K(p) == "lb<2, EqGlobal>/k_eq_small2" and not hi_ne_lo(p)),
            ("lb<2, EqGlobal> ungated over the full pointer table", lambda p: K(p) == "lb<2, EqGlobal>/k_eq_small2" and full(p)),
            ("lb<2, EqGlobal> gated, factor tables of different sizes", lambda p: K(p) == "lb<2, EqGlobal>/k_eq_small2_mem" and p["lb"]["gate"] and hi_ne_lo(p)),
            ("lb<2, EqGlobal> gated, factor tables of equal size", lambda p: K(p) == "lb<2, EqGlobal>/k_eq_small2_mem" and p["lb"]["gate"] and not hi_ne_lo(p)),
            ("lb<2, EqInline> at 14 coordinates stays as it is", lambda p: K(p) == "lb<2, EqInline>" and p["ell"] == 14),
            ("lb<2, EqInlineMem> at 14 coordinates stays as it is", lambda p: K(p) == "lb<2, EqInlineMem>" and p["ell"] == 14)],
        "LASSO_DIRECT_NX=0": [(f"{k} through the second stage on a grid that goes out direct by default", lambda p, k=k: K(p) == k and 1 < p["nx"] <= 16 and not p["direct"])
                              for k in ("fused<2, wide>", "fused<3, narrow>", plain_lb, "lb<3, EqNone>", "fused<2, wide>/inkernel", "lb<2, EqInline>")],
        "LASSO_DIRECT_NX=64": [
            ("fused<2, wide>, 64 groups direct", lambda p: K(p) == "fused<2, wide>" and p["direct"] and p["nx"] == 64),
            ("fused<2, wide> over the full pointer table, 32 groups direct", lambda p: K(p) == "fused<2, wide>" and p["direct"] and p["nx"] == 32 and full(p)),
            ("fused<3>, more than 16 groups direct", lambda p: K(p) == "fused<3, narrow>" and p["direct"] and p["nx"] > 16),
            ("lb<2, EqNone> over the full pointer table, 64 groups direct", lambda p: K(p) == plain_lb and p["direct"] and p["nx"] == 64 and full(p)),
            ("lb<3>, 64 groups direct", lambda p: K(p) == "lb<3, EqNone>" and p["direct"] and p["nx"] == 64),
            ("a round launched ahead, more than 16 groups direct", lambda p: K(p) == "fused<2, wide>/gate" and p["direct"] and p["nx"] > 16),
            ("lb<2, EqInline>, 64 groups direct", lambda p: K(p) == "lb<2, EqInline>" and p["direct"] and p["nx"] == 64),
            ("lb<2, EqInlineMem>, 64 groups direct", lambda p: K(p) == "lb<2, EqInlineMem>" and p["direct"] and p["nx"] == 64)],
        "LASSO_AHEAD_INKERNEL_WGS=0": [
            ("k_gate in front of a single workgroup", lambda p: K(p) == "fused<2, wide>/gate" and wgs(p) == 1),
            ("k_gate in front of the 32 workgroups that wait inside their kernel by default", lambda p: K(p) == "fused<2, wide>/gate" and wgs(p) == 32)],
        "LASSO_AHEAD_INKERNEL_WGS=4096": [
            ("the in-kernel wait over the full pointer table", lambda p: K(p) == "fused<2, wide>/inkernel" and full(p)),
            ("the in-kernel wait on 64 workgroups", lambda p: K(p) == "fused<2, wide>/inkernel" and wgs(p) == 64),
            ("the in-kernel wait on 256 workgroups", lambda p: K(p) == "fused<2, wide>/inkernel" and wgs(p) == 256)],
        "LASSO_CUBIC_NX=64": [(f"{k} at the cap of 64, several passes per workgroup", lambda p, k=k: K(p) == k and p["nx"] == 64 and at_cap(p))
                              for k in ("fused<2, wide>", "fused<3, narrow>", plain_lb, "fused<2, wide>/gate", plain_lb + "/k_eq_small2+k_eq_outer")],
        "LASSO_CUBIC_NX=17": [
            ("fused<2, wide> through the second stage at nx == direct_nx + 1", lambda p: K(p) == "fused<2, wide>" and not p["direct"] and p["nx"] == p["sw"]["direct_nx"] + 1),
            ("lb<2, EqNone> through the second stage at nx == direct_nx + 1", lambda p: K(p) == plain_lb and not p["direct"] and p["nx"] == p["sw"]["direct_nx"] + 1),
            ("a round launched ahead at nx == direct_nx + 1", lambda p: K(p) == "fused<2, wide>/gate" and not p["direct"] and p["nx"] == p["sw"]["direct_nx"] + 1),
            ("fused<2, wide>, block sums direct at nx == direct_nx under the same cap", lambda p: K(p) == "fused<2, wide>" and p["direct"] and p["nx"] == p["sw"]["direct_nx"])],
        "LASSO_TAGGED_RESULTS=0": [("k_cubic_eqw_small through the flag protocol", lambda p: K(p).startswith("small<"))] + [
            (f"{k} through the flag protocol: no block sums direct", lambda p, k=k: K(p) == k and p["nx"] > 1 and not p["direct"] and not p["sw"]["tagged"])
            for k in ("fused<2, wide>", plain_lb, "lb<3, EqNone>", "fused<2, wide>/inkernel", "fused<2, wide>/gate", "lb<2, EqInline>", "lb<2, EqInlineMem>", plain_lb + "/k_eq_small2_mem+k_eq_outer")],
    }
    return needs


def test_every_setting_reaches_what_it_is_there_for(planned):
    needs = _per_setting_needs()
    assert set(needs) == {V.env_id(e) for e in V.ENVS}
    missing, idle = [], []
    for env in V.ENVS:
        rows = V.rows_of(env)
        for what, pred in needs[V.env_id(env)]:
            if not any(pred(planned[r.id]) for r in rows):
                missing.append(f"[{V.env_id(env)}] {what}")
        idle += [r.id for r in rows if not any(pred(planned[r.id]) for _, pred in needs[V.env_id(env)])]
    assert not missing, "no row of tests/roundvariants.py TABLE reaches: " + "; ".join(missing)
    assert not idle, "rows that reach nothing their setting is there for: " + ", ".join(idle)


def test_the_scratch_covers_every_planned_launch(planned):
    """cubic_eqw_launch_t's layout: 3 partials per workgroup, the two factor tables behind them — inside scratch_elems; a direct launch's groups fit wait_flag's limit of 64"""
    for rid, p in planned.items():
        if p["form"] in ("LB", "FUSED"):
            assert p["part_elems"] == p["nx"] * p["ny"] * 3 and 1 <= p["nx"] <= _nx_cap(p), rid
            extra = (1 << p["lb"]["g_hi"]) + (1 << p["lb"]["g_lo"]) if p["lb"] and p["lb"]["factors"] else 0
            assert p["scratch_elems"] >= p["part_elems"] + extra, rid
            assert not p["direct"] or 1 < p["nx"] <= 64, rid


@pytest.mark.parametrize("curve", CURVES)
def test_default_shapes_of_the_kernel_tests_reach_the_forms_their_comments_name(curve):
    S = V.Shape
    calls, want = [], {}

    def call(cid, entry, n, k, form, **more):
        calls.append((cid, entry, S(n, k, 0))); want[cid] = {"form": form, **more}
    for n, k in V.CUBIC_EQW_ROUND_SHAPES:          # "n <= 128: latency-shaped kernel"
        call(f"eqw_round[{n}-{k}]", "eqw_round", n, k, "SMALL" if n <= 128 else "LB", NT=3)
    for n, k in V.CUBIC_EQW_ROUND_FUSED_SHAPES:    # "n <= 256: latency-shaped kernel"; the test's second call is the plain round on the bound half
        call(f"eqw_round_fused[{n}-{k}]", "eqw_round_fused", n, k, "SMALL" if n <= 256 else "FUSED", NT=3, bind=True)
        call(f"eqw_round_fused[{n}-{k}]:again", "eqw_round", n // 2, k, "SMALL" if n // 2 <= 128 else "LB")
    for n, k in V.CUBIC_EQW2_SHAPES:
        call(f"eqw2[{n}-{k}]", "eqw2_begin", n, k, "SMALL" if n <= 128 else "LB", NT=2, **({} if n <= 128 else {"lb.eq": "TABLE", "lb.pipe": 1, "lb.nt": False}))
        if n >= 4:
            call(f"eqw2[{n}-{k}]:r", "eqw2_begin_r", n, k, "SMALL" if n <= 256 else "FUSED", NT=2, bind=True, **({} if n <= 256 else {"wide": True}))
    for n, k in V.CUBIC_ROUND_AHEAD_SHAPES:
        if n // 8 <= 64:                           # "too short for the streaming kernel": the test asks for a round of 256 and expects the refusal
            call(f"ahead[{n}-{k}]:256", "eqw2_begin_ahead", 256, k, "REFUSED", refusal=V.REFUSAL_AHEAD)
        else:
            for m in (n, n // 2, n // 4):          # two rounds launched ahead and served, a third abandoned
                call(f"ahead[{n}-{k}]:{m}", "eqw2_begin_ahead", m, k, "FUSED", NT=2, bind=True, wide=True)
    for n, k, _ in V.CUBIC_ROUND0_EQ_SHAPES:       # "above 2^14 entries: factor tables in memory"
        big = n // 2 > 1 << 14
        call(f"round0_eq[{n}-{k}]", "eqw2_begin_eq", n, k, "LB", **{"lb.eq": "TABLE" if big else "LDS", "lb.factors": big, "lb.eq_outer": big, "lb.gate": False})
    for n, k, _, _ in V.LAYER_AHEAD_SHAPES:
        if n // 2 > 1 << 9:                        # up to 2^9 entries the resident tail serves the layer: no cubic round
            big = n // 2 > 1 << 14
            call(f"layer_ahead[{n}-{k}]", "eqw2_begin_eq_ahead", n, k, "LB", **{"lb.eq": "TABLE" if big else "GATED", "lb.factors_gated": big, "lb.eq_outer": big, "lb.gate": True})
    got = V.plans({}, calls, curve)
    bad = [f"{cid}: " + "; ".join(m) for cid, w in want.items() for m in [V.plan_mismatches(got[cid], w)] if m]
    assert not bad, "\n".join(bad)
    # both sides of every comment's boundary are among the shapes
    assert {got[c]["form"] for c in got if c.startswith("eqw_round[")} == {"SMALL", "LB"} and {got[c]["form"] for c in got if c.startswith("eqw_round_fused[") and ":" not in c} == {"SMALL", "FUSED"}
    assert {got[c]["lb"]["eq"] for c in got if c.startswith("round0_eq[")} == {"LDS", "TABLE"} and {got[c]["lb"]["eq"] for c in got if c.startswith("layer_ahead[")} == {"GATED", "TABLE"}
    assert {got[c]["gate"] for c in got if c.startswith("ahead[") and got[c]["form"] == "FUSED"} == {True, False}      # both forms of the wait
    # test_big_eq_tables_formed_inside_round0_in_their_own_process re-runs the last two lists under LASSO_EQ_INLINE_BIG=1: EqGlobal above 2^14 entries, nothing else moves
    eq_calls = [c for c in calls if c[1] in ("eqw2_begin_eq", "eqw2_begin_eq_ahead")]
    big = V.plans({"LASSO_EQ_INLINE_BIG": "1"}, eq_calls, curve)
    for cid, _, shape in eq_calls:
        if shape.n // 2 > 1 << 14:
            assert big[cid]["lb"]["eq"] == "FACTORS" and not big[cid]["lb"]["eq_outer"] and big[cid]["lb"]["factors"], cid
        else:
            assert big[cid]["lb"] == got[cid]["lb"], cid
