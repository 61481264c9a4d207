"""Every row of tests/passvariants.py makes the running sum it names reach its fold — checked on the CPU, before any of it runs on a GPU.

tests/cpp/pass_plan_dump.cpp is the device library's own decision about a launch's grid (round_nx, cubic_plan, reduce_nx and matvec_plan of launch_plan.cuh over
device_switches.cuh), run once per switch setting as a child process with that environment, for both curve builds.  From the grid follow the passes of its loop every workgroup
makes: workgroup x of nx takes ceil((blocks - x) / nx) of the launch's blocks.  Statements:

  1. each row's claim (`fold+`, `carry`, `stage2 k`: tests/passvariants.py) holds for the grid planned;
  2. every kernel and instantiation that keeps a lazily reduced running sum has a `fold+` or `carry` row, the lanes-per-index kernels one per T;
  3. every row is the only one of its setting and data set to reach one thing: a row that goes, or moves to another kernel, is reported by what is no longer reached;
  4. the periods in the table are the ones in the source: `& 127u`, `& 63u`, `++cnt == 3` and `LT_FOLD_EVERY() 32u` are read from the .cuh / .hip text of each kernel (or of the
     macro or function its body names); the caps the reduction launches pass to reduce_nx and the dispatch tables of the lanes-per-index kernels are read there too.  A period that
     changes fails here with the kernel's name, so that the row's shape is revisited."""
import os
import re

import pytest

import passvariants as V

CURVES = ["curve25519", "bn254"]
CSRC = os.path.join(V.ROOT, "lasso_amd", "csrc")


@pytest.fixture(scope="module", params=CURVES)
def planned(request):
    """{row id: grid} of the whole table on one curve build: one run of the plan program per switch setting"""
    out = {}
    for env in V.ENVS:
        out.update(V.plans(env, V.rows_of(env), request.param))
    return out


def test_every_row_keeps_its_claim(planned):
    bad = [f"{r.id} ({r.kernel}, period {r.period}, {r.per_pass} items per workgroup and pass): {why}" for r in V.TABLE for why in [V.claim_failure(r, planned[r.id])] if why]
    assert not bad, "\n".join(bad)


def test_the_cubic_rows_get_the_kernel_they_name(planned):
    """cubic_plan's form, sums and accumulator width are the instantiation in the row's `kernel`"""
    for r in V.TABLE:
        if r.entry in V.CUBIC_ENTRIES:
            p = planned[r.id]
            k = f"k_cubic_eqw_lb<{p['NT']}>" if p["form"] == "LB" else f"k_cubic_eqw_fused<{p['NT']}>" if p["NT"] == 3 else f"k_cubic_eqw_fused<2, {'wide' if p['is_wide'] else 'narrow'}>"
            assert p["form"] in ("LB", "FUSED") and k == r.kernel, f"{r.id}: planned {p['form']} {k}, the table names {r.kernel}"


def test_the_settings_are_the_ones_the_issue_names():
    assert {V.env_id(e) for e in V.ENVS} == {"LASSO_CUBIC_NX=3", "LASSO_CUBIC_NX=3,LASSO_CUBIC_WIDE=0", "LASSO_REDUCE_NX=3", "default"}
    assert all(set(e) <= set(V.SWITCHES) for e in V.ENVS)
    # every row on uniform data and on the data that maximises its sums (the LT round from bits: both extreme patterns)
    for env in V.ENVS:
        by_call = {}
        for r in V.rows_of(env):
            by_call.setdefault((r.entry, tuple(r.args.items())), set()).add(r.data)
        assert all(d == set(V.data_sets(entry)) for (entry, _), d in by_call.items())


def _lanes(kernel):
    """T of a lanes-per-index instantiation: k_combine_round_lt<A, D, T ..>, k_combine_round_lt_u32<A, D, T>, k_combine_round_custom<D, T, MULTI>"""
    targs = [x.strip() for x in kernel.split("<")[1].rstrip(">").split(",")]
    return int(targs[1] if kernel.startswith("k_combine_round_custom<") else targs[2])


def test_every_kernel_that_keeps_a_running_sum_reaches_its_fold(planned):
    reached = {r.kernel for r in V.TABLE if r.claim in ("fold+", "carry") and V.claim_failure(r, planned[r.id]) is None}
    missing = [k for k in V.REQUIRED_KERNELS if k not in reached]
    assert not missing, "no row of tests/passvariants.py TABLE folds the running sum of: " + "; ".join(missing)
    # the lanes-per-index kernels once per T
    lanes = lambda prefix, suffix=">": {_lanes(k) for k in reached if k.startswith(prefix) and k.endswith(suffix) and ("PROD" in k) == ("PROD" in suffix)}
    assert lanes("k_combine_round_lt<") == {1, 2, 3} and lanes("k_combine_round_lt<", "PROD>") == {1, 2, 3} and lanes("k_combine_round_lt_u32<") == {1, 2, 3}
    assert lanes("k_combine_round_custom<", "false>") == {1, 2, 3} and lanes("k_combine_round_custom<", "true>") == {1, 2, 3, 5}
    assert {r.period for r in V.TABLE if r.claim != "carry" and not r.claim.startswith("stage2")} == {32, 64, 128}
    assert {int(r.claim.split()[1]) for r in V.TABLE if r.claim.startswith("stage2")} == {2, 4}
    # at least one term list of the caller-defined strategies makes pack_custom_terms set a fold mark (flag 4); the coefficient-1 paths are there
    assert any(V.sets_fold_mark(n) for n in V.CUSTOM_TERMS) and not all(V.sets_fold_mark(n) for n in V.CUSTOM_TERMS)
    assert any(cf == 1 for t in V.CUSTOM_TERMS.values() for cf, _ in t)


def _needs():
    """{setting: [(what the setting must reach, the entry point that reaches it, predicate over a row)]}: what each child process of tests/test_gpu_pass_variants.py is there for"""
    def need(what, kernel, entry, claim, **args):
        return (what, entry, lambda r: r.kernel == kernel and r.entry == entry and r.claim == claim and all(r.args.get(k) == v for k, v in args.items()))
    cn3 = [need("the 128-fold of k_cubic_round_lb", "k_cubic_round_lb", "cubic_round", "fold+"),
           need("the 128-fold of k_cubic_eqw_lb<3>", "k_cubic_eqw_lb<3>", "eqw_round", "fold+"),
           need("the 128-fold of k_cubic_eqw_fused<3>", "k_cubic_eqw_fused<3>", "eqw_round_fused", "fold+"),
           need("the carries of k_cubic_eqw_lb<2>", "k_cubic_eqw_lb<2>", "eqw2_begin", "carry"),
           need("the carries of k_cubic_eqw_fused<2, wide>", "k_cubic_eqw_fused<2, wide>", "eqw2_begin_r", "carry")]
    for alpha in (1, 3):
        for kernel, entry, n in (("k_dot_eqw_lb", "linear_eqw_round", 1 << 13), ("k_dot_eqw_lb_u32", "linear_eqw_round_u32", 1 << 13), ("k_dot_eqw_fused<false>", "linear_eqw_round_fused", 1 << 14),
                                 ("k_dot_eqw_fused<false>", "linear_eqw_round_fused_from", 1 << 14), ("k_dot_eqw_fused_from_u32", "linear_eqw_round_fused_from_u32", 1 << 14),
                                 ("k_dot_eqw_fused<true>", "linear_eqw_round_fused_ahead", 1 << 14)):
            cn3.append(need(f"the carries of {kernel} through {entry}, alpha = {alpha}", kernel, entry, "carry", alpha=alpha, n=n))
    cn3 += [need("57 carries in a row in k_dot_eqw_lb", "k_dot_eqw_lb", "linear_eqw_round", "carry", n=1 << 18),
            need("57 carries in a row in k_dot_eqw_fused<false>", "k_dot_eqw_fused<false>", "linear_eqw_round_fused", "carry", n=1 << 19)]
    rn3 = [need("the 64-fold of k_combine_round_linear over AND's weights", "k_combine_round_linear", "combine_round", "fold+", kind="and"),
           need("the 64-fold of k_combine_round_linear over the range check's weights", "k_combine_round_linear", "combine_round", "fold+", kind="range")]
    for c in (1, 2, 4, 8, 16):
        k = "k_combine_round_lt<%d, %d, %d>" % V.lt_instance(2 * c)
        rn3.append(need(f"the 32-fold of {k} behind k_lt_prescale's copies", k, "combine_round", "fold+", kind="lt", c=c))
        rn3.append(need(f"the 32-fold of {k} on the caller's scaled arrays", k, "combine_round_lt_scaled", "fold+", c=c))
    for c in (3, 8, 16):
        k = "k_combine_round_lt<%d, %d, %d, PROD>" % V.lt_instance(2 * c)
        rn3.append(need(f"the 32-fold of {k}", k, "combine_round", "fold+", kind="spark", c=c))
    for c in (4, 8, 16):
        k = "k_combine_round_lt_u32<%d, %d, %d>" % V.lt_instance(2 * c)
        rn3.append(need(f"the 32-fold of {k}", k, "combine_round_lt_u32", "fold+", c=c))
    for kind, c, a in (("and", 1, 2), ("lt", 16, 32), ("range", 4, 4)):
        rn3.append(need(f"the 128-fold of k_combine_claim<{a}> ({kind})", f"k_combine_claim<{a}>", "combine_claim", "fold+", kind=kind, c=c))
    for name in V.CUSTOM_TERMS:
        multi = len(V.CUSTOM_TERMS[name]) > 1
        k = "k_combine_round_custom<%d, %d, %s>" % (*V.custom_instance(V.custom_degree(name), multi), "true" if multi else "false")
        rn3.append(need(f"the 32-fold of {k} (`{name}`)", k, "combine_round", "fold+", strategy=name))
        rn3.append(need(f"the 128-fold of k_combine_claim_custom over `{name}`", "k_combine_claim_custom", "combine_claim", "fold+", strategy=name))
    rn3 += [need("the 128-fold of k_inner_lr", "k_inner_lr", "inner_products_lr", "fold+"),
            need("the carries of k_multi_dot with a partly filled last block", "k_multi_dot", "multi_dot", "carry", k=2)]
    default = [need("the second stage over 512 partials of 3 values", "reduce_partials_row", "combine_round", "stage2 2"),
               need("the second stage over 1024 partials of 3 values", "reduce_partials_row", "combine_round", "stage2 4"),
               need("the second stage over 1024 partials of one value", "reduce_partials_row", "combine_claim", "stage2 4"),
               need("the carries of k_multi_dot at its own cap of 512 workgroups", "k_multi_dot", "multi_dot", "carry", k=1)]
    for entry in ("matvec_left", "matvec_left_dev"):
        default += [need(f"the carries of k_matvec_left through lasso_{entry}", "k_matvec_left", entry, "carry"),
                    need(f"the 128-fold of k_matvec_reduce through lasso_{entry}", "k_matvec_reduce", entry, "fold+")]
    return {"LASSO_CUBIC_NX=3": cn3, "LASSO_CUBIC_NX=3,LASSO_CUBIC_WIDE=0": [need("the 128-fold of k_cubic_eqw_fused<2, narrow>", "k_cubic_eqw_fused<2, narrow>", "eqw2_begin_r", "fold+")],
            "LASSO_REDUCE_NX=3": rn3, "default": default}


def test_every_row_is_the_only_one_to_reach_what_it_is_there_for(planned):
    needs = _needs()
    assert set(needs) == {V.env_id(e) for e in V.ENVS}
    missing, twice, idle = [], [], []
    for env in V.ENVS:
        rows = [r for r in V.rows_of(env) if V.claim_failure(r, planned[r.id]) is None]
        for what, entry, pred in needs[V.env_id(env)]:
            for data in V.data_sets(entry):
                hits = [r.id for r in rows if r.data == data and pred(r)]
                if not hits:
                    missing.append(f"[{V.env_id(env)}] {what}, {data} data")
                if len(hits) > 1:
                    twice.append(f"[{V.env_id(env)}] {what}, {data} data: {hits}")
        idle += [r.id for r in V.rows_of(env) if not any(pred(r) for _, _, pred in needs[V.env_id(env)])]
        assert len({r.purpose for r in V.rows_of(env)}) == len(V.rows_of(env)), "two rows of one setting name the same purpose"
    assert not missing, "no row of tests/passvariants.py TABLE reaches: " + "; ".join(missing)
    assert not twice, "more than one row for: " + "; ".join(twice)
    assert not idle, "rows that reach nothing their setting is there for: " + ", ".join(idle)


# ---- the periods, caps and dispatch tables in the source

def _read(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def _kernel_body(text, name):
    """the text of __global__ kernel `name`: from its name to the next kernel, macro or section"""
    m = re.search(r"__global__ void[^\n]*?\b" + re.escape(name) + r"\(", text)
    assert m, f"kernel {name} is no longer in the source"
    rest = text[m.end():]
    end = re.search(r"\n(?:template|__global__|#define|#undef|// -{20})", rest)
    return rest[:end.start()] if end else rest


def _macro_body(text, name):
    m = re.search(r"#define " + re.escape(name) + r"\b", text)
    assert m, f"macro {name} is no longer in the source"
    lines = text[m.start():].split("\n")
    out = []
    for ln in lines:
        out.append(ln)
        if not ln.rstrip().endswith("\\"):
            break
    return "\n".join(out)


def _function_body(text, signature):
    m = re.search(re.escape(signature), text)
    assert m, f"`{signature}` is no longer in the source"
    return text[m.start():text.index("\n}\n", m.start())]


def _periods_in(body):
    """every fold period a piece of source states literally"""
    return ({int(x) + 1 for x in re.findall(r"\(\+\+\w+ & (\d+)u\) == 0", body)} | {int(x) for x in re.findall(r"\+\+cnt == (\d+)\)", body)})


# kernel as the rows name it -> (file, kernel in the source, what its body must name for the period to be the macro's or function's: None = the body states it itself)
SOURCES = {
    "k_cubic_round_lb": ("poly_kernels.cuh", "k_cubic_round_lb", "CUBIC_ACCUMULATE"), "k_cubic_eqw_lb<3>": ("poly_kernels.cuh", "k_cubic_eqw_lb", "CUBIC_ACCUMULATE"),
    "k_cubic_eqw_fused<3>": ("poly_kernels.cuh", "k_cubic_eqw_fused", "CUBIC_ACCUMULATE"), "k_cubic_eqw_fused<2, narrow>": ("poly_kernels.cuh", "k_cubic_eqw_fused", "CUBIC_ACCUMULATE2"),
    "k_cubic_eqw_lb<2>": ("poly_kernels.cuh", "k_cubic_eqw_lb", None), "k_cubic_eqw_fused<2, wide>": ("poly_kernels.cuh", "k_cubic_eqw_fused", None),
    "k_dot_eqw_lb": ("poly_kernels.cuh", "k_dot_eqw_lb", "DOT_EQW_LB_BODY"), "k_dot_eqw_lb_u32": ("poly_kernels.cuh", "k_dot_eqw_lb_u32", "DOT_EQW_LB_BODY"),
    "k_dot_eqw_fused<false>": ("poly_kernels.cuh", "k_dot_eqw_fused", "DOT_EQW_FUSED_BODY"), "k_dot_eqw_fused<true>": ("poly_kernels.cuh", "k_dot_eqw_fused", "DOT_EQW_FUSED_BODY"),
    "k_dot_eqw_fused_from_u32": ("poly_kernels.cuh", "k_dot_eqw_fused_from_u32", "DOT_EQW_FUSED_BODY"),
    "k_multi_dot": ("poly_kernels.cuh", "k_multi_dot", None), "k_matvec_left": ("poly_kernels.cuh", "k_matvec_left", None), "k_matvec_reduce": ("poly_kernels.cuh", "k_matvec_reduce", "acc_add"),
    "k_combine_claim": ("poly_kernels.cuh", "k_combine_claim", "acc_add"), "k_combine_claim_custom": ("poly_kernels.cuh", "k_combine_claim_custom", "acc_add"),
    "k_inner_lr": ("lasso_hip.hip", "k_inner_lr", None), "k_combine_round_linear": ("poly_kernels.cuh", "k_combine_round_linear", None),
    "k_combine_round_lt": ("poly_kernels.cuh", "k_combine_round_lt", "LT_FOLD_EVERY"), "k_combine_round_lt_u32": ("poly_kernels.cuh", "k_combine_round_lt_u32", "LT_FOLD_EVERY"),
    "k_combine_round_custom": ("poly_kernels.cuh", "k_combine_round_custom", "LT_FOLD_EVERY"),
}


def _source_period(kernel):
    """the fold period of `kernel` as the source states it today, with the place it was read from"""
    key = kernel if kernel in SOURCES else kernel.split("<")[0]
    fname, name, via = SOURCES[key]
    text = _read(fname)
    body = _kernel_body(text, name)
    if via is None:
        found, where = _periods_in(body), f"{name} in {fname}"
    else:
        assert re.search(re.escape(via) + r"\b", body), f"{name} no longer uses {via}: its fold period has to be read elsewhere"
        if via == "LT_FOLD_EVERY":
            m = re.search(r"#define LT_FOLD_EVERY\(\) (\d+)u", text)
            assert m, "#define LT_FOLD_EVERY() <N>u is no longer in poly_kernels.cuh"
            assert re.search(r"\+\+cnt >= LT_FOLD_EVERY\(\)", body), f"{name} no longer folds at `++cnt >= LT_FOLD_EVERY()`"
            found = {int(m.group(1))}
        elif via == "acc_add":
            found = _periods_in(_function_body(text, "void acc_add("))
        else:
            found = _periods_in(_macro_body(text, via))
        where = f"{via} ({fname}), which {name} uses"
    return found, where


def test_the_periods_in_the_table_are_the_ones_in_the_source():
    bad = []
    for kernel, period in sorted({(r.kernel, r.period) for r in V.TABLE if not r.claim.startswith("stage2")}):
        found, where = _source_period(kernel)
        if period not in found or (len(found) > 1 and kernel.split("<")[0] not in ("k_cubic_eqw_lb", "k_cubic_eqw_fused")):
            bad.append(f"{kernel}: the table says it folds every {period} passes; {where} now states {sorted(found)} — revisit the shapes of its rows in tests/passvariants.py")
    assert not bad, "\n".join(bad)
    # the second stage: one pass of reduce_partials_row per blockDim.x = LASSO_BLOCK = 256 partials
    text = _read("poly_kernels.cuh")
    assert "for (uint32_t x = threadIdx.x; x < nx; x += blockDim.x)" in _function_body(text, "void reduce_partials_row(")
    assert re.search(r"#define LASSO_BLOCK 256\b", _read("launch_plan.cuh"))


def test_the_items_per_pass_are_the_kernels():
    """256 indices per workgroup and pass, 256 / T for the lanes-per-index kernels (SLOTS = LASSO_BLOCK / T, T the third template argument the row names)"""
    text = _read("poly_kernels.cuh")
    for name in ("k_combine_round_lt", "k_combine_round_lt_u32", "k_combine_round_custom"):
        body = _kernel_body(text, name)
        assert "constexpr uint32_t SLOTS = LASSO_BLOCK / T;" in body and "i += (size_t)gridDim.x * SLOTS" in body, name
    for r in V.TABLE:
        base = r.kernel.split("<")[0]
        if base in ("k_combine_round_lt", "k_combine_round_lt_u32", "k_combine_round_custom"):
            assert r.per_pass == 256 // _lanes(r.kernel), r.id
        elif base in ("k_matvec_left", "k_matvec_reduce"):
            assert r.per_pass == 1, r.id       # a pass is a row of its chunk / a chunk
        else:
            assert r.per_pass == 256, r.id


def test_the_caps_and_dispatch_tables_are_the_sources():
    hip = _read("lasso_hip.hip")
    sites = {"combine_round": ["static int32_t combine_round_custom(", "static int32_t combine_round_impl("], "combine_round_lt_u32": ["int32_t lasso_sumcheck_combine_round_lt_u32("],
             "combine_claim": ["static int32_t combine_claim_custom(", "int32_t lasso_combine_claim("], "multi_dot": ["int32_t lasso_multi_dot("],
             "inner_products_lr": ["int32_t lasso_inner_products_lr("]}
    for entry, sigs in sites.items():
        for sig in sigs:
            caps = re.findall(r"nx = reduce_nx\(\w+, (\d+)\)", _function_body(hip, sig))
            assert caps == [str(V.REDUCE_CAPS[entry])], f"{sig}: reduce_nx caps {caps}, the table has {V.REDUCE_CAPS[entry]}"
    assert V.REDUCE_CAPS["combine_round_lt_scaled"] == V.REDUCE_CAPS["combine_round"]      # the same combine_round_impl
    # the switch applies to the round kernel only: k_lt_prescale keeps grid_for
    assert "k_lt_prescale, dim3(grid_for(n, 1024), S.c - 1)" in _function_body(hip, "static int32_t combine_round_impl(")
    lt = re.findall(r"\(alpha\) <= (\d+)\) \{ FN\((\d+), (\d+), (\d+)\)", _macro_body(hip, "DISPATCH_LT")) + re.findall(r"else \{ FN\((\d+), (\d+), (\d+)\); \} \} while", _macro_body(hip, "DISPATCH_LT"))
    assert [(int(x[-3]), int(x[-2]), int(x[-1])) for x in lt] == V.LT_DISPATCH
    cu = _macro_body(hip, "DISPATCH_CUSTOM")
    got = {False: [], True: []}
    for d, t, multi in re.findall(r"FN\((\d+), (\d+), (false|true)\)", cu):
        got[multi == "true"].append((int(d), int(d), int(t)))
    assert got == V.CUSTOM_DISPATCH
    assert [int(x) for x in re.findall(r"FN\((\d+), \d+\)", _macro_body(hip, "DISPATCH_A"))] == V.CLAIM_DISPATCH
