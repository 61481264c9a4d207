"""Every row of tests/msmvariants.py reaches the kernel it names — checked on the CPU, before any of it runs on a GPU.

tests/cpp/msm_plan_dump.cpp is the device library's own decision (launch_plan.cuh over device_switches.cuh, as run_msm, run_msm_direct and bullet_round_fused call them), run once
per switch setting as a child process with that environment, for both curve builds.  Two statements:

  1. each row's plan is the row's `expect`;
  2. the union of the table's plans holds every MsmKernel and MsmResult enumerator and every loop shape of the kernels behind them: k_msm_rows8w with one row per wave and with
     several (rpw > 1, the last wave partly filled); k_msm_rows8 with one and two byte windows, one chunk and several, and at >= 1024 rows; k_msm_rows_full<8> with one chunk per row and
     several, a chunk of more than 128 columns (MSM_FULL8_COLS: more than one LDS batch) and a ragged last batch; k_msm_buckets on 4- and 32-byte scalars, each chunked;
     k_msm_pip_* with one group of rows and several; k_msm_direct and k_bullet_msm over both multiple tables, each with one chunk, several, and items per chunk at the cap;
     slab mode (lasso_bullet_round_slab, lasso_msm_dev_slab: world > 1, every rank run by the row): both mappings of k_bullet_msm's columns (wide, half >= world, and narrow), the
     boundary half == world, one chunk and several in each mapping, both tables, a first round, world == n, more fold weights than one pass of the extra workgroups' loop
     writes; k_msm_direct behind a scalar stride with one chunk and several, both tables, items per chunk at the cap.

And the shapes of test_hyrax_commit, test_hyrax_commit_u32 and test_hyrax_commit_full_width_wide_windows (tests/test_gpu_kernels.py, default switches) go through the same program:
the kernel the comments beside them name is the kernel planned.  Move MSM_SMALL_ROWS, the 1024-row bound of k_msm_rows8w or a chunking rule, and the row that lost its kernel fails
here by name."""
import pytest

import msmvariants as V

CURVES = ["curve25519", "bn254"]
FULL8_COLS = 128      # msm_kernels.cuh MSM_FULL8_COLS: columns of recoded scalars k_msm_rows_full stages in LDS at a time


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


def test_every_row_names_its_kernel():
    """a row without an expectation about WHICH kernel or table serves it would be a shape, not a lock"""
    assert all(any(k in r.expect for k in ("kernel", "direct.w8", "bullet.w8")) for r in V.TABLE)


def _msm(planned, kernel=None):
    return [(rid, p["msm"]) for rid, p in planned.items() if p["msm"] is not None and (kernel is None or p["msm"]["kernel"] == kernel)]


def _chunk_widths(m):
    """columns of every chunk of a row"""
    return [min(m["cols_per_chunk"], m["n_cols"] - k * m["cols_per_chunk"]) for k in range(m["K"])]


def test_the_table_reaches_every_kernel_result_path_and_loop_shape(planned):
    msm = _msm(planned)
    assert {m["kernel"] for _, m in msm} == {"DIRECT", "ROWS8W", "ROWS8", "PIP", "FULL8", "BUCKETS"}
    assert {m["result"] for _, m in msm} == {"FLAG", "COMPRESSED_MAPPED", "COMPRESSED_MEMCPY", "DEVICE_ROWS", "MEMCPY"}
    missing = []

    def need(what, found):
        if not found:
            missing.append(what)
    w = [m for _, m in _msm(planned, "ROWS8W")]
    need("k_msm_rows8w, one row per wave (rpw == 1)", any(m["rpw"] == 1 for m in w))
    need("k_msm_rows8w, rpw > 1 with a partly filled last wave", any(m["rpw"] > 1 and m["rows"] % m["rpw"] != 0 for m in w))
    need("k_msm_rows8w, one and two byte windows", {m["W8"] for m in w} >= {1, 2})
    r8 = [m for _, m in _msm(planned, "ROWS8")]
    need("k_msm_rows8, one and two byte windows", {m["W8"] for m in r8} >= {1, 2})
    need("k_msm_rows8, K == 1 and K > 1", any(m["K"] == 1 for m in r8) and any(m["K"] > 1 for m in r8))
    need("k_msm_rows8 at >= 1024 rows", any(m["rows"] >= 1024 for m in r8))
    f8 = [m for _, m in _msm(planned, "FULL8")]
    need("k_msm_rows_full, K == 1 and K > 1", any(m["K"] == 1 for m in f8) and any(m["K"] > 1 for m in f8))
    need("k_msm_rows_full, a chunk of more than 128 columns whose last batch is ragged", any(c > FULL8_COLS and c % FULL8_COLS for m in f8 for c in _chunk_widths(m)))
    need("k_msm_rows_full, a chunked row (K > 1) with a chunk of more than 128 columns", any(m["K"] > 1 and max(_chunk_widths(m)) > FULL8_COLS for m in f8))
    need("k_msm_rows_full, a last chunk narrower than the others", any(len(set(_chunk_widths(m))) > 1 for m in f8))
    bk = [m for _, m in _msm(planned, "BUCKETS")]
    for bps in (4, 32):
        need(f"k_msm_buckets on {bps}-byte scalars with K > 1", any(m["bps"] == bps and m["K"] > 1 for m in bk))
    pip = [m for _, m in _msm(planned, "PIP")]
    need("k_msm_pip_*, one group of rows", any(m["pip_group"] == m["rows"] for m in pip))
    need("k_msm_pip_*, several groups, the last one partly filled", any(m["pip_group"] < m["rows"] and m["rows"] % m["pip_group"] for m in pip))
    for part, kernel in (("direct", "k_msm_direct"), ("bullet", "k_bullet_msm")):
        for w8 in (True, False):
            ps = [p[part] for p in planned.values() if p[part] is not None and p[part]["w8"] == w8]
            tab = "byte-multiple" if w8 else "digit-multiple"
            need(f"{kernel} over the {tab} table, K == 1", any(p["K"] == 1 for p in ps))
            need(f"{kernel} over the {tab} table, K > 1", any(p["K"] > 1 for p in ps))
            need(f"{kernel} over the {tab} table, items per chunk at the cap", any(p["ipc"] == p["ipc_cap"] for p in ps))
    # slab mode: the rows of lasso_bullet_round_slab and lasso_msm_dev_slab (world > 1)
    slab = [(r, planned[r.id]["bullet"]) for r in V.TABLE if r.entry == "bullet_round_slab"]
    assert all(r.shape.world > 1 and p["world"] == r.shape.world and p["n_loc"] * p["world"] == r.shape.rows for r, p in slab)
    for wide in (True, False):
        name = "wide" if wide else "narrow"
        ps = [p for _, p in slab if p["wide"] == wide]
        need(f"k_bullet_msm in slab mode, {name} mapping, K == 1", any(p["K"] == 1 for p in ps))
        need(f"k_bullet_msm in slab mode, {name} mapping, K > 1", any(p["K"] > 1 for p in ps))
    need("k_bullet_msm in slab mode at the boundary half == world (one local column per weight block)", any(p["half"] == p["world"] for _, p in slab))
    need("k_bullet_msm in slab mode, narrow mapping one round below the boundary (1 < half < world)", any(1 < p["half"] < p["world"] for _, p in slab))
    need("k_bullet_msm in slab mode with world == n", any(p["n_loc"] == 1 for _, p in slab))
    need("k_bullet_msm in slab mode over both tables", {p["w8"] for _, p in slab} == {True, False})
    need("k_bullet_msm in slab mode, a first round in each of one chunk and several", {p["K"] > 1 for r, p in slab if r.shape.form == "first"} == {True, False})
    need("k_bullet_msm in slab mode, items per chunk at the cap", any(p["ipc"] == p["ipc_cap"] for _, p in slab))
    need("k_bullet_msm in slab mode, more fold weights than the 512 one pass of the two extra workgroups writes", any(r.shape.form == "fold" and p["weights"] > 512 for r, p in slab))
    sm = [(r, planned[r.id]["direct"]) for r in V.TABLE if r.entry == "msm_dev_slab"]
    need("lasso_msm_dev_slab with one chunk and several", {p["K"] > 1 for _, p in sm} == {True, False})
    need("lasso_msm_dev_slab over both tables", {p["w8"] for _, p in sm} == {True, False})
    need("lasso_msm_dev_slab with items per chunk at the cap", any(p["ipc"] == p["ipc_cap"] for _, p in sm))
    need("lasso_msm_dev_slab with world == n and with an odd number of local columns", any(r.shape.world == r.shape.cols for r, _ in sm) and any(r.shape.cols // r.shape.world % 2 for r, _ in sm))
    assert not missing, "no row of tests/msmvariants.py TABLE reaches: " + "; ".join(missing)


def test_the_scratch_covers_every_planned_launch(planned):
    """run_msm's layout behind the scalars: K partial points per row, the row sums (16-byte aligned, as pt29), the wire bytes (16-byte aligned) — inside msm_pts_bytes"""
    for rid, m in _msm(planned):
        if m["kernel"] != "DIRECT":
            assert m["pts_bytes"] >= m["rows"] * m["K"] * 144 + 15 + m["rows"] * 144 + 15 + m["rows"] * 32, rid
            assert m["K"] * m["cols_per_chunk"] >= m["n_cols"] and m["rpw"] * m["waves"] >= m["rows"], rid


@pytest.mark.parametrize("curve", CURVES)
def test_default_shapes_of_the_kernel_tests_reach_the_kernels_their_comments_name(curve):
    calls, want = [], {}
    for (ls, rs, maxv), (k_points, k_wire) in zip(V.HYRAX_COMMIT_SHAPES, V.HYRAX_COMMIT_KERNELS, strict=True):
        shape = V.Shape(ls, rs, "random" if maxv is None else ("below", maxv), V.NGENS_300)
        for entry, k in (("hyrax_commit", k_points), ("hyrax_commit_compressed", k_wire)):
            cid = f"test_hyrax_commit[{ls}-{rs}-{maxv}]:{entry}"
            calls.append((cid, entry, shape)); want[cid] = k
    for (ls, rs, tbits), k in zip(V.HYRAX_COMMIT_U32_SHAPES, V.HYRAX_COMMIT_U32_KERNELS, strict=True):
        for entry in ("hyrax_commit_compressed_u32", "hyrax_commit_compressed"):
            cid = f"test_hyrax_commit_u32[{ls}-{rs}-{tbits}]:{entry}"
            calls.append((cid, entry, V.Shape(ls, rs, ("below", 1 << tbits), V.NGENS_300))); want[cid] = k
    got = V.plans({}, calls, curve)
    bad = [f"{cid}: planned {got[cid]['msm']['kernel']}, the comment says {k}" for cid, k in want.items() if got[cid]["msm"]["kernel"] != k]
    assert not bad, "\n".join(bad)
    r8 = [got[c]["msm"] for c, k in want.items() if k == "ROWS8"]
    assert {m["W8"] for m in r8} == {1, 2} and any(m["K"] > 1 for m in r8) and any(m["n_cols"] % 256 for m in r8)      # "one and two byte windows, ragged columns", a chunked row
    r8w = [got[c]["msm"] for c, k in want.items() if k == "ROWS8W"]
    assert {m["W8"] for m in r8w} == {1, 2} and any(m["n_cols"] < 64 for m in r8w) and any(m["rows"] % 4 for m in r8w) and all(m["rpw"] == 1 for m in r8w)
    # test_hyrax_commit_full_width_wide_windows sets its three switches itself: the 12-bit-window kernels from 32 columns on, "groups" in several groups of rows, LASSO_MSM_PIP=0
    wide = [(f"wide[{ls}-{rs}-{cls}]", "hyrax_commit", V.Shape(ls, rs, "random", V.NGENS_300)) for ls, rs, cls in V.FULL_WIDTH_WIDE_SHAPES]
    on = V.plans({"LASSO_MSM_PIP_MIN_COLS": "32", "LASSO_MSM_PIP": "1"}, wide, curve)
    assert all(p["msm"]["kernel"] == "PIP" and p["msm"]["pip_group"] == p["msm"]["rows"] for p in on.values()), on
    grouped = V.plans({"LASSO_MSM_PIP_MIN_COLS": "32", "LASSO_MSM_PIP": "1", "LASSO_MSM_PIP_SCRATCH_MB": "16"}, [c for c in wide if "groups" in c[0]], curve)
    assert all(p["msm"]["kernel"] == "PIP" and p["msm"]["pip_group"] == 64 and p["msm"]["rows"] % 64 for p in grouped.values()), grouped
    off = V.plans({"LASSO_MSM_PIP_MIN_COLS": "32", "LASSO_MSM_PIP": "0"}, wide, curve)
    assert all(p["msm"]["kernel"] == "BUCKETS" for p in off.values()), off
