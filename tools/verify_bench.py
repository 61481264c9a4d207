#!/usr/bin/env python3
"""Time HostProver.verify with the proof's and the commitment's compressed points decoded on the host (LASSO_VERIFY_DEVICE_POINTS=0: one point after the other on one CPU
thread, the only path before the device decoder existed) and on the device (the default: ONE lasso_points_decompress call per proof, include/lasso_hip_wire.h).

AND, C = 1, M = 2^16 at 2^10, 2^16, 2^20 and 2^24 lookups on curve25519 (2^24 is the headline instance) and at 2^20 on BN254.  The switches are read once per process,
so every (instance, setting) is measured in a fresh child process: it proves once, verifies `--runs` times (host clock around verify), and — with the device decoder —
reports the kernel's own time from the library's event brackets (lasso_prof_*, family LASSO_K_MISC, in an extra verify that is not among the timed ones).

Writes one JSON file (default profiles/verify_device_points.json) with, per instance, median / min / max of both settings, the ratio, and whether the acceptance condition
holds: the default is not slower than the host path by more than the host path's own spread.  Needs the built libraries and a GPU; nothing here falls back to a CPU.

--ab msm_points: the same five instances with the verifier's MSMs over commitment rows table-free (the default: lasso_msm_points, include/lasso_hip_msm.h) against
LASSO_VERIFY_MSM_POINTS=0 (lasso_bases_create + lasso_msm + lasso_bases_destroy per call, the only path before).  Per setting, beside the verify times: the host timers
of Verifier::msm_points' phases and of the G_hat MSM (LASSO_TRACE=2 buckets, mean per verify over the timed runs) and the peak device bytes during a verify
(lasso_host_mem_stats).  Default output: profiles/verify_msm_points.json.

--ab mle: caller-defined strategies (linear g, C = 1, one memory per subtable, random 32-bit tables) with log_m in {8, 12, 16, 20, 24} x subtables in {1, 4, 16} at 2^16
lookups on curve25519, the subtables' MLEs by the host loop (LASSO_VERIFY_DEVICE_MLE=0: the only path of the parent commit) against one lasso_tables_mle call per verify
(LASSO_MLE_DEVICE_MIN=0: the threshold out of the way).  A fresh process per setting, the two settings of an instance one after the other.  Beside the verify times: the
device call's own time (lasso_prof_*, families LASSO_K_DOT + LASSO_K_EQ, in an extra verify) and its table bytes per second as a share of the MI355X's 8 TB/s HBM peak.
Reports the smallest measured num_subtables * 2^log_m at which the device route's max is below the host route's min: what LASSO_MLE_DEVICE_MIN defaults to.
--only takes names like m16k4.  Default output: profiles/verify_device_mle.json."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

INSTANCES = [("curve25519", 10), ("curve25519", 16), ("curve25519", 20), ("curve25519", 24), ("bn254", 20)]


def child(curve, log_s, runs):
    import numpy as np  # noqa: F401
    from lasso_amd import HostProver, _abi
    from lasso_amd.device import load_device_library
    hp = HostProver(curve=curve)
    c, log_m, s = 1, 16, 1 << log_s
    idx = hp.gen_indices(s, 1 << log_m, c); r = hp.gen_random_point(log_s)
    S = _abi.Strategy(_abi.KINDS["and"], c, log_m, 0)
    gens = hp.gens(c, s, c, log_m); hp.gens_prepare(gens)
    dense = hp.densify(idx, log_m)
    comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, S, r)
    hp.free(dense)
    assert hp.verify(gens, S, s, r, proof, comm) is True      # warm-up: buffers, tables
    hp.wire_stats(reset=True); hp.msm_stats(reset=True)
    live_before = hp.mem_stats(reset=True)["live_bytes"]
    sys.stderr.write("VERIFY_BENCH_TIMED_BEGIN\n"); sys.stderr.flush()
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ok = hp.verify(gens, S, s, r, proof, comm)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert ok is True
    sys.stderr.write("VERIFY_BENCH_TIMED_END\n"); sys.stderr.flush()
    mem = hp.mem_stats()
    points = hp.wire_stats()["device_points"] // runs
    msm_calls = hp.msm_stats()["points_calls"] // runs
    kernel_ms = None
    if points:
        lib = load_device_library(curve=curve)      # the same shared object the host library is linked against
        ctx = C.c_void_p(hp.ctx())
        lib.lasso_prof_reset(ctx); lib.lasso_prof_enable(ctx, 1 << _abi.K_MISC)
        assert hp.verify(gens, S, s, r, proof, comm) is True
        n, t, b = C.c_uint64(), C.c_double(), C.c_double()
        lib.lasso_prof_get(ctx, _abi.K_MISC, C.byref(n), C.byref(t), C.byref(b))
        lib.lasso_prof_enable(ctx, 0)
        kernel_ms = t.value
    hp.free(None, gens); hp.close()
    print("VERIFY_BENCH " + json.dumps({"curve": curve, "log_s": log_s, "verify_ms": ms, "device_points_per_verify": points, "kernel_ms": kernel_ms, "proof_bytes": len(proof),
                                        "commitment_bytes": len(comm), "msm_points_calls_per_verify": msm_calls, "live_bytes_before": live_before,
                                        "peak_bytes_during_verifies": mem["peak_bytes"]}))


MLE_LOG_MS, MLE_SUBTABLES, MLE_LOG_S = [8, 12, 16, 20, 24], [1, 4, 16], 16
HBM_PEAK_BYTES_PER_S = 8e12      # MI355X data sheet


def child_mle(log_m, k, runs):
    import numpy as np
    from lasso_amd import CustomStrategy, HostProver, _abi
    from lasso_amd.device import load_device_library
    hp = HostProver()
    s = 1 << MLE_LOG_S
    rng = np.random.default_rng(1000 * log_m + k)
    tables = [rng.integers(0, 2**32, size=1 << log_m, dtype=np.uint64).astype(np.uint32) for _ in range(k)]
    cs = CustomStrategy(1, log_m, tables, [(1 + i, [i]) for i in range(k)], num_memories=k, memory_subtable=list(range(k)), memory_dimension=[0] * k)
    idx = hp.gen_indices(s, 1 << log_m, 1); r = hp.gen_random_point(MLE_LOG_S)
    gens = hp.gens(1, s, k, log_m); hp.gens_prepare(gens)
    dense = hp.densify(idx, log_m)
    comm = hp.commit(dense, gens); proof = hp.prove(dense, gens, cs, r)
    hp.free(dense)
    assert hp.verify(gens, cs, s, r, proof, comm) is True      # warm-up: buffers, tables
    hp.mle_stats(reset=True)
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        ok = hp.verify(gens, cs, s, r, proof, comm)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert ok is True
    tables_dev = hp.mle_stats()["device_tables"] // runs
    call_ms = None
    if tables_dev:
        lib = load_device_library()
        ctx = C.c_void_p(hp.ctx())
        lib.lasso_prof_reset(ctx); lib.lasso_prof_enable(ctx, (1 << _abi.K_DOT) | (1 << _abi.K_EQ))
        assert hp.verify(gens, cs, s, r, proof, comm) is True
        call_ms = 0.0
        for fam in (_abi.K_DOT, _abi.K_EQ):
            n, t, b = C.c_uint64(), C.c_double(), C.c_double()
            lib.lasso_prof_get(ctx, fam, C.byref(n), C.byref(t), C.byref(b))
            call_ms += t.value
        lib.lasso_prof_enable(ctx, 0)
    hp.free(None, gens); hp.close()
    print("VERIFY_BENCH " + json.dumps({"log_m": log_m, "subtables": k, "verify_ms": ms, "device_tables_per_verify": tables_dev, "device_call_ms": call_ms, "proof_bytes": len(proof)}))


def write_mle(a, runs, rows):
    # the threshold: the smallest measured size from which EVERY measured size has the device route's max below the host route's min
    by_size = sorted(rows, key=lambda r: r["entries"])
    threshold = None
    for i, r in enumerate(by_size):
        if all(q["device_max_below_host_min"] for q in by_size[i:]):
            threshold = r["entries"]; break
    out = {"what": "HostProver.verify of caller-defined strategies at 2^16 lookups, the subtables' MLEs by the host loop (LASSO_VERIFY_DEVICE_MLE=0: the parent commit's only "
                   "path) against one lasso_tables_mle call (LASSO_MLE_DEVICE_MIN=0); same session, same machine, a fresh process per setting, the two settings of an instance "
                   "back to back; median of the timed verifies with [min, max]", "runs_per_setting": runs, "hbm_peak_bytes_per_s_assumed": HBM_PEAK_BYTES_PER_S, "rows": rows,
           "smallest_measured_entries_from_which_device_max_is_below_host_min": threshold}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)


def main_mle(a, runs):
    rows = []
    for log_m in MLE_LOG_MS:
        for k in MLE_SUBTABLES:
            name = f"m{log_m}k{k}"
            if a.only and name not in a.only.split(","):
                continue
            off = run_child("mle", f"{log_m}:{k}", runs, {"LASSO_VERIFY_DEVICE_MLE": "0"})
            on = run_child("mle", f"{log_m}:{k}", runs, {"LASSO_MLE_DEVICE_MIN": "0"})
            assert off["device_tables_per_verify"] == 0 and on["device_tables_per_verify"] == k
            so, sn = summary(off["verify_ms"]), summary(on["verify_ms"])
            table_bytes = k * (1 << log_m) * 4
            row = {"instance": name, "log_m": log_m, "subtables": k, "entries": k << log_m, "table_bytes": table_bytes, "host_loop": so, "device_call": sn,
                   "device_call_own_ms": on["device_call_ms"], "table_bytes_per_s": table_bytes / (on["device_call_ms"] * 1e-3) if on["device_call_ms"] else None,
                   "speedup": so["median_ms"] / sn["median_ms"], "device_max_below_host_min": sn["max_ms"] < so["min_ms"]}
            row["share_of_hbm_peak_8TBps"] = row["table_bytes_per_s"] / HBM_PEAK_BYTES_PER_S if row["table_bytes_per_s"] else None
            rows.append(row)
            print(f"{name}: host loop {so['median_ms']:.2f} ms [{so['min_ms']:.2f}, {so['max_ms']:.2f}]   device {sn['median_ms']:.2f} ms [{sn['min_ms']:.2f}, {sn['max_ms']:.2f}]   "
                  f"call {row['device_call_own_ms']:.3f} ms = {100 * (row['share_of_hbm_peak_8TBps'] or 0):.2f} % of HBM peak   x{row['speedup']:.2f}", flush=True)
            write_mle(a, runs, rows)      # after every instance: a run that is cut short keeps what it measured
    print("wrote", a.out)


def run_child(curve, log_s, runs, env_extra):
    env = dict(os.environ)
    env.pop("LASSO_VERIFY_DEVICE_POINTS", None); env.pop("LASSO_VERIFY_MSM_POINTS", None); env.pop("LASSO_TRACE", None)
    env.pop("LASSO_VERIFY_DEVICE_MLE", None); env.pop("LASSO_MLE_DEVICE_MIN", None); env.pop("LASSO_MLE_STRIP", None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", curve, str(log_s), "--runs", str(runs)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    if res.returncode != 0:
        raise SystemExit(f"child failed ({curve}, 2^{log_s}, {env_extra}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    line = [ln for ln in res.stdout.split("\n") if ln.startswith("VERIFY_BENCH ")][-1]
    out = json.loads(line[len("VERIFY_BENCH "):])
    # LASSO_TRACE=2: the host time buckets ("[host] <name> <ms> ms" on stderr, dumped after every verify) of the timed runs, mean per verify
    err = res.stderr
    if "VERIFY_BENCH_TIMED_BEGIN" in err:
        timed = err.split("VERIFY_BENCH_TIMED_BEGIN", 1)[1].split("VERIFY_BENCH_TIMED_END", 1)[0]
        buckets = {}
        for ln in timed.split("\n"):
            if ln.startswith("[host] ") and ln.endswith(" ms"):
                name, val = ln[len("[host] "):-len(" ms")].rsplit(None, 1)
                buckets[name.strip()] = buckets.get(name.strip(), 0.0) + float(val)
        out["host_buckets_ms_per_verify"] = {k: v / runs for k, v in sorted(buckets.items())}
    return out


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "spread_ms": max(ms) - min(ms), "all_ms": ms}


PHASES = ["verify: msm_points create", "verify: msm_points msm", "verify: msm_points destroy", "verify: msm_points (table-free)", "verify: G_hat msm"]


def main_msm_points(a, runs):
    rows = []
    for curve, log_s in INSTANCES:
        name = f"{curve}-2p{log_s}"
        if a.only and name not in a.only.split(","):
            continue
        off = run_child(curve, log_s, runs, {"LASSO_VERIFY_MSM_POINTS": "0", "LASSO_TRACE": "2"})
        on = run_child(curve, log_s, runs, {"LASSO_VERIFY_MSM_POINTS": "1", "LASSO_TRACE": "2"})
        assert off["msm_points_calls_per_verify"] == 0 and on["msm_points_calls_per_verify"] > 0
        so, sn = summary(off["verify_ms"]), summary(on["verify_ms"])
        row = {"instance": name, "strategy": "and", "C": 1, "log_m": 16, "commitment_rows": (on["commitment_bytes"] - 16) // 32, "msm_points_calls_per_verify": on["msm_points_calls_per_verify"],
               "table_path": so, "table_free": sn,
               "table_path_phases_ms_per_verify": {k: off.get("host_buckets_ms_per_verify", {}).get(k) for k in PHASES if k != "verify: msm_points (table-free)"},
               "table_free_phases_ms_per_verify": {k: on.get("host_buckets_ms_per_verify", {}).get(k) for k in PHASES[3:]},
               "table_path_peak_device_bytes": off["peak_bytes_during_verifies"], "table_free_peak_device_bytes": on["peak_bytes_during_verifies"],
               "peak_device_bytes_saved": off["peak_bytes_during_verifies"] - on["peak_bytes_during_verifies"],
               "speedup": so["median_ms"] / sn["median_ms"],
               "no_slower_than_table_path_within_its_spread": sn["median_ms"] <= so["median_ms"] + so["spread_ms"]}
        rows.append(row)
        print(f"{name}: table path {so['median_ms']:.2f} ms [{so['min_ms']:.2f}, {so['max_ms']:.2f}] peak {row['table_path_peak_device_bytes'] / 1e6:.1f} MB   table-free {sn['median_ms']:.2f} ms "
              f"[{sn['min_ms']:.2f}, {sn['max_ms']:.2f}] peak {row['table_free_peak_device_bytes'] / 1e6:.1f} MB   x{row['speedup']:.2f}", flush=True)
        print("   phases (ms per verify): table path", row["table_path_phases_ms_per_verify"], " table-free", row["table_free_phases_ms_per_verify"], flush=True)
    out = {"what": "HostProver.verify, the MSMs over commitment rows through lasso_bases_create + lasso_msm + lasso_bases_destroy per call (LASSO_VERIFY_MSM_POINTS=0: the only "
                   "path of the parent commit, here with host timers around its phases) against table-free (the default, lasso_msm_points); same session, same machine, a fresh "
                   "process per setting, LASSO_TRACE=2 for the phase timers in both", "runs_per_setting": runs, "rows": rows,
           "table_free_ahead_at_every_instance": all(r["table_free"]["median_ms"] < r["table_path"]["median_ms"] for r in rows)}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", nargs=2, metavar=("CURVE", "LOG_S"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--ab", choices=["device_points", "msm_points", "mle"], default="device_points", help="which switch is compared (see above)")
    ap.add_argument("--out", default=None, help="default: profiles/verify_device_points.json, profiles/verify_msm_points.json with --ab msm_points, profiles/verify_device_mle.json with --ab mle")
    ap.add_argument("--only", default="", help="comma-separated subset, e.g. curve25519-2p10,bn254-2p20")
    a = ap.parse_args()
    if a.child and a.child[0] == "mle":
        return child_mle(*map(int, a.child[1].split(":")), a.runs)
    if a.child:
        return child(a.child[0], int(a.child[1]), a.runs)
    runs = max(a.runs, 5)
    if a.out is None:
        a.out = os.path.join(ROOT, "profiles", "verify_msm_points.json" if a.ab == "msm_points" else "verify_device_points.json")
    if a.ab == "mle":
        if a.out is None or a.out.endswith("verify_device_points.json"):
            a.out = os.path.join(ROOT, "profiles", "verify_device_mle.json")
        return main_mle(a, max(a.runs, 7))
    if a.ab == "msm_points":
        return main_msm_points(a, max(a.runs, 7))
    rows = []
    for curve, log_s in INSTANCES:
        name = f"{curve}-2p{log_s}"
        if a.only and name not in a.only.split(","):
            continue
        off = run_child(curve, log_s, runs, {"LASSO_VERIFY_DEVICE_POINTS": "0"})
        on = run_child(curve, log_s, runs, {"LASSO_WIRE_DEVICE_MIN": os.environ.get("LASSO_WIRE_DEVICE_MIN", "1")})      # threshold out of the way: the decoder itself is measured at every size
        so, sn = summary(off["verify_ms"]), summary(on["verify_ms"])
        row = {"instance": name, "strategy": "and", "C": 1, "log_m": 16, "wire_points": on["device_points_per_verify"], "host_points": so, "device_points": sn,
               "kernel_ms": on["kernel_ms"], "speedup": so["median_ms"] / sn["median_ms"],
               "no_slower_than_host_path_within_its_spread": sn["median_ms"] <= so["median_ms"] + so["spread_ms"]}
        assert off["device_points_per_verify"] == 0 and on["device_points_per_verify"] > 0
        rows.append(row)
        print(f"{name}: {row['wire_points']} points  host {so['median_ms']:.2f} ms [{so['min_ms']:.2f}, {so['max_ms']:.2f}]  device {sn['median_ms']:.2f} ms "
              f"[{sn['min_ms']:.2f}, {sn['max_ms']:.2f}]  kernel {row['kernel_ms']:.3f} ms  x{row['speedup']:.2f}", flush=True)
    wins = [r["wire_points"] for r in rows if r["device_points"]["median_ms"] < r["host_points"]["median_ms"]]
    out = {"what": "HostProver.verify, compressed points decoded on the host (LASSO_VERIFY_DEVICE_POINTS=0) against on the device (LASSO_WIRE_DEVICE_MIN=1)", "runs_per_setting": runs,
           "rows": rows, "smallest_measured_batch_where_the_device_wins": min(wins) if wins else None}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
