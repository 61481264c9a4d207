#!/usr/bin/env python3
"""Time lasso_host_gens_new (the label-derived generators of SparsePolyCommitmentGens::new) with every point built on the host (LASSO_GENS_DEVICE=0: one CPU thread,
the only path before lasso_points_from_candidates existed) and with the candidates' arithmetic on the device (the default route, threshold out of the way:
LASSO_GENS_DEVICE_MIN=1), on both curves, at the set sizes

    66 points        AND C = 1, M = 2^8 at 2^10 lookups
    8194 points      AND C = 1 at 2^24 lookups (the headline instance)
    2^15 + 2 points  RangeCheck C = 4 at 2^26 lookups (configs[3])
    2^16 + 2 points  Spark C = 16 at 2^26 lookups

The switches are read once per process, so every (curve, size, setting) is measured in a fresh child process: `--runs` calls of lasso_host_gens_new (host clock around
the call, the object freed after each; the call includes the upload of the points and the window tables, the same work in both settings), then — on the device route —
one more call with the library's event brackets on (lasso_prof_*, family LASSO_K_MISC) for the kernel's own time, and the candidates handed over per call
(lasso_host_gens_stats).

Writes one JSON file (default profiles/gens_device.json) with, per row, median / min / max of both settings and whether the device route's [min, max] range lies wholly
below the host route's, and the smallest measured size at which that holds on both curves: the value LASSO_GENS_DEVICE_MIN defaults to.  Needs the built libraries and
a GPU; nothing here falls back to a CPU."""
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

# (name, points of the widest set, (c, s, memories, log_m))
SIZES = [("and-c1-2p10", 66, (1, 1 << 10, 1, 8)), ("and-c1-2p24", 8194, (1, 1 << 24, 1, 16)), ("range-c4-2p26", (1 << 15) + 2, (4, 1 << 26, 4, 16)),
         ("spark-c16-2p26", (1 << 16) + 2, (16, 1 << 26, 16, 8))]
CURVES = ["curve25519", "bn254"]


def child(curve, name, runs):
    from lasso_amd import HostProver, _abi
    from lasso_amd.device import load_device_library
    _, points, shape = next(s for s in SIZES if s[0] == name)
    hp = HostProver(curve=curve)
    lib = load_device_library(curve=curve)      # the same shared object the host library is linked against
    ctx = C.c_void_p(hp.ctx())
    ms = []
    for _ in range(runs):
        lib.lasso_sync(ctx)
        t0 = time.perf_counter()
        gens = hp.gens(*shape)
        lib.lasso_sync(ctx)
        ms.append((time.perf_counter() - t0) * 1e3)
        assert max(hp.gens_points(gens, w).shape[0] for w in range(3)) == points
        hp.free(None, gens)
    candidates = hp.gens_stats()["device_candidates"] // runs
    kernel_ms = None
    if candidates:
        lib.lasso_prof_reset(ctx); lib.lasso_prof_enable(ctx, 1 << _abi.K_MISC)
        gens = hp.gens(*shape)
        n, t, b = C.c_uint64(), C.c_double(), C.c_double()
        lib.lasso_prof_get(ctx, _abi.K_MISC, C.byref(n), C.byref(t), C.byref(b))
        lib.lasso_prof_enable(ctx, 0)
        kernel_ms = t.value
        hp.free(None, gens)
    hp.close()
    print("GENS_BENCH " + json.dumps({"curve": curve, "size": name, "points": points, "gens_new_ms": ms, "candidates_per_call": candidates, "kernel_ms": kernel_ms}))


def run_child(curve, name, runs, env_extra):
    env = dict(os.environ)
    for k in ("LASSO_GENS_DEVICE", "LASSO_GENS_DEVICE_MIN", "LASSO_GENS_DEVICE_BATCH"):
        env.pop(k, None)
    env.update(env_extra)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", curve, name, "--runs", str(runs)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    if res.returncode != 0:
        raise SystemExit(f"child failed ({curve}, {name}, {env_extra}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    line = [ln for ln in res.stdout.split("\n") if ln.startswith("GENS_BENCH ")][-1]
    return json.loads(line[len("GENS_BENCH "):])


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", nargs=2, metavar=("CURVE", "SIZE"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "gens_device.json"))
    ap.add_argument("--only", default="", help="comma-separated subset, e.g. curve25519/and-c1-2p24,bn254/and-c1-2p10")
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs)
    rows = []
    for curve in CURVES:
        for name, points, shape in SIZES:
            if a.only and f"{curve}/{name}" not in a.only.split(","):
                continue
            off = run_child(curve, name, a.runs, {"LASSO_GENS_DEVICE": "0"})
            on = run_child(curve, name, a.runs, {"LASSO_GENS_DEVICE_MIN": "1"})      # threshold out of the way: the route itself is measured at every size
            assert off["candidates_per_call"] == 0 and on["candidates_per_call"] >= 2 * points
            so, sn = summary(off["gens_new_ms"]), summary(on["gens_new_ms"])
            row = {"curve": curve, "instance": name, "points": points, "shape_c_s_memories_log_m": list(shape), "host_route": so, "device_route": sn,
                   "candidates_per_call": on["candidates_per_call"], "kernel_ms": on["kernel_ms"], "speedup": so["median_ms"] / sn["median_ms"],
                   "device_range_wholly_below_host_range": sn["max_ms"] < so["min_ms"]}
            rows.append(row)
            print(f"{curve} {name}: {points} points  host {so['median_ms']:.2f} ms [{so['min_ms']:.2f}, {so['max_ms']:.2f}]  device {sn['median_ms']:.2f} ms "
                  f"[{sn['min_ms']:.2f}, {sn['max_ms']:.2f}]  {row['candidates_per_call']} candidates, kernel {row['kernel_ms']:.3f} ms  x{row['speedup']:.2f}", flush=True)
    # the smallest measured size at which the device route's range lies below the host route's on every curve measured
    ahead = sorted(p for p in {r["points"] for r in rows} if all(r["device_range_wholly_below_host_range"] for r in rows if r["points"] == p))
    ahead_from = ahead[0] if ahead else None
    out = {"what": "lasso_host_gens_new, every generator built on the host (LASSO_GENS_DEVICE=0) against the candidates' arithmetic on the device (LASSO_GENS_DEVICE_MIN=1); a fresh "
                   "process per setting, wall time of each of the calls (first call of the process included)", "runs_per_setting": a.runs, "rows": rows,
           "smallest_measured_size_at_which_the_device_range_is_below_the_host_range": ahead_from,
           "sizes_at_which_it_is_not": sorted({r["points"] for r in rows} - set(ahead))}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
