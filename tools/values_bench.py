#!/usr/bin/env python3
"""Time lasso_lookup_values (include/lasso_hip_values.h): the launch alone, from the library's own event brackets (lasso_prof_*, family LASSO_K_MISC), in a fresh child
process per (shape, form), the median of `--runs` launches (default 7) with [min, max], after one untimed launch.

Shapes: AND C = 1, M = 2^16 at 2^24 lookups (the headline shape); XOR C = 8 at 2^24; LT C = 16 at 2^22; Spark C = 4 at 2^20 (M = 2^16 throughout); the field form everywhere
and the 64-bit form where it is offered.  Addresses are random, one draw per lookup and dimension.

Beside each time: the ALGORITHMIC bytes — 4 * C read plus 8 or 32 written per lookup; the subtables are NOT counted (the kernel gathers them through L2: at most 3 x 256 KiB
of integers, 4 x 2 MiB of field elements for Spark) — and their rate as a share of the MI355X's 8 TB/s HBM peak.

Reference point, not a pass / fail line: what the parent commit offers for the same vector before any combine — NUM_MEMORIES lasso_gather launches into 32-byte arrays
(`gather`), timed the same way (all launches of one pass bracketed, their times added).  Its bytes are lasso_gather's own model, 68 per lookup and memory.

Writes one JSON file (default profiles/lookup_values.json).  Needs the built libraries and a GPU; nothing here falls back to a CPU."""
import argparse
import json
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = [("and", 1, 16, 24), ("xor", 8, 16, 24), ("lt", 16, 16, 22), ("spark", 4, 16, 20)]
PEAK = 8e12


def child(curve, kind, c, log_m, log_n, what, runs):
    import ctypes as C
    import numpy as np
    from lasso_amd import Device, _abi
    from lasso_amd.custom import strategy_ptr
    dev = Device(0, curve=curve)
    n, m = 1 << log_n, 1 << log_m
    st = _abi.Strategy(_abi.KINDS[kind], c, log_m, 0)
    rng = np.random.default_rng(1)
    d_dim = [dev.upload(rng.integers(0, m, size=n, dtype=np.uint32)) for _ in range(c)]
    field = kind == "spark"
    nsub = {"lt": 2, "spark": c}.get(kind, 1)
    alpha = 2 * c if kind == "lt" else c
    tabs = []
    for k in range(nsub):
        p = dev.alloc((32 if field else 4) * m)
        if field:
            dev.eq_evals(rng.integers(0, 2**60, size=(log_m, 4), dtype=np.uint64), p)
        else:
            dev._chk(dev.lib.lasso_materialize_subtable_u32(dev.ctx, strategy_ptr(st), k, C.c_void_p(p)))
        tabs.append(p)
    dev.prof_enable(1 << _abi.K_MISC)
    times = []
    if what == "gather":
        fr_tabs = tabs
        if not field:
            fr_tabs = []
            for p in tabs:
                q = dev.alloc(32 * m); dev.fr_from_u32(p, m, q); fr_tabs.append(q)
        d_out = dev.alloc(32 * n)          # one array takes every launch's output: the traffic is the same, the 32 * n * alpha bytes of E are not needed to time it
        maps = [(i % nsub, i if kind == "spark" else i // nsub) for i in range(alpha)]
        for it in range(runs + 1):
            dev.sync(); dev.prof_reset()
            for sub, dim in maps:
                dev.gather(fr_tabs[sub], d_dim[dim], n, d_out)
            dev.sync()
            launches, ms, _ = dev.prof_get(_abi.K_MISC)
            assert launches == alpha
            if it:
                times.append(ms)
        alg = 68.0 * n * alpha
    else:
        form = _abi.VALUES_U64 if what == "u64" else _abi.VALUES_FR
        elem = 8 if what == "u64" else 32
        d_out = dev.alloc(elem * n)
        for it in range(runs + 1):
            dev.sync(); dev.prof_reset()
            dev.lookup_values(strategy_ptr(st), d_dim, tabs, field, n, form, d_out)
            dev.sync()
            launches, ms, alg = dev.prof_get(_abi.K_MISC)
            assert launches == 1 and alg == (4.0 * c + elem) * n
            if it:
                times.append(ms)
    print(json.dumps({"ms": times, "alg_bytes": alg}))
    dev.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--child", nargs=7)
    ap.add_argument("--curve", default="curve25519")
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--only", default="")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lookup_values.json"))
    a = ap.parse_args()
    if a.child:
        curve, kind, c, log_m, log_n, what, runs = a.child
        return child(curve, kind, int(c), int(log_m), int(log_n), what, int(runs))
    rows = []
    for kind, c, log_m, log_n in SHAPES:
        name = f"{kind}_c{c}_m{log_m}_2p{log_n}"
        if a.only and a.only not in name:
            continue
        for what in ["field"] + (["u64"] if kind != "spark" else []) + ["gather"]:
            res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", a.curve, kind, str(c), str(log_m), str(log_n), what, str(a.runs)],
                                 capture_output=True, text=True, timeout=600)
            if res.returncode != 0:
                sys.stderr.write(res.stderr[-3000:])
                raise SystemExit(f"{name} {what}: the child ended with status {res.returncode}; nothing further is started")
            r = json.loads(res.stdout.strip().split("\n")[-1])
            med = statistics.median(r["ms"])
            row = {"shape": name, "curve": a.curve, "what": what, "lookups": 1 << log_n, "c": c, "runs": len(r["ms"]), "ms_median": med, "ms_min": min(r["ms"]), "ms_max": max(r["ms"]),
                   "alg_bytes": r["alg_bytes"], "alg_bytes_note": "addresses read + values written; subtables excluded (L2 gathers)" if what != "gather" else "lasso_gather's model: 68 bytes per lookup and memory",
                   "tb_per_s": r["alg_bytes"] / (med * 1e-3) / 1e12, "share_of_8tbs_peak": r["alg_bytes"] / (med * 1e-3) / PEAK}
            rows.append(row)
            print(json.dumps(row), flush=True)
    with open(a.out, "w") as f:
        json.dump({"tool": "tools/values_bench.py", "timer": "lasso_prof_* event brackets around the launch, fresh process per row", "rows": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
