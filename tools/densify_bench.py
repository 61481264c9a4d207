#!/usr/bin/env python3
"""Time densify from lookup indices against densify from operand columns (include/lasso_hip_operands.h, lasso_host_densify_operands).

Three settings per shape, each in a fresh child process (the pools, the context's scratch buffer and the switches start the same way every time):
  indices          HostProver.densify(indices)                      the baseline: the index path of the same build, 8 C bytes per lookup uploaded
  operands_host    HostProver.densify_operands(x, y) on numpy       16 (two operands) or 8 (one) bytes per lookup uploaded, the indices formed on the device
  operands_device  lasso_host_densify_operands(where = 1)           columns already on the device (what HostProver.densify_operands does with GPU tensors): nothing is uploaded
Shapes: AND C = 1 2^24; XOR C = 8 2^24; RangeCheck<64> C = 4 2^26 (one operand), all at log_m = 16.  What the bytes predict: the upload falls by 8 C / 16 for two
operands and 8 C / 8 for one; at C = 1 with two operands it DOUBLES; the sort's own time does not change.

A child warms up once, then runs `--runs` calls (median / min / max of the wall time of the call, host clock), and one more call under the library's event brackets for the
LASSO_K_MISC kernel time (lasso_prof_*) with lasso_host_mem_stats reset in front of it for the peak device bytes.  Writes profiles/densify_operands.json.  Needs the
built libraries and a GPU; nothing here falls back to a CPU.  No test runs this tool."""
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

# name -> (kind, C, log_m, log_r, log2 lookups)
SHAPES = {"and": ("and", 1, 16, 0, 24), "xor": ("xor", 8, 16, 0, 24), "range": ("range", 4, 16, 64, 26)}
SETTINGS = ["indices", "operands_host", "operands_device"]


def child(shape, setting, runs, log_s):
    import numpy as np
    from lasso_amd import HostProver, _abi
    from lasso_amd.device import load_device_library
    kind, c, log_m, log_r, default_log_s = SHAPES[shape]
    n = 1 << (log_s or default_log_s)
    hp = HostProver()
    lay = hp.operand_layout(_abi.Strategy(_abi.KINDS[kind], c, log_m, log_r))
    rng = np.random.default_rng(1)
    bits = min(64, c * lay.chunk_bits)
    col = lambda: np.ascontiguousarray((rng.integers(0, 1 << 63, size=n, dtype=np.uint64) * np.uint64(2) + rng.integers(0, 2, size=n, dtype=np.uint64)) >> np.uint64(64 - bits))
    x = col(); y = col() if lay.operands == 2 else None
    if setting == "indices":
        idx = hp.operand_indices(x, y, layout=lay, c=c, log_m=log_m)
        call = lambda: hp.densify(idx, log_m)
        uploaded = idx.nbytes
    elif setting == "operands_host":
        call = lambda: hp.densify_operands(x, y, layout=lay, c=c, log_m=log_m)
        uploaded = x.nbytes * lay.operands
    else:
        # the columns put on the device through the host's own context (lasso_alloc + lasso_upload): what a caller whose witness generator runs on the GPU holds
        dlib = load_device_library(); dctx = C.c_void_p(hp.ctx())
        ptrs = []
        for a in (x, y):
            p = C.c_void_p()
            if a is not None:
                assert dlib.lasso_alloc(dctx, a.nbytes, C.byref(p)) == 0 and dlib.lasso_upload(dctx, p, a.ctypes.data_as(C.c_void_p), a.nbytes) == 0
            ptrs.append(p if a is not None else None)

        def call():
            d = C.c_void_p()
            hp._chk(hp.lib.lasso_host_densify_operands(hp.h, C.byref(lay), ptrs[0], ptrs[1], n, c, log_m, 1, C.byref(d)))
            return d
        uploaded = 0
    hp.free(call())                                   # warm-up: the context's scratch buffer, the pool
    ms = []
    for _ in range(runs):
        t0 = time.perf_counter()
        d = call()
        ms.append((time.perf_counter() - t0) * 1e3)
        hp.free(d)
    lib = load_device_library()                       # the same shared object the host library is linked against
    ctx = C.c_void_p(hp.ctx())
    hp.densify_stats(reset=True); hp.mem_stats(reset=True)
    lib.lasso_prof_reset(ctx); lib.lasso_prof_enable(ctx, 1 << _abi.K_MISC)
    d = call()
    mem = hp.mem_stats(); stats = hp.densify_stats()
    launches, t, b = C.c_uint64(), C.c_double(), C.c_double()
    lib.lasso_prof_get(ctx, _abi.K_MISC, C.byref(launches), C.byref(t), C.byref(b))
    lib.lasso_prof_enable(ctx, 0)
    hp.free(d); hp.close()
    print("DENSIFY_BENCH " + json.dumps({"shape": shape, "setting": setting, "lookups": n, "C": c, "log_m": log_m, "operands": lay.operands, "densify_ms": ms, "uploaded_bytes": uploaded,
                                         "k_misc_ms": t.value, "k_misc_brackets": launches.value, "peak_device_bytes": mem["peak_bytes"], "prover_peak_bytes": mem["prover_peak_bytes"],
                                         "operand_dims_on_device": stats["operand_dims_on_device"]}))


def run_child(shape, setting, runs, log_s):
    env = dict(os.environ); env.pop("LASSO_DENSIFY_OPERANDS", None)
    res = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", shape, setting, "--runs", str(runs), "--log-s", str(log_s)], env=env, cwd=ROOT, capture_output=True, text=True, timeout=1500)
    if res.returncode != 0:
        raise SystemExit(f"child failed ({shape}, {setting}):\n{res.stdout[-2000:]}\n{res.stderr[-4000:]}")
    line = [ln for ln in res.stdout.split("\n") if ln.startswith("DENSIFY_BENCH ")][-1]
    return json.loads(line[len("DENSIFY_BENCH "):])


def summary(ms):
    return {"median_ms": statistics.median(ms), "min_ms": min(ms), "max_ms": max(ms), "all_ms": ms}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--child", nargs=2, metavar=("SHAPE", "SETTING"))
    ap.add_argument("--runs", type=int, default=7)
    ap.add_argument("--log-s", type=int, default=0, help="log2 of the lookups of every shape (0: each shape's own size)")
    ap.add_argument("--shapes", default="and,xor,range")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "densify_operands.json"))
    a = ap.parse_args()
    if a.child:
        return child(a.child[0], a.child[1], a.runs, a.log_s)
    runs = max(a.runs, 7)
    rows = []
    for shape in a.shapes.split(","):
        got = {st: run_child(shape, st, runs, a.log_s) for st in SETTINGS}
        assert got["indices"]["operand_dims_on_device"] == 0 and all(got[st]["operand_dims_on_device"] == got[st]["C"] for st in SETTINGS[1:])
        row = {"shape": shape, "strategy": SHAPES[shape][0], "C": got["indices"]["C"], "log_m": got["indices"]["log_m"], "lookups": got["indices"]["lookups"], "operands": got["indices"]["operands"]}
        for st in SETTINGS:
            row[st] = dict(summary(got[st]["densify_ms"]), uploaded_bytes=got[st]["uploaded_bytes"], k_misc_ms=got[st]["k_misc_ms"], peak_device_bytes=got[st]["peak_device_bytes"],
                           prover_peak_bytes=got[st]["prover_peak_bytes"])
        for st in SETTINGS[1:]:
            row[st]["speedup_over_indices"] = row["indices"]["median_ms"] / row[st]["median_ms"]
        rows.append(row)
        print(f"{shape} C={row['C']} 2^{row['lookups'].bit_length() - 1}: " + "   ".join(
            f"{st} {row[st]['median_ms']:.2f} ms [{row[st]['min_ms']:.2f}, {row[st]['max_ms']:.2f}] kernels {row[st]['k_misc_ms']:.2f} ms peak {row[st]['peak_device_bytes'] / 2**20:.0f} MiB" for st in SETTINGS), flush=True)
    out = {"what": "HostProver.densify(indices) (the index path of the same build: the parent commit's behaviour) against HostProver.densify_operands with host columns and with "
                   "device-resident columns; one session, a fresh process per setting and shape; wall time of the call, LASSO_K_MISC kernel time of one more call, peak device bytes of that call",
           "runs_per_setting": runs, "rows": rows}
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
    print("wrote", a.out)


if __name__ == "__main__":
    main()
