#!/usr/bin/env python3
"""bench.py — prover lookups/s for SparsePolynomialEvaluationProof on MI355X (BASELINE.json metric).

A "step" = one SparsePolynomialEvaluationProof::prove over one batch of s synthetic lookups whose densified representation
is already resident in HBM (the reference's `SparsePoly.prove` span; generator construction, densify, commit and verify are
outside the timed region exactly as in the reference's published logs).  Default workload = the configuration the metric
is quoted on: AND table, C=1, M=2^16, s=2^24 (src/benches/bench.rs `halo2_comparison_benchmarks`, src/benches/*.log).

N > 1 (torch.distributed / RCCL, one process per GPU): each rank proves an independent batch of s lookups — the path
partitions by proof, there is no data-path collective — so value = N*s*K / max-over-ranks time and scaling is "weak".

One JSON line on rank 0.  A plain run sets up, warms up, times --steps proofs and prints the line (headline, `ms_per_step`, setup spans, library digests,
multi_gpu); --dump-outputs DIR also writes the last timed proof as DIR/proof.npy (one float32 per byte).  Everything below is measured only with --full.
Extra objects (--full): roofline (dominant HBM-streaming kernel family, HIP events on the library's stream; `frac` = algorithmic
bytes / time / peak and `frac_traffic` = counter-measured HBM bytes / time / peak), roofline_bind_top (the kernel the north star names),
roofline_msm (the MSM families: group additions of the reference's algorithm per second against the measured mixed-addition ceiling),
dominant_family (largest family by time over ALL families), kernels (every kernel family: launches, ms, algorithmic GB/s),
cpu_baseline (the oracle prover on ALL host cores at the same 2^24-lookup instance, one-thread figure beside it; rank 0, N=1) and
parity_checked (the GPU's commitment and proof compared byte for byte with the oracle's for that instance).
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

HBM_PEAK_GBS = 8000.0   # MI355X_MICROARCH.md: HBM3E 8.0 TB/s spec peak
# the only published number for this exact metric — 2^24 AND lookups, C=1, `SparsePoly.prove` span, rayon on an Apple M1 16 GB:
# 35.3 s (src/benches/m1_16gb_parallel_benches.log:439) = 2^24 / 35.3 lookups/s.  Other hardware: a reference point, not a like-for-like comparison.
PUBLISHED_LOOKUPS_PER_S = (1 << 24) / 35.3


def parse():
    p = argparse.ArgumentParser()
    p.add_argument("--gpus", type=int, default=1)
    p.add_argument("--steps", type=int, default=3)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--log-s", type=int, default=24, help="log2 of lookups per proof (default 24 = the headline metric)")
    p.add_argument("--c", type=int, default=1)
    p.add_argument("--kind", default="and", choices=["and", "or", "xor", "lt", "range", "spark"], help="\"spark\" = LASSO_SPARK_UNCONFIRMED: BASELINE.json configs[4]'s strategy as SURVEY 8(f3) describes it (not in the reference snapshot)")
    p.add_argument("--log-m", type=int, default=16)
    p.add_argument("--log-r", type=int, default=40)
    p.add_argument("--cpu-log-s", type=int, default=24, help="log2 lookups of the CPU-baseline instance, proved by the oracle on all host cores (2^24 = the metric's own size)")
    p.add_argument("--cpu-1t-log-s", type=int, default=20, help="log2 lookups of the bounded ONE-thread sample reported beside the all-core figure")
    p.add_argument("--curve", default="curve25519", choices=["curve25519", "bn254"], help="the group G: curve25519 (the reference harness's, the headline metric) or BN254 G1 "
                                                                                          "(BASELINE.json configs[1]; the liblasso_*_bn254.so pair)")
    p.add_argument("--no-cpu-baseline", action="store_true")
    p.add_argument("--no-prof", action="store_true")
    p.add_argument("--concurrent", type=int, default=16, help="extra leg at N=1: this many independent proofs proved concurrently on the one GPU (own context, stream and host "
                                                              "thread each), swept over 2, 4, 8, ... up to this many; reported beside the headline, never as `value`.  0 = skip")
    p.add_argument("--backend", default=None, choices=["nccl", "gloo"], help="torch.distributed backend for N > 1 (default: nccl = RCCL when a GPU is visible).  gloo lets the N > 1 "
                                                                              "code path be exercised on a box with fewer GPUs than ranks (ranks share devices)")
    p.add_argument("--shard-proof", action="store_true", help="N > 1: ONE proof of s lookups sharded over the N GPUs by low index bits (slab mode, strong scaling) "
                                                                "instead of one independent proof per GPU (the default, weak scaling)")
    p.add_argument("--slab-kind", default="range", choices=["and", "or", "xor", "lt", "range", "spark"], help="the extra slab-mode leg's workload: by default BASELINE.json configs[3], "
                                                                                                       "RangeCheck C=4 2^26 (the configuration the north star shards over several GPUs)")
    p.add_argument("--slab-c", type=int, default=4)
    p.add_argument("--slab-log-s", type=int, default=26)
    p.add_argument("--slab-steps", type=int, default=2)
    p.add_argument("--no-slab-leg", action="store_true", help="skip the extra slab-mode leg (ONE proof over all N GPUs; at N = 1 its single-GPU reference time)")
    p.add_argument("--slab-timeout", type=float, default=240.0)
    p.add_argument("--slab-capacity", action="store_true", help="slab leg in capacity mode (lasso_host_set_capacity): per-rank high-water mark = the prover's live peak")
    p.add_argument("--no-bind-sweep", action="store_true", help="skip the kernel-level bind_top sweep (SURVEY 8(d): n in {2^24, 2^26, 2^28} x {1, 9} polynomials)")
    p.add_argument("--only-bind-sweep", action="store_true", help="run only the bind_top sweep and print its object (the command the rocprofv3 / PMC passes of profiles/r04_* wrap)")
    p.add_argument("--full", action="store_true", help="also measure everything beside the headline: per-kernel profile and rooflines, concurrent proofs, bind_top sweep, "
                                                        "CPU baseline with oracle parity, slab leg (the --no-* / --concurrent options select among them)")
    p.add_argument("--dump-outputs", default=None, metavar="DIR", help="write the proof of the last timed step as DIR/proof.npy (float32, one element per byte; rank 0)")
    p.add_argument("--slab-worker", default=None, help=argparse.SUPPRESS)   # internal: rank,world,device,shm_name — the slab leg's child process
    a = p.parse_args()
    if a.steps < 1:
        p.error("--steps must be at least 1")
    if not a.full:      # a plain run does only what the headline needs
        a.no_prof = a.no_cpu_baseline = a.no_bind_sweep = a.no_slab_leg = True
        a.concurrent = 0
    return a


def dump_outputs(d, proof):
    """--dump-outputs: what a caller of the timed path receives — the serialized proof — one float32 per byte (exact), as DIR/proof.npy"""
    os.makedirs(d, exist_ok=True)
    np.save(os.path.join(d, "proof.npy"), np.frombuffer(proof, dtype=np.uint8).astype(np.float32))


def _oracle_run(orc, kind_id, c, log_m, log_r, log_s, threads, want_bytes):
    orc.orc_set_threads(threads)
    td, tc, tp = C.c_double(), C.c_double(), C.c_double()
    cap = 1 << 23
    pb = (C.c_uint8 * cap)() if want_bytes else None; cb = (C.c_uint8 * cap)() if want_bytes else None; pl = C.c_size_t(); cl = C.c_size_t()
    rc = orc.orc_bench_bytes(kind_id, C.c_size_t(c), C.c_size_t(1 << log_m), C.c_size_t(log_r), C.c_size_t(1 << log_s), C.byref(td), C.byref(tc), C.byref(tp), 0,
                             pb, C.c_size_t(cap), C.byref(pl), cb, C.c_size_t(cap), C.byref(cl))
    if rc != 0:
        return None
    return {"densify_s": td.value, "commit_s": tc.value, "prove_s": tp.value, "proof": bytes(pb[: pl.value]) if want_bytes else None, "comm": bytes(cb[: cl.value]) if want_bytes else None}


def cpu_baseline(kind_id, c, log_m, log_r, log_s, log_s_1t, curve="curve25519"):
    """The oracle prover ("port": the C++ restatement of the reference, OpenMP over the sites the reference hands to rayon) on ALL of this box's host
    cores at 2^log_s lookups — the harness instance itself, so its commitment and proof bytes double as the parity check of the GPU's — plus a bounded
    one-thread sample.  Returns (json object, commitment bytes, proof bytes)."""
    import subprocess
    so = "liblasso_oracle_bn254.so" if curve == "bn254" else "liblasso_oracle.so"
    subprocess.check_call(["make", "-s", "-C", os.path.join(ROOT, "oracle"), so])
    orc = C.CDLL(os.path.join(ROOT, "oracle", so))
    orc.orc_set_threads(0)               # one thread per physical core (oracle_capi.cpp orc_set_threads)
    cores = orc.orc_max_threads()
    full = _oracle_run(orc, kind_id, c, log_m, log_r, log_s, cores, True)
    if not full:
        return None, None, None
    one = _oracle_run(orc, kind_id, c, log_m, log_r, min(log_s_1t, log_s), 1, False) if cores > 1 else None
    orc.orc_set_threads(cores)
    out = {"value": (1 << log_s) / full["prove_s"], "unit": "lookups/s", "cores": cores, "kind": "port", "host_physical_cores": orc.orc_physical_cores(), "host_logical_cpus": os.cpu_count(),
           "sample": f"oracle (C++ restatement of the reference prover, OpenMP = the reference's rayon sites) SparsePoly.prove, kind={kind_id} C={c} M=2^{log_m} s=2^{log_s} "
                     f"on {cores} threads: {full['prove_s']:.2f}s (densify {full['densify_s']:.2f}s, commit {full['commit_s']:.2f}s)"}
    if one:
        ls1 = min(log_s_1t, log_s)
        out["one_thread"] = {"value": (1 << ls1) / one["prove_s"], "unit": "lookups/s", "cores": 1,
                             "sample": f"the same prover on 1 thread at s=2^{ls1}: {one['prove_s']:.2f}s (commit {one['commit_s']:.2f}s)"}
    return out, full["comm"], full["proof"]


def device_library_path(curve):
    """liblasso_hip[_bn254].so; LASSO_DEVICE_LIB (with LASSO_PROVER_LIB, lasso_amd/prover.py) names another build of the same C ABI — the CPU test of the N > 1 plumbing"""
    return os.environ.get("LASSO_DEVICE_LIB") or os.path.join(ROOT, "lasso_amd", "liblasso_hip_bn254.so" if curve == "bn254" else "liblasso_hip.so")


def workload_key(kind, c, log_m, log_s, curve):
    """names the configuration a measurement belongs to: PMC traffic, digests and ceilings are only ever applied to the workload they were taken on"""
    return f"{kind}_c{c}_m{log_m}_2p{log_s}_{curve}"


def pmc_traffic(key):
    """HBM bytes per launch from the committed rocprofv3 PMC passes of this same command ON THIS WORKLOAD (profiles/r0N_pmc/<workload key>/bench_traffic.json, written by
    tools/pmc_summary.py: FETCH_SIZE x2 per MI355X_MICROARCH.md's gfx950 correction + WRITE_SIZE, large launches only).  {} when no pass of this workload is
    committed — `traffic` / `frac_traffic` are then null rather than borrowed from another configuration (VERDICT r2 "What's weak" 4)."""
    for d in ("r06_pmc", "r05_pmc", "r03_pmc", "r02_pmc", "r01_pmc"):     # newest committed passes first
        for sub in (key, ""):
            try:
                with open(os.path.join(ROOT, "profiles", d, sub, "bench_traffic.json")) as f:
                    t = json.load(f)
            except Exception:
                continue
            wk = t.pop("_workload", "and_c1_m16_2p24_curve25519")      # files of rounds 1-2 carry no key: they are passes of the default command
            if wk == key:
                t["_pass"] = {"dir": f"profiles/{d}/{sub}".rstrip("/"), "device_sources_sha256": t.pop("_device_sources_sha256", None)}
                return t
    return {}


def prover_library_path(curve):
    """the host library lasso_amd/prover.py loads (LASSO_PROVER_LIB overrides it, as there)"""
    return os.environ.get("LASSO_PROVER_LIB") or os.path.join(ROOT, "lasso_amd", "liblasso_prover_bn254.so" if curve == "bn254" else "liblasso_prover.so")


def host_info():
    """CPU model and what the prover's host share runs on: lasso_amd/host/field52.hpp (AVX-512 IFMA, eight field elements per register, take-over budget 128) where the CPU has
    it and LASSO_HOST_IFMA != 0, the scalar loop (budget 32) otherwise; LASSO_HOST_TAIL overrides the budget (lasso_amd/host/prover.hpp host_tail_budget)"""
    info = {"cpu_model": None, "avx512ifma": None}
    try:
        txt = open("/proc/cpuinfo").read()
        for line in txt.splitlines():
            if line.startswith("model name") and info["cpu_model"] is None:
                info["cpu_model"] = line.split(":", 1)[1].strip()
            if line.startswith("flags") and info["avx512ifma"] is None:
                fl = line.split(":", 1)[1].split(); info["avx512ifma"] = "avx512ifma" in fl and "avx512f" in fl
    except OSError:
        pass
    ifma = bool(info["avx512ifma"]) and os.environ.get("LASSO_HOST_IFMA", "1")[:1] != "0"
    info["host_rounds"] = "avx512-ifma (lasso_amd/host/field52.hpp)" if ifma else "scalar 4 x u64 (lasso_amd/host/field_host.hpp H4)"
    info["host_tail_budget"] = int(os.environ["LASSO_HOST_TAIL"]) if os.environ.get("LASSO_HOST_TAIL", "").lstrip("-").isdigit() else (128 if ifma else 32)
    return info


def lib_sha(curve):
    """sha256 over the sources the two libraries are built from, and whether the .so files THIS RUN LOADED are at least as new as every one of them: a stale prebuilt
    binary cannot be timed silently (VERDICT r2 "What's weak" 10).  The paths are the ones actually opened — LASSO_DEVICE_LIB / LASSO_PROVER_LIB included (a line
    produced under an override used to report the digests of libraries that were not the ones timed) — and `overridden` says when they are not the in-tree product pair."""
    import hashlib
    h = hashlib.sha256(); hd = hashlib.sha256()
    files = []
    for d in ("lasso_amd/csrc", "lasso_amd/host", "include"):
        for fn in sorted(os.listdir(os.path.join(ROOT, d))):
            if fn.endswith((".hip", ".cuh", ".hpp", ".cpp", ".h")):
                files.append(os.path.join(ROOT, d, fn))
    newest_dev = newest_host = 0.0
    for fpath in files:
        rel = os.path.relpath(fpath, ROOT)
        with open(fpath, "rb") as f:
            data = f.read()
        h.update(rel.encode()); h.update(data)
        device_side = rel.startswith("lasso_amd/csrc") or rel == "include/lasso_hip.h"     # what liblasso_hip.so is built from (lasso_amd/build.py build_device)
        if device_side:
            hd.update(rel.encode()); hd.update(data); newest_dev = max(newest_dev, os.path.getmtime(fpath))
        if not rel.endswith(".hip"):                                                        # the host library: host/*, the shared .cuh arithmetic, both headers (build_host)
            newest_host = max(newest_host, os.path.getmtime(fpath))
    dev, host = os.path.abspath(device_library_path(curve)), os.path.abspath(prover_library_path(curve))
    libs = [dev, host]
    # each library against ITS OWN sources (round 4 compared both with the newest file of either: a host-only edit made the untouched device library look stale)
    fresh = os.path.exists(dev) and os.path.getmtime(dev) >= newest_dev and os.path.exists(host) and os.path.getmtime(host) >= newest_host
    return {"sources_sha256": h.hexdigest(), "device_sources_sha256": hd.hexdigest(), "libraries_newer_than_sources": bool(fresh),
            "libraries_sha256": {os.path.basename(l): hashlib.sha256(open(l, "rb").read()).hexdigest()[:16] for l in libs if os.path.exists(l)},
            "libraries_loaded": [os.path.relpath(l, ROOT) for l in libs], "overridden": bool(os.environ.get("LASSO_DEVICE_LIB") or os.environ.get("LASSO_PROVER_LIB"))}


def golden_digest(kind, c, log_m, log_r, log_s):
    """the oracle's digests for a full-size harness instance (tests/golden/full_config_digests.json, recorded by tools/parity_full_configs.py), or None"""
    try:
        with open(os.path.join(ROOT, "tests", "golden", "full_config_digests.json")) as f:
            return json.load(f).get(f"{kind},{c},{log_m},{log_r},{log_s}", {}).get("oracle")
    except Exception:
        return None


def madd_ceiling(curve):
    """Ceiling of mixed point additions per second that NO schedule of the kernels' arithmetic can exceed: VALU instructions of one pt_madd read off the gfx950 ISA
    (tools/madd_isa_count.py, `hipcc -S`) against the chip's VALU issue peak, 256 CUs x 64 lane-instructions per clock x 2.4 GHz (profiles/r04_madd_ceiling.json states the
    derivation).  Rounds 2-3 normalised by a measured microbenchmark instead, which the product kernels then beat (frac 1.02-1.08, VERDICT r3 "weak" 4); that figure
    stays in the output as `microbenchmark` — since round 6 the rate of a SPILL-FREE chain of additions at three waves per SIMD (tools/madd_bench.hip), which no product kernel exceeds
    (`frac_microbench` <= 1 is asserted).  None when no derivation is committed for this curve build."""
    out = None
    try:
        with open(os.path.join(ROOT, "profiles", "r04_madd_ceiling.json")) as f:
            out = json.load(f).get(curve)
    except Exception:
        return None
    try:   # the measured ceiling: round 6's spill-free chain (tools/madd_bench.hip; profiles/r06_madd_ceiling.json says why round 2's 16.08 G/s was a spilling kernel's rate)
        with open(os.path.join(ROOT, "profiles", "r06_madd_ceiling.json")) as f:
            m = json.load(f).get(curve)
        if out and m:
            out = dict(out); out["microbenchmark_G_madd_per_s"] = m["G_madd_per_s"]; out["microbenchmark_source"] = m["source"]
    except Exception:
        pass
    return out


def concurrent_leg(HostProver, _abi, max_streams, steps, S, c, log_m, log_s, curve="curve25519", kernel_ms_per_proof=None):
    """Throughput mode: T independent proofs at a time on one GPU, T swept over {2, 4, 8, 16} (up to max_streams).  One proof is latency-bound by its ~470 sequential transcript
    rounds (the device idles most of the time at 2^24 lookups); independent proofs on their own contexts / streams (one PINNED host thread each) fill the gaps.  Every proof of
    every stream is compared with the bytes the same prover produced alone (sequentially) before the sweep.  Serving-style throughput, reported beside — never as — the
    one-proof-at-a-time metric, which is what the reference's harness measures."""
    import hashlib
    import threading
    s = 1 << log_s
    alpha = 2 * c if S.kind == _abi.KINDS["lt"] else c
    sweep = [t for t in (2, 4, 8, 16) if t <= max_streams] or [max_streams]
    try:
        cpus = sorted(os.sched_getaffinity(0))
    except Exception:
        cpus = []
    workers = []
    for t in range(max(sweep)):
        hp = HostProver(curve=curve)
        hp.set_throughput_mode(True)      # one of several hosts on this GPU: no kernel waits on the device for its host thread (include/lasso_prover.h)
        idx = (hp.gen_indices(s, 1 << log_m, c) + t) % (1 << log_m)
        r = hp.gen_random_point(log_s)
        gens = hp.gens(c, s, alpha, log_m); dense = hp.densify(idx, log_m); del idx
        want = hashlib.sha256(hp.prove(dense, gens, S, r)).digest()      # warm-up = the sequential reference bytes of this stream's instance
        workers.append((hp, dense, gens, r, want))
    results, errors = [], []

    def run_round(T):
        bar = threading.Barrier(T + 1)
        bad = [0] * T

        def run(t):
            hp, dense, gens, r, want = workers[t]
            try:
                if cpus:      # one core per stream, spread over the socket(s): the host side of a proof is a spin loop + Keccak, it must not migrate or share a core
                    os.sched_setaffinity(0, {cpus[(t * max(1, len(cpus) // T)) % len(cpus)]})
                bar.wait(timeout=120)
                for _ in range(steps):
                    if hashlib.sha256(hp.prove(dense, gens, S, r)).digest() != want:
                        bad[t] += 1
                bar.wait(timeout=120)
            except Exception as e:   # a failed proof must not leave the others (and the bench line) waiting at the barrier
                errors.append(repr(e)); bar.abort()
        ths = [threading.Thread(target=run, args=(t,)) for t in range(T)]
        for th in ths:
            th.start()
        el = None
        try:
            bar.wait(timeout=120); t0 = time.perf_counter(); bar.wait(timeout=120); el = time.perf_counter() - t0
        except threading.BrokenBarrierError:
            errors.append("barrier broken")
        for th in ths:
            th.join()
        return el, sum(bad)
    for T in sweep:
        el, nbad = run_round(T)
        if errors:
            break
        results.append({"streams": T, "proofs": T * steps, "value": T * steps * s / el, "ms_per_round_of_proofs": round(el / steps * 1e3, 3), "proofs_differing_from_sequential": nbad})
    for hp, dense, gens, r, _ in workers:
        hp.free(dense, gens); hp.close()
    if errors:
        return {"sweep": results, "error": "; ".join(errors)[:400]}
    best = max(results, key=lambda x: x["value"])
    out = {"streams": best["streams"], "proofs": best["proofs"], "value": best["value"], "unit": "lookups/s", "ms_per_round_of_proofs": best["ms_per_round_of_proofs"],
           "all_proofs_identical_to_sequential": all(x["proofs_differing_from_sequential"] == 0 for x in results), "sweep": results, "host_threads_pinned": bool(cpus),
           "note": "independent proofs proved concurrently on one GPU (one context, stream and pinned host thread each), every proof compared with its sequential bytes; not the headline metric"}
    if kernel_ms_per_proof:
        # what bounds it: a proof's kernels occupy the device for kernel_ms_per_proof when nothing else runs; proofs that only ever interleaved (no two kernels at once) could
        # not exceed s / that.  Above it, small kernels of different proofs are sharing the chip; far below it, the host side (spin + Keccak per stream) or the runtime's
        # launch path is the limit.
        bound = s / (kernel_ms_per_proof * 1e-3)
        out["device_serial_bound"] = {"kernel_ms_per_proof": round(kernel_ms_per_proof, 3), "lookups_per_s_if_kernels_never_overlap": bound, "achieved_over_bound": round(best["value"] / bound, 3)}
    return out


def bind_top_sweep(dev_lib, ctx, _abi, curve, iterations=20, warmup=3):
    """SURVEY 8(d)'s kernel-level sweep of `bound_poly_var_top` (src/poly/dense_mlpoly.rs:209-216), the kernel BASELINE.json's north star puts its one numeric 1-GPU target on:
    n in {2^24, 2^26, 2^28} x polys in {1, 9}, `iterations` timed launches after `warmup`, each on a buffer set the previous launch did not touch (two or more sets, rotated:
    nothing is served from the 256 MiB Infinity Cache), algorithmic bytes 48 * n * p (read 32 n, write 16 n per polynomial) / the HIP-event time of the launch on the library's
    stream.  Returns the `bind_top_sweep` object of the bench line."""
    rows = []
    vp = C.c_void_p

    def chk(rc, what):      # a device call that fails ends this row of the sweep, not the bench line
        if rc != 0:
            raise RuntimeError(f"{what} failed ({rc})")
    r = np.array([0x123456789abcdef1, 0x0fedcba987654321, 0x1111111122222222, 0x0123456701234567], dtype=np.uint64)   # any field element < p in ark-ff's in-memory form
    for log_n in (24, 26, 28):
        for polys in (1, 9):
            n = 1 << log_n
            set_bytes = polys * n * 32
            sets = max(2, min(4, int(150e9 // set_bytes)))
            if sets * set_bytes > 170e9:
                rows.append({"log_n": log_n, "polys": polys, "skipped": "does not fit beside the resident proof"}); continue
            bufs = []
            try:
                src = vp(); chk(dev_lib.lasso_alloc(ctx, n * 4, C.byref(src)), "lasso_alloc")
                # fill: seeded random 32-bit integers lifted to Fr — v * 2^256 mod p in memory, i.e. full-width field elements (8(d): "uniformly random canonical field elements")
                h_src = np.random.default_rng(1).integers(0, 1 << 32, size=n, dtype=np.uint32)
                chk(dev_lib.lasso_upload(ctx, src, h_src.ctypes.data_as(vp), n * 4), "lasso_upload")
                del h_src
                for _ in range(sets):
                    b = vp()
                    if dev_lib.lasso_alloc(ctx, set_bytes, C.byref(b)) != 0:
                        raise MemoryError("lasso_alloc")
                    bufs.append(b)
                    for k in range(polys):
                        chk(dev_lib.lasso_fr_from_u32(ctx, src, n, vp(b.value + k * n * 32)), "lasso_fr_from_u32")
                dev_lib.lasso_sync(ctx)
                tabs = []
                for b in bufs:
                    tabs.append((vp * polys)(*[vp(b.value + k * n * 32) for k in range(polys)]))
                for i in range(warmup):
                    chk(dev_lib.lasso_bind_top(ctx, tabs[i % sets], polys, n, r.ctypes.data_as(vp)), "lasso_bind_top")
                dev_lib.lasso_sync(ctx)
                dev_lib.lasso_prof_reset(ctx); dev_lib.lasso_prof_enable(ctx, 1 << _abi.K_BIND)
                for i in range(iterations):
                    chk(dev_lib.lasso_bind_top(ctx, tabs[(warmup + i) % sets], polys, n, r.ctypes.data_as(vp)), "lasso_bind_top")
                dev_lib.lasso_sync(ctx)
                cnt = C.c_uint64(); ms = C.c_double(); by = C.c_double()
                dev_lib.lasso_prof_get(ctx, _abi.K_BIND, C.byref(cnt), C.byref(ms), C.byref(by)); dev_lib.lasso_prof_enable(ctx, 0)
                alg = 48.0 * n * polys
                gbps = alg * cnt.value / (ms.value * 1e-3) / 1e9
                rows.append({"log_n": log_n, "polys": polys, "launches": cnt.value, "us_per_launch": round(ms.value * 1e3 / cnt.value, 2), "alg_bytes_per_launch": int(alg),
                             "alg_GBps": round(gbps, 1), "frac": round(gbps / HBM_PEAK_GBS, 4), "buffer_sets_rotated": sets})
            except (MemoryError, RuntimeError) as e:
                rows.append({"log_n": log_n, "polys": polys, "error": repr(e)})
            finally:
                dev_lib.lasso_sync(ctx)
                for b in bufs:
                    dev_lib.lasso_free(ctx, b)
                if src:
                    dev_lib.lasso_free(ctx, src)
    ok = [x for x in rows if "frac" in x]
    out = {"kernel": "k_bind_top (lasso_bind_top = DensePolynomial::bound_poly_var_top, src/poly/dense_mlpoly.rs:209-216)", "bound": "hbm", "peak": HBM_PEAK_GBS, "unit": "GB/s",
           "iterations": iterations, "warmup": warmup, "algorithmic_bytes": "48 * n * polys per launch (read 32 n + write 16 n per polynomial, SURVEY 8(d))",
           "timing": "HIP events on the library's stream around each launch (lasso_prof_*), buffer sets rotated so that no launch re-reads what the previous one touched",
           "rows": rows, "frac_min": min((x["frac"] for x in ok), default=None), "frac_max": max((x["frac"] for x in ok), default=None)}
    out["traffic"] = None
    for d in ("r06_pmc", "r05_pmc", "r04_pmc"):     # counter-measured HBM bytes of the same sweep (separate rocprofv3 --pmc FETCH_SIZE / WRITE_SIZE passes of `bench.py --only-bind-sweep`, tools/pmc_bind_summary.py)
        try:
            with open(os.path.join(ROOT, "profiles", d, "bind_top_sweep", "bench_traffic.json")) as f:
                t = json.load(f)
        except Exception:
            continue
        if t.get("_curve", "curve25519") == curve:
            sha = t.get("_device_sources_sha256"); now = lib_sha(curve).get("device_sources_sha256")
            t["fresh"] = bool(sha) and sha == now
            t["note"] = "PMC pass taken on these device sources" if t["fresh"] else f"STALE: pass under profiles/{d}/bind_top_sweep taken on other device sources (digest {str(sha)[:12]}, this run {now[:12]})"
            out["traffic"] = t
            break
    return out


def slab_units(kind, c, capacity=False):
    """Per-rank device footprint of ONE proof in slab mode, in units of (s / P) field elements of 32 bytes, from the prover's allocation schedule (lasso_amd/host/prover.hpp;
    DESIGN 5 holds the measured table this is checked against): the two merged committed polynomials dim|read (2C, padded to a power of two) and E (alpha, padded), dim as u32
    (C / 8), the eq table of r and the chi table (2), the primary sumcheck's work arrays (alpha / 2; alpha for LT's clones), and — the peak — the read / write product trees
    (2 per tree, 4 alpha) with the layer's eq table (1/4).  Capacity mode (lasso_host_set_capacity) keeps those trees without their leaf layers: 2 alpha, plus the mini-layers
    of the chunked leaf rounds (2 alpha / 8), and holds dim | read as 4-byte integers only (2C / 8; no field-element copy of that merged polynomial).  The M-sized polynomials,
    generator tables and scratch are the constant term (slab_bytes_per_rank)."""
    alpha = 2 * c if kind == "lt" else c
    p2 = lambda x: 1 << (x - 1).bit_length()
    committed = (2 * c / 8.0 if capacity else p2(2 * c) + c / 8.0) + p2(alpha)
    sumcheck_peak = committed + 2 + (alpha if kind in ("lt", "spark") else alpha / 2.0)     # LT and Spark bind clones of all their polynomials
    trees_peak = committed + (2 * alpha + alpha / 4.0 if capacity else 2 + 4 * alpha) + 0.25            # capacity mode also lets go of the eq / chi tables for the duration of the trees
    return max(sumcheck_peak, trees_peak)


def slab_bytes_per_rank(kind, c, log_s, world, log_m=16, capacity=False):
    """slab_units x (s / P) x 32 bytes + the constant term: the generator tables (per generator 64 window entries + 512 digit multiples of 128 bytes (one cache line per table entry since round 6), + 4096 byte multiples for sets of at most 2^14 generators; the rank's residue class
    again as its slab table; 2 x 255 byte multiples for the commitments' table, of the rank's class only when P > 1) over the three Hyrax widths, and ~1.5 GB of scratch.
    Checked against lasso_mem_stats at configs[3], P = 1, 2, 4, 8 (profiles/r04_slab_peak_bytes.json)."""
    alpha = 2 * c if kind == "lt" else c
    p2 = lambda x: 1 << (x - 1).bit_length()
    width = lambda n_elems: 1 << ((n_elems.bit_length() - 1) - (n_elems.bit_length() - 1) // 2)      # R = 2^(nv - nv / 2), eq_poly.rs:40-42
    r_l, r_e, r_m = width(p2(2 * c) << log_s), width(p2(alpha) << log_s), width(p2(c) << log_m)
    # per generator: 64 window entries + 512 digit multiples, and 4096 byte multiples for sets of up to 2^14 generators (the openings' MSMs, lasso_bases_create_opt) — for the
    # set the openings read (the full one on one GPU, the rank's residue class in slab mode), not in capacity mode
    ent = lambda n_gens, bytes_too: (576 + (4096 if bytes_too and not capacity and n_gens <= (1 << 14) + 64 else 0)) * n_gens
    fixed = 128 * sum(ent(rr + 2, world == 1) + (ent(rr // world + 2, True) if world > 1 else 0) for rr in (r_l, r_e, r_m)) + 2 * 255 * 128 * (r_l + r_e) / world + 1.5e9
    return slab_units(kind, c, capacity) * ((1 << log_s) / world) * 32 + fixed


def slab_worker(a):
    """Child process of the slab leg (one per rank, `bench.py --slab-worker rank,world,device,shm_name`): ONE proof over the ranks, no torch.distributed —
    the ranks meet in the shared-memory segment.  Prints the leg's JSON object on its last stdout line."""
    import hashlib
    from lasso_amd import HostProver, _abi
    rank, world, device, shm_name = a.slab_worker.split(",", 3)
    rank, world, device = int(rank), int(world), int(device)
    kind, c, log_m, log_s = a.slab_kind, a.slab_c, a.log_m, a.slab_log_s
    alpha = 2 * c if kind == "lt" else c
    s = 1 << log_s
    hp = HostProver(device=device, curve=a.curve)
    if a.slab_capacity:
        hp.set_capacity(True)
    if world > 1:
        hp.set_comm_shm(rank, world, shm_name)
    S = _abi.Strategy(_abi.KINDS[kind], c, log_m, a.log_r if kind == "range" else 0)
    idx = hp.gen_indices(s, 1 << log_m, c)                 # the SAME lookups on every rank: one proof
    r = hp.gen_random_point(log_s)
    dev_lib = C.CDLL(device_library_path("curve25519")); _abi.declare(dev_lib)
    t0 = time.perf_counter(); gens = hp.gens(c, s, alpha, log_m); dense = hp.densify(idx, log_m); del idx
    comm = hp.commit(dense, gens); t_setup = time.perf_counter() - t0
    proof = hp.prove(dense, gens, S, r)                    # warm-up
    t0 = time.perf_counter()
    for _ in range(a.slab_steps):
        proof = hp.prove(dense, gens, S, r)
    el = (time.perf_counter() - t0) / a.slab_steps
    rccl = dev_lib.lasso_rccl_ready(hp.ctx())
    mem = hp.mem_stats()
    out = {"workload": f"{kind.upper()} subtable, C={c}, M=2^{log_m}, s=2^{log_s} lookups, ONE proof over {world} GPU(s)" + (" (BASELINE.json configs[3])" if (kind, c, log_s) == ("range", 4, 26) else ""),
           "n_gpus": world, "scaling": "strong", "ms_per_proof": el * 1e3, "value": s / el, "unit": "lookups/s", "steps": a.slab_steps,
           "rccl_ranks": int(rccl), "exchange": ("per-round sums: shared-memory all-gather (lasso_amd/host/shm_comm.hpp); partial row commitments: " +
                                                  ("RCCL ncclAllGather on the library's stream + device-side row sums" if rccl == world and world > 1 else "shared-memory all-gather + host row sums")) if world > 1 else "none (single GPU)",
           "peak_bytes_per_rank": mem["peak_bytes"], "prover_peak_bytes_per_rank": mem["prover_peak_bytes"], "model_bytes_per_rank": int(slab_bytes_per_rank(kind, c, log_s, world, log_m, bool(a.slab_capacity))),
           "capacity_mode": bool(a.slab_capacity),
           "setup_s": round(t_setup, 2), "proof_bytes": len(proof), "proof_sha256": hashlib.sha256(proof).hexdigest(), "commitment_sha256": hashlib.sha256(comm).hexdigest()}
    gold = golden_digest(kind, c, log_m, S.log_r, log_s)
    if gold:     # byte parity of the sharded proof with the ORACLE's proof of the same harness instance (tests/golden/full_config_digests.json)
        out["parity"] = out["proof_sha256"] == gold["proof_sha256"] and out["commitment_sha256"] == gold["commitment_sha256"]
        out["parity_against"] = f"oracle prover digests of this instance (tests/golden/full_config_digests.json; oracle on {gold['threads']} threads, tools/parity_full_configs.py)"
    else:
        out["parity"] = None
    print(json.dumps(out), flush=True)      # the leg's result so far: whatever happens in the capacity pass below, the parent still has this line (it takes the LAST one it can parse)
    if not a.slab_capacity:
        # the same proof once more in capacity mode (lasso_host_set_capacity: product trees without their leaf layers): what a rank holds at most, and what it costs
        try:
            # the representation is densified again under the mode (dim / read then stay 4-byte integers: DensifiedRepresentation::compact)
            hp.free(dense, gens); dense = gens = None     # the generator sets too: under the mode they come without the openings' byte-multiple tables
            hp.set_capacity(True); hp.mem_stats(reset=True)
            gens = hp.gens(c, s, alpha, log_m)
            idx = hp.gen_indices(s, 1 << log_m, c); dense = hp.densify(idx, log_m); del idx
            comm2 = hp.commit(dense, gens)
            p2 = hp.prove(dense, gens, S, r)      # warm-up of the capacity path
            t0 = time.perf_counter(); p2 = hp.prove(dense, gens, S, r); el2 = time.perf_counter() - t0
            m2 = hp.mem_stats()
            out["capacity_mode"] = {"ms_per_proof": el2 * 1e3, "peak_bytes_per_rank": m2["peak_bytes"], "prover_peak_bytes_per_rank": m2["prover_peak_bytes"],
                                    "model_bytes_per_rank": int(slab_bytes_per_rank(kind, c, log_s, world, log_m, True)), "same_bytes_as_pooled": p2 == proof and comm2 == comm,
                                    "compact_dim_read": hp.dense_info(dense)["compact"],
                                    "note": "generator sets + densify + commit + two proofs under lasso_host_set_capacity (the high-water mark was reset after the pooled proofs)"}
        except Exception as e:
            out["capacity_mode"] = {"error": repr(e)[:300]}
    hp.free(dense, gens); hp.close()
    print(json.dumps(out), flush=True)


def slab_leg(a, grp, shm_name):
    """ONE proof over the N ranks (include/lasso_prover.h lasso_host_set_comm_shm): per-round partial sums through the shared-memory exchange, partial row
    commitments through RCCL all-gather on the library's stream when every rank could join the communicator.  Every rank runs the leg in a CHILD process
    (slab_worker) under a timeout: whatever happens in there — an exchange that never completes, a fault in a code path no multi-GPU node has run yet —
    stays in there, and the main line's numbers, final before the leg starts, are printed regardless.  Returns the leg's JSON object (rank 0's child's)."""
    import subprocess
    rank, world = grp.rank, grp.world
    kind, c, log_s = a.slab_kind, a.slab_c, a.slab_log_s
    alpha = 2 * c if kind == "lt" else c
    # 288 GB of HBM3E per GPU, 200 GB budgeted per rank; the model is the prover's allocation schedule (slab_units), checked against lasso_mem_stats at configs[3] for
    # P = 1, 2, 4, 8 (profiles/r04_slab_peak_bytes.json).  A shape that only fits without the trees' leaf layers runs in capacity mode.
    need = slab_bytes_per_rank(kind, c, log_s, world, a.log_m, a.slab_capacity)
    if need > 200e9 and not a.slab_capacity and slab_bytes_per_rank(kind, c, log_s, world, a.log_m, True) <= 200e9:
        a.slab_capacity = True; need = slab_bytes_per_rank(kind, c, log_s, world, a.log_m, True)
    if need > 200e9:
        return {"skipped": f"{kind} C={c} 2^{log_s} needs ~{need / 1e9:.0f} GB per rank on {world} GPU(s) even in capacity mode", "model_bytes_per_rank": int(need)}
    cmd = [sys.executable, os.path.abspath(__file__), "--slab-worker", f"{rank},{world},{grp.device_index},{shm_name}_slab", "--slab-kind", kind, "--slab-c", str(c),
           "--slab-log-s", str(log_s), "--slab-steps", str(a.slab_steps), "--log-m", str(a.log_m), "--log-r", str(a.log_r), "--curve", a.curve] + (["--slab-capacity"] if a.slab_capacity else [])
    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "WORLD_SIZE", "LOCAL_RANK", "MASTER_ADDR", "MASTER_PORT")}   # the child is not a torch.distributed rank
    def last_line(text):
        for ln in reversed([x for x in (text or "").strip().splitlines() if x.startswith("{")]):
            try:
                return json.loads(ln)
            except Exception:
                continue
        return None
    try:
        res = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=a.slab_timeout)
    except subprocess.TimeoutExpired as e:
        got = last_line(e.stdout.decode() if isinstance(e.stdout, bytes) else e.stdout)
        if got:     # the pooled pass finished and printed; only the capacity pass behind it did not
            got["capacity_mode"] = {"error": f"did not finish within {a.slab_timeout:.0f} s"}; return got
        return {"error": f"slab leg did not finish within {a.slab_timeout:.0f} s", "timed_out": True, "n_gpus": world}
    got = last_line(res.stdout)
    if got is None:
        return {"error": f"slab worker exited with {res.returncode}: {res.stderr.strip()[-400:]}", "n_gpus": world}
    if res.returncode != 0:
        got.setdefault("capacity_mode", {"error": f"worker exited with {res.returncode}: {res.stderr.strip()[-300:]}"})
    return got


def self_launch(a):
    """`python bench.py --gpus N` outside a launcher: start the N ranks ourselves (one process per GPU, torch.distributed.run on 127.0.0.1) and pass their
    output through.  With fewer visible GPUs than ranks the ranks share devices over gloo (the N > 1 code path still runs end to end; RCCL needs a GPU per rank)."""
    import socket
    import subprocess
    try:
        import torch
        ngpu = torch.cuda.device_count()
    except Exception:
        ngpu = 0
    with socket.socket() as sk:
        sk.bind(("127.0.0.1", 0)); port = sk.getsockname()[1]
    argv = [x for x in sys.argv[1:]]
    if a.backend is None and ngpu < a.gpus:
        argv += ["--backend", "gloo"]
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={a.gpus}", "--master-addr", "127.0.0.1", "--master-port", str(port), os.path.abspath(__file__)] + argv
    env = dict(os.environ); env.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0"); env["LASSO_BENCH_SELF_LAUNCHED"] = "1"
    return subprocess.call(cmd, env=env)


def main():
    a = parse()
    if a.slab_worker:
        return slab_worker(a)
    if a.gpus > 1 and "WORLD_SIZE" not in os.environ:
        return self_launch(a)
    if a.only_bind_sweep:
        from lasso_amd import HostProver, _abi
        hp = HostProver(curve=a.curve); dev_lib = C.CDLL(device_library_path(a.curve)); _abi.declare(dev_lib)
        print(json.dumps({"bind_top_sweep": bind_top_sweep(dev_lib, hp.ctx(), _abi, a.curve), "lib_sha": lib_sha(a.curve)}), flush=True)
        hp.close()
        return
    from lasso_amd import HostProver, _abi
    from lasso_amd.parallel import Group, shard_indices
    grp = Group(backend=a.backend)     # torch.distributed (nccl = RCCL) only when WORLD_SIZE > 1
    rank, world = grp.rank, grp.world
    hp = HostProver(device=grp.device_index, curve=a.curve)
    slab = a.shard_proof and world > 1
    shm_name = f"/lasso_bench_{os.environ.get('MASTER_PORT', '0')}_{os.getuid()}_{grp.shared_nonce():x}"   # per-job name: a stale segment of a crashed job cannot be picked up
    if slab:
        # slab mode: every polynomial split by low index bits; per-round partial sums through the library's shared-memory exchange, the partial row
        # commitments all-gathered by RCCL over xGMI on the library's stream (lasso_host_set_comm_shm)
        hp.set_comm_shm(rank, world, shm_name + "_main")
    lib = hp.lib
    dev_lib = C.CDLL(device_library_path(a.curve))
    _abi.declare(dev_lib)
    ctx = hp.ctx()

    kind_id = _abi.KINDS[a.kind]
    c, log_m, s = a.c, a.log_m, 1 << a.log_s
    alpha = 2 * c if a.kind == "lt" else c
    S = _abi.Strategy(kind_id, c, log_m, a.log_r if a.kind == "range" else 0)

    t0 = time.time()
    idx = shard_indices(hp, s, 1 << log_m, c, 0 if slab else rank)   # benches/bench.rs:13-21 (rank 0 exactly; other ranks: their own batch, or the same lookups in slab mode)
    r = hp.gen_random_point(a.log_s)                        # benches/bench.rs:27-34
    gens = hp.gens(c, s, alpha, log_m)                      # SparsePolyCommitmentGens::new(b"gens_sparse_poly", C, S, C, log_m)
    t_derive = time.time() - t0                             # indices + point + the generators' derivation, upload and window / digit-multiple tables
    t1 = time.time(); hp.gens_prepare(gens); dev_lib.lasso_sync(ctx); t_tables = time.time() - t1   # the byte-multiple tables of the small-scalar commitments, built eagerly (lasso_host_gens_prepare): not in `commit_s`
    t_setup = time.time() - t0
    t0 = time.time(); dense = hp.densify(idx, log_m); dev_lib.lasso_sync(ctx); t_densify = time.time() - t0
    t0 = time.time(); comm = hp.commit(dense, gens); t_commit = time.time() - t0
    t_commit_warm = None
    if a.full:
        t0 = time.time(); hp.commit(dense, gens); t_commit_warm = time.time() - t0      # the first call also pays first-use costs (kernel load, table faults)

    def barrier():
        dev_lib.lasso_sync(ctx)
        grp.barrier()

    proof = None
    for _ in range(a.warmup):
        proof = hp.prove(dense, gens, S, r)
    # Roofline numbers are measured live, inside the timed region, with HIP events on the library's stream — but only around the launches
    # in the HBM-bound regime (>= 256 MiB of algorithmic bytes, past the Infinity Cache: ~20 per proof), so the brackets cost nothing.
    # Bracketing all ~950 launches of a proof adds ~8% wall time; that full per-family table comes from one extra, untimed, profiled step.
    STREAM = [_abi.K_BIND, _abi.K_CUBIC, _abi.K_COMBINE, _abi.K_EQ, _abi.K_GP, _abi.K_FINGERPRINT, _abi.K_DOT, _abi.K_MATVEC]
    TIMED = STREAM + [_abi.K_MSM]       # the commitment MSM (rows > 16) counts as a large launch: one per proof, bracketed in the timed region as well
    LARGE_ONLY = 0x40000000
    if not a.no_prof:
        dev_lib.lasso_prof_reset(ctx); dev_lib.lasso_prof_enable(ctx, sum(1 << k for k in TIMED) | LARGE_ONLY)
    barrier()
    t0 = time.perf_counter()
    for _ in range(a.steps):
        proof = hp.prove(dense, gens, S, r)
    dev_lib.lasso_sync(ctx)
    elapsed = time.perf_counter() - t0
    barrier()
    if a.dump_outputs and rank == 0:
        dump_outputs(a.dump_outputs, proof)

    def family(kid, large):
        n = C.c_uint64(); ms = C.c_double(); b = C.c_double(); u = C.c_double()
        (dev_lib.lasso_prof_get_large if large else dev_lib.lasso_prof_get)(ctx, kid, C.byref(n), C.byref(ms), C.byref(b))
        dev_lib.lasso_prof_get_units(ctx, kid, 1 if large else 0, C.byref(u))
        if not n.value:
            return None
        out = {"kernel": _abi.KERNEL_NAMES[kid], "launches": n.value, "ms": round(ms.value, 3), "alg_GB": round(b.value / 1e9, 3),
               "alg_GBps": round(b.value / (ms.value * 1e-3) / 1e9, 1) if ms.value > 0 else None, "avg_launch_us": round(ms.value * 1e3 / n.value, 2)}
        if u.value:
            out["ref_group_adds"] = round(u.value); out["ref_G_adds_per_s"] = round(u.value / (ms.value * 1e-3) / 1e9, 2) if ms.value > 0 else None
            dev_lib.lasso_prof_get_units(ctx, kid, (1 if large else 0) | 2, C.byref(u))
            out["executed_madds_upper_bound"] = round(u.value)
            dev_lib.lasso_prof_get_units(ctx, kid, (1 if large else 0) | 4, C.byref(u))      # counted by the kernels (non-zero digits), only in the fully-profiled step
            if u.value:
                out["executed_madds"] = round(u.value)
        return out
    kernels, timed_large = [], {}
    if not a.no_prof:
        dev_lib.lasso_prof_enable(ctx, 0)
        timed_large = {k: family(k, True) for k in TIMED}
        dev_lib.lasso_prof_reset(ctx); dev_lib.lasso_prof_enable(ctx, (1 << _abi.K_COUNT) - 1)
        hp.prove(dense, gens, S, r)                      # extra untimed step, every launch of every family bracketed
        dev_lib.lasso_prof_enable(ctx, 0)
        kernels = [f for f in (family(k, False) for k in range(_abi.K_COUNT)) if f]
    elapsed = grp.max_over_ranks(elapsed)
    digests = grp.gather_digests(proof)
    mem_now = hp.mem_stats()
    peaks = grp.gather_floats(mem_now["peak_bytes"]); rccl_all = grp.gather_floats(dev_lib.lasso_rccl_ready(ctx))

    if rank == 0:
        ms_per_step = elapsed / a.steps * 1e3
        value = (1 if slab else world) * s * a.steps / elapsed
        out = {"metric": "prover lookups/sec for SparsePolynomialEvaluationProof, 2^24 AND lookups" if (a.kind, a.log_s, c) == ("and", 24, 1) else f"prover lookups/sec for SparsePolynomialEvaluationProof, 2^{a.log_s} {a.kind.upper()} lookups",
               "value": value, "unit": "lookups/s", "n_gpus": world, "steps": a.steps, "warmup": a.warmup, "ms_per_step": ms_per_step,
               "higher_is_better": True, "scaling": "strong" if slab else "weak",
               "vs_baseline": (value / PUBLISHED_LOOKUPS_PER_S) if (a.kind, a.log_s, c, a.curve) == ("and", 24, 1, "curve25519") else None, "dtype": "u256 (Montgomery Fr / BN254 Fq integers)" if a.curve == "bn254" else "u256 (Montgomery Fr / ed25519 Fq integers)", "data": "synthetic",
               "config": {"workload": f"{a.kind.upper()} subtable, C={c}, M=2^{log_m}, s=2^{a.log_s} lookups per proof, G={'BN254 G1 (ark_bn254)' if a.curve == 'bn254' else 'curve25519 (ark_curve25519)'}, harness inputs of src/benches/bench.rs; "
                                      f"timed = SparsePolynomialEvaluationProof::prove with the densified representation resident in HBM",
                          "vs_baseline_reference": "2^24 AND lookups, C=1, SparsePoly.prove 35.3 s with rayon on an Apple M1 16 GB (reference's src/benches/m1_16gb_parallel_benches.log:439; BASELINE.md §1)",
                          "per_rank": ("one proof sharded over the ranks by low index bits (slab mode)" if slab else "one independent proof per rank") if world > 1 else "single proof",
                          "proof_bytes": len(proof), "proof_sha256": __import__("hashlib").sha256(proof).hexdigest(), "distinct_proofs": len(set(digests)), "densify_s": round(t_densify, 3), "commit_s": round(t_commit, 3), "commit_warm_s": round(t_commit_warm, 3) if t_commit_warm is not None else None, "gens_setup_s": round(t_setup, 3), "gens_derive_s": round(t_derive, 3), "gens_tables_s": round(t_tables, 3),
                          "whole_bench_lookups_per_s": s / (t_densify + t_commit + ms_per_step / 1e3)}}
        out["lib_sha"] = lib_sha(a.curve)
        out["host"] = host_info()   # the metric depends on the host's share of the Fiat-Shamir chain: say what the host was
        out["config"]["workload_key"] = workload_key(a.kind, c, log_m, a.log_s, a.curve)
        if a.kind == "spark":    # not a parity claim against upstream
            out["config"]["unverified_against_reference"] = ("kind=spark is LASSO_SPARK_UNCONFIRMED: BASELINE.json configs[4] names a SparkSubtableStrategy the reference snapshot does not contain "
                                                             "(src/subtables/mod.rs:22-26); tables, degree and combine function are restated from SURVEY 8(f3)'s one-line description — GPU == this repo's own oracle, nothing more")
        # self-describing multi-GPU line: what ran on how many ranks, which exchange, and what each rank held at most
        out["multi_gpu"] = {"ranks": world, "mode": ("one proof sharded over the ranks by low index bits (slab mode)" if slab else "one independent proof per rank, no data-path collective") if world > 1 else "single GPU",
                            "rccl_ranks": int(min(rccl_all)) if rccl_all else 0,
                            "exchange": ("per-round partial sums: shared-memory all-gather (lasso_amd/host/shm_comm.hpp); partial row commitments: " +
                                         ("RCCL ncclAllGather on the library's stream + device-side row sums" if world > 1 and int(min(rccl_all)) == world else "shared-memory all-gather + host row sums"))
                                        if slab else ("none on the data path; torch.distributed (" + str(a.backend or ("nccl" if world > 1 else "-")) + ") for the timing barrier and the 32-byte proof digests" if world > 1 else "none"),
                            "peak_bytes_per_rank": [int(x) for x in peaks]}
        if os.environ.get("LASSO_BENCH_SELF_LAUNCHED"):
            out["config"]["launched_by"] = "bench.py --gpus N itself (torch.distributed.run, 127.0.0.1)"
        if kernels:
            out["kernels_one_profiled_step"] = kernels
            out["large_launches_timed"] = {v["kernel"]: {"per_step": v["launches"] // a.steps, "alg_bytes_per_launch": round(v["alg_GB"] * 1e9 / v["launches"])} for v in timed_large.values() if v}
            traffic = pmc_traffic(workload_key(a.kind, c, log_m, a.log_s, a.curve))
            def roof(kid):
                """HBM roofline of one kernel family from the launches bracketed inside the timed region (the HBM-bound regime).  `frac` prices the ALGORITHMIC
                bytes of SURVEY 8(d) (what the reference's loop would move); `frac_traffic` prices the bytes the kernel really moved (PMC counters of the
                committed rocprofv3 passes of this command) over the same live-measured time — an eq-weighted or fused kernel that skips bytes gets no credit there."""
                k = timed_large.get(kid)
                if not k:
                    return None
                ach = k["alg_GB"] / (k["ms"] * 1e-3)
                allk = next((x for x in kernels if x["kernel"] == k["kernel"]), None)
                tr = traffic.get(k["kernel"])
                ach_tr = tr["bytes_per_launch"] * k["launches"] / (k["ms"] * 1e-3) / 1e9 if tr else None
                # The counters are a committed rocprofv3 pass, not part of this run: they describe THIS run's kernels only if the device sources are the ones the pass was
                # taken on.  The pass records their digest (tools/pmc_summary.py); anything else is labelled stale instead of passing as measured at HEAD (VERDICT r4 "weak" 6).
                pas = traffic.get("_pass") or {}
                fresh = bool(pas.get("device_sources_sha256")) and pas["device_sources_sha256"] == out["lib_sha"].get("device_sources_sha256")
                return {"kernel": k["kernel"], "bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s", "frac": round(ach / HBM_PEAK_GBS, 4),
                        "traffic": tr["bytes_per_launch"] if tr else None, "achieved_traffic": round(ach_tr, 1) if ach_tr else None,
                        "frac_traffic": round(ach_tr / HBM_PEAK_GBS, 4) if ach_tr else None,
                        "traffic_fresh": fresh if tr else None,
                        "traffic_note": None if not tr else ("PMC pass taken on these device sources" if fresh else
                                                             f"STALE: the PMC pass under {pas.get('dir')} was taken on other device sources (its digest {str(pas.get('device_sources_sha256'))[:12]}, this run's "
                                                             f"{out['lib_sha'].get('device_sources_sha256', '')[:12]}): bytes per launch of an older build of the kernel"),
                        "alg_bytes_per_launch": round(k["alg_GB"] * 1e9 / k["launches"]),
                        "launches": k["launches"], "avg_launch_us": k["avg_launch_us"],
                        "scope": "launches with >= 256 MiB algorithmic bytes, HIP events inside the timed region",
                        "traffic_source": tr["source"] if tr else None,
                        "all_launches_one_profiled_step": {"achieved": allk["alg_GBps"], "launches": allk["launches"], "avg_launch_us": allk["avg_launch_us"]} if allk else None}
            stream_names = [_abi.KERNEL_NAMES[i] for i in STREAM]
            stream = [k for k in kernels if k["kernel"] in stream_names]
            dom = max(stream, key=lambda k: k["ms"]) if stream else None                      # dominant HBM-streaming kernel family by total time
            if dom:
                out["roofline"] = roof(_abi.KERNEL_NAMES.index(dom["kernel"]))
            out["roofline_bind_top"] = roof(_abi.K_BIND)                                        # the kernel BASELINE.json's north_star names (bound_poly_var)
            if out["roofline_bind_top"]:   # inside a proof this family's `frac` is NOT a bandwidth figure
                rb = out["roofline_bind_top"]
                rb["frac_is"] = ("reference-equivalent: the bytes the reference's bound_poly_var_top would move (48 per element of alpha + 1 polynomials) over the measured time.  Inside a proof the "
                                 "family's launches are the primary sumcheck's fused rounds, whose FIRST rounds read the lookup polynomials as u32 values (4 bytes instead of 32) and never bind "
                                 "the eq polynomial, so the kernel moves ~0.4x those bytes: `frac_traffic` (counter-measured bytes) is the bandwidth figure.  The kernel-level figure for "
                                 "k_bind_top on full-width polynomials is `bind_top_sweep` (0.61-0.68 of 8 TB/s at n = 2^24 .. 2^28, traffic 1.005-1.009x algorithmic)")
            # the MSM families are bounded by integer-ALU throughput, not HBM: mixed additions the kernels executed per second against the
            # ISA-derived ceiling of that addition (instructions per pt_madd / the chip's VALU issue peak; tools/madd_isa_count.py, profiles/r04_madd_ceiling.json)
            ceil_ = madd_ceiling(a.curve)
            def roof_msm(kid, src, scope):
                """MSM families: `achieved` = mixed additions the kernels EXECUTED (counted on the device in the profiled step: one per non-zero digit / byte; the
                launches of a step are the same every step) / the measured time; `peak` = VALU issue peak / VALU instructions of one pt_madd (ISA count): no schedule
                of the same arithmetic can exceed it, so this is a utilisation figure <= 1 by construction (asserted below).  `reference_equivalent` prices the additions the reference's msm_bigint_wnaf would
                perform for the same inputs over the same time (it can exceed the ceiling: the kernels' tables remove work), beside — never as — the fraction."""
                k = src.get(kid) if isinstance(src, dict) else next((x for x in src if x["kernel"] == _abi.KERNEL_NAMES[kid]), None)
                prof = next((x for x in kernels if x["kernel"] == _abi.KERNEL_NAMES[kid]), None)
                if not k or not k.get("ref_group_adds"):
                    return None
                large = isinstance(src, dict)
                if large:    # launches bracketed in the timed region: take the exact count per launch from the profiled step's launches of the same class
                    u = C.c_double(); n = C.c_uint64(); ms = C.c_double(); b = C.c_double()
                    dev_lib.lasso_prof_get_units(ctx, kid, 1 | 4, C.byref(u)); dev_lib.lasso_prof_get_large(ctx, kid, C.byref(n), C.byref(ms), C.byref(b))
                    exact_per_launch = u.value / n.value if n.value and u.value else None
                else:
                    exact_per_launch = prof["executed_madds"] / prof["launches"] if prof and prof.get("executed_madds") else None
                ub_per_launch = k["executed_madds_upper_bound"] / k["launches"] if k.get("executed_madds_upper_bound") else None
                per_launch = exact_per_launch or ub_per_launch
                secs = k["ms"] * 1e-3
                ach = per_launch * k["launches"] / secs / 1e9 if per_launch else None
                ref = k["ref_group_adds"] / secs / 1e9
                peak = ceil_["G_madd_per_s"] if ceil_ else None
                return {"kernel": k["kernel"], "bound": "valu (integer multiply-add issue; no MFMA, no HBM stream)", "achieved": round(ach, 2) if ach else None, "peak": peak,
                        "unit": "G mixed additions/s", "frac": round(ach / peak, 4) if ach and peak else None,
                        # the same rate against what a SPILL-FREE chain of nothing but mixed additions sustains on this part at three waves per SIMD (tools/madd_bench.hip,
                        # profiles/r06_madd_ceiling.json: 31.0 G/s on curve25519 = 0.89 of the ISA-derived figure, 17.0 on BN254) — the practical ceiling
                        "frac_microbench": round(ach / ceil_["microbenchmark_G_madd_per_s"], 4) if ach and ceil_ and ceil_.get("microbenchmark_G_madd_per_s") else None,
                        "counted": "on the device (non-zero digits / bytes), profiled step" if exact_per_launch else "upper bound (one per digit read; zero digits are skipped)",
                        "executed_madds_per_launch": round(per_launch) if per_launch else None, "launches": k["launches"], "avg_launch_us": k["avg_launch_us"], "scope": scope,
                        "peak_source": ceil_["source"] if ceil_ else None, "valu_instructions_per_madd": ceil_.get("valu_instructions_per_madd") if ceil_ else None,
                        "microbenchmark_G_madd_per_s": ceil_.get("microbenchmark_G_madd_per_s") if ceil_ else None,
                        "reference_equivalent": {"ref_group_adds_per_launch": round(k["ref_group_adds"] / k["launches"]), "G_ref_adds_per_s": round(ref, 2),
                                                 "note": "additions the reference's msm_bigint_wnaf (msm/mod.rs:91-164, SURVEY 8(d) formula) would perform for the same inputs / the same time; "
                                                         "not a utilisation figure (precomputed window / byte-multiple tables remove bucket reductions and doubling chains)"}}
            def _check_msm(r):   # a utilisation above 1 in a driver-facing line is noise — it would mean the ceiling was measured wrongly (as round 2's was)
                if r and r.get("frac_microbench") is not None and r["frac_microbench"] > 1.0:
                    r["frac_microbench_note"] = "ABOVE 1: the measured ceiling (profiles/r06_madd_ceiling.json) is stale for this build — re-run tools/madd_bench"
                assert not (r and r.get("frac") is not None and r["frac"] > 1.0), "an MSM family above its ISA-derived ceiling: the instruction count is stale (tools/madd_isa_count.py --write)"
                return r
            out["roofline_msm"] = {"commit": roof_msm(_abi.K_MSM, timed_large, "row-parallel commitment MSMs (rows > 16), HIP events inside the timed region"),
                                   "opening": roof_msm(_abi.K_MSM_DIRECT, kernels, "latency-shaped opening MSMs (2 rows of full-width scalars per bullet round), one profiled step")}
            out["roofline_msm"] = {k: _check_msm(v) for k, v in out["roofline_msm"].items()}
            for fam, rm in out["roofline_msm"].items():     # a fraction above 1 is a broken denominator, not a result: say so instead of printing it
                if rm and rm.get("frac") is not None and rm["frac"] > 1.0:
                    rm["error"] = f"frac {rm['frac']} > 1: the ceiling is not a ceiling"; rm["frac"] = None
            if a.kind in ("lt", "spark"):
                # The degree-C strategies' round kernel (prove_arbitrary with a product form, sumcheck.rs:165-255) is VALU-bound, not HBM-bound: per index it evaluates
                # comb_func at d + 1 points, ~alpha field products each (g = prod E_m for Spark; the LT / EQ chain of lt.rs:60-83) — 17 x 16 products per index at C = 16
                # against 32 (alpha + 1) bytes.  Its ceiling is the part's field-product rate (tools/microbench.hip: 180 G reduced 29-bit-limb products/s sustained;
                # 256 CUs x 64 lanes x 2.4 GHz / 210 VALU instructions per fr29_mul = 187 G/s from the ISA), not 8 TB/s (VERDICT r4 "weak" 3).
                kc = next((x for x in kernels if x["kernel"] == _abi.KERNEL_NAMES[_abi.K_COMBINE]), None)
                if kc and kc["ms"] > 0:
                    deg1 = (c + 1) + 1                                                        # sumcheck_poly_degree() + 1 evaluation points
                    n_total = kc["alg_GB"] * 1e9 / (32.0 * (alpha + 1))                        # sum over the launches of the arrays' length (the family's algorithmic bytes are 32 (alpha + 1) n)
                    products = n_total / 2 * deg1 * alpha
                    ach = products / (kc["ms"] * 1e-3) / 1e9
                    # the numerator is the REFERENCE loop's product count; the kernels do fewer (LT: Horner form over pre-scaled arrays, round 0 in 32-bit integer arithmetic — half the
                    # sumcheck's work), so a quotient above 1 is "the reference's products per second", not a utilisation: it is then reported as such and `frac` left null
                    out["roofline_combine"] = {"kernel": kc["kernel"], "bound": "valu (field products; the HBM figure of this family is not its roofline for degree-C strategies)",
                                               "achieved": round(ach, 1), "peak": 180.0, "peak_isa": 187.2, "unit": "G field products/s (reference-loop count)", "frac": round(ach / 180.0, 4) if ach <= 180.0 else None,
                                               "note": None if ach <= 180.0 else "the kernels execute fewer products than the reference's loop (Horner form, integer round 0): reference-equivalent rate, not a utilisation figure",
                                               "products_counted": "reference loop: (n / 2) indices x (d + 1) points x alpha products, summed over the family's launches of one profiled step",
                                               "launches": kc["launches"], "ms": kc["ms"], "peak_source": "tools/microbench.hip (profiles/r02_microbench_sweep_and_ceiling.txt): 180 G fr29 products/s sustained; ISA: 210 VALU instructions per product"}
            allfam = max(kernels, key=lambda k: k["ms"])                                        # over ALL families, streaming or not
            msm_ms = sum(k["ms"] for k in kernels if k["kernel"].startswith("msm"))
            out["dominant_family"] = {"by_time_one_profiled_step": allfam["kernel"], "ms": allfam["ms"], "msm_families_ms": round(msm_ms, 3),
                                      "sum_all_families_ms": round(sum(k["ms"] for k in kernels), 3),
                                      "covered_by": "roofline_msm" if allfam["kernel"].startswith("msm") else ("roofline" if dom and allfam["kernel"] == dom["kernel"] else "kernels_one_profiled_step")}
        if world == 1 and a.concurrent > 1:
            T = a.concurrent
            while T > 1 and T * s * alpha * 450 > 150e9:   # ~400 bytes of HBM per lookup and memory per resident proof
                T //= 2
            if T > 1:
                kms = sum(k["ms"] for k in kernels) if kernels else None
                out["concurrent_proofs"] = concurrent_leg(HostProver, _abi, T, max(2, min(a.steps, 10)), S, c, log_m, a.log_s, a.curve, kms)
        if world == 1 and not a.no_bind_sweep and (a.kind, a.log_s, c) == ("and", 24, 1):
            out["bind_top_sweep"] = bind_top_sweep(dev_lib, ctx, _abi, a.curve)
        if world == 1 and not a.no_cpu_baseline:
            cls = min(a.cpu_log_s, a.log_s)
            cb, o_comm, o_proof = cpu_baseline(kind_id, c, log_m, S.log_r, cls, a.cpu_1t_log_s, a.curve)
            if cb:
                out["cpu_baseline"] = cb
                # parity at the size the claim is made on: the oracle proved the harness instance of 2^cls lookups; the GPU's commitment and proof of the SAME
                # instance (the timed one when the sizes agree, otherwise proved here) must be the same bytes
                if cls == a.log_s:
                    g_comm, g_proof = comm, proof
                else:
                    idx2 = shard_indices(hp, 1 << cls, 1 << log_m, c, 0); r2 = hp.gen_random_point(cls)
                    gens2 = hp.gens(c, 1 << cls, alpha, log_m); dense2 = hp.densify(idx2, log_m)
                    g_comm = hp.commit(dense2, gens2); g_proof = hp.prove(dense2, gens2, S, r2); hp.free(dense2, gens2)
                import hashlib
                out["parity_checked"] = {"log_s": cls, "equal": g_proof == o_proof, "commitment_equal": g_comm == o_comm, "proof_bytes": len(g_proof), "commitment_bytes": len(g_comm),
                                         "proof_sha256": hashlib.sha256(g_proof).hexdigest(), "against": f"oracle prover on {cb['cores']} threads, same harness instance (benches/bench.rs:13-34 inputs)"}
    hp.free(dense, gens)
    hp.close()
    # Extra leg, beside — never instead of — `value`: ONE proof sharded over all N GPUs (slab mode, strong scaling) on the configuration the north star
    # shards (BASELINE.json configs[3] by default).  At N = 1 the same proof on the one GPU: the base of the strong-scaling curve.  The main line's numbers
    # are final before this leg starts; the leg runs in a child process per rank under a timeout, so that nothing in it can take the bench line with it.
    if not a.no_slab_leg and not slab and a.curve == "curve25519":
        res = slab_leg(a, grp, shm_name)
        if rank == 0:
            out["slab_mode"] = res
    if rank == 0:
        print(json.dumps(out), flush=True)
    grp.close()


if __name__ == "__main__":
    main()
