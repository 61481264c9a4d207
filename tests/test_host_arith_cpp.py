"""The product's __host__ __device__ arithmetic headers (lasso_amd/csrc/fr.cuh, fq.cuh, fe29.cuh) checked on the CPU against the
oracle's independent 64-bit arithmetic (tests/cpp/*.cpp).  Both host forms are covered: the 64-bit-limb form g++ builds for the
host prover, and (-DLASSO_HOST_LIMBS32) the 32-bit-limb form the device executes."""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", ["test_arith_host", "test_fe29_host", "test_fr29_host", "test_modinv_host"])
@pytest.mark.parametrize("flags", [[], ["-DLASSO_HOST_LIMBS32"]], ids=["limbs64", "limbs32"])
def test_cpp_arith(name, flags):
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    if not os.path.exists(src):
        pytest.skip(f"{name}.cpp not present")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name + ("_32" if flags else "_64"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "OK" in res.stdout


@pytest.mark.parametrize("name", ["test_bn254_host", "test_fr29_host"])
@pytest.mark.parametrize("flags", [[], ["-DLASSO_HOST_LIMBS32"]], ids=["limbs64", "limbs32"])
def test_cpp_arith_bn254(name, flags):
    """The BN254 build of the same headers (-DLASSO_BN254: the BN254 traits of bn254_fr.cuh / fr29.cuh, bn254_fq.cuh, bn254_fe29.cuh, over mont32.cuh / mont29.cuh) against the oracle's BN254 instantiation."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name + "_bn254" + ("_32" if flags else "_64"))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-DLASSO_BN254", "-DORC_BN254", *flags, "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0, res.stdout[-2000:] + res.stderr[-2000:]
    assert "OK" in res.stdout


@pytest.mark.parametrize("name,flags", [("test_fr29_host", []), ("test_fe29_host", []), ("test_fr29_host", ["-DLASSO_BN254"]), ("test_bn254_host", ["-DLASSO_BN254", "-DORC_BN254"])],
                         ids=["fr29", "fe29", "fr29-bn254", "curve-bn254"])
def test_limb_bounds_hold_under_ubsan(name, flags):
    """The 29-bit-limb forms rely on magnitudes never leaving their 32- / 64-bit containers (no carries between partial products).  The same tests
    built with -fsanitize=undefined turn any signed overflow on the way — in a product column, a lazy sum, a quotient estimate — into a failure, for both
    curve builds (it found the BN254 table conversion feeding a 2^259 value to a reduction that accepts 2^258)."""
    src = os.path.join(ROOT, "tests", "cpp", name + ".cpp")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, name + "_ubsan" + ("_bn254" if flags else ""))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", *flags, "-o", exe, src])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    assert "OK" in res.stdout


MODULI = {
    "Curve25519Fr": 2**252 + 27742317777372353535851937790883648493,
    "Bn254Fr": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
    "Bn254Fq": 21888242871839275222246405745257275088696311157297823662689037894645226208583,
}
# trait -> (field, the constants it must print): the 8 x u32 form (mont32.cuh) and the nine-29-bit-limb form (mont29.cuh)
TRAITS = {
    "curve25519": {"Curve25519FrM32": ("Curve25519Fr", {"p", "INV32", "INV64", "WRAPS", "ONE", "R2"}),
                   "Curve25519FrM": ("Curve25519Fr", {"p", "PINV", "ONE_S", "K5", "K10", "R2S"})},   # its reductions take the quotient from a shift: no QC, no K522
    "bn254": {"Bn254FrM32": ("Bn254Fr", {"p", "INV32", "INV64", "WRAPS", "ONE", "R2"}),
              "Bn254FqM32": ("Bn254Fq", {"p", "INV32", "INV64", "WRAPS", "ONE", "R2"}),
              "Bn254FrM": ("Bn254Fr", {"p", "PINV", "ONE_S", "QC", "K522", "K5", "K10", "R2S"}),
              "Bn254FqM": ("Bn254Fq", {"p", "PINV", "ONE_S", "QC", "K522"})},
}


@pytest.mark.parametrize("curve", ["curve25519", "bn254"])
def test_field_trait_constants(curve):
    """Every constant of every modulus trait (tests/cpp/test_field_traits_host.cpp prints them as integers) against Python's big integers: both limb forms spell
    the same p; INV32 / INV64 / PINV = -p^-1 mod 2^32 / 2^64 / 2^29; ONE, R2 = 2^256, 2^512 mod p; ONE_S, K522, K5, K10, R2S = 2^261, 2^522, 2^266, 2^271, 2^517 mod p;
    QC = floor(2^284 / p); 2^256 < WRAPS p.  The program runs a second time under UBSan."""
    flags = ["-DLASSO_BN254"] if curve == "bn254" else []
    src = os.path.join(ROOT, "tests", "cpp", "test_field_traits_host.cpp")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    outputs = []
    for tag, opt in (("", ["-O2"]), ("_ubsan", ["-O1", "-fsanitize=undefined", "-fno-sanitize-recover=undefined"])):
        exe = os.path.join(out_dir, "test_field_traits_" + curve + tag)
        subprocess.check_call(["g++", *opt, "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, src])
        res = subprocess.run([exe], capture_output=True, text=True, timeout=60)
        assert res.returncode == 0 and "runtime error" not in res.stderr and res.stdout.rstrip().endswith("OK"), res.stdout[-2000:] + res.stderr[-2000:]
        outputs.append(res.stdout)
    assert outputs[0] == outputs[1]
    got = {}
    for line in outputs[0].splitlines()[:-1]:
        name, value = line.split(" = ")
        trait, const = name.split(".")
        assert const not in got.setdefault(trait, {}), line
        got[trait][const] = int(value, 16)
    assert {t: set(c) for t, c in got.items()} == {t: names for t, (_, names) in TRAITS[curve].items()}
    power_of_two = {"ONE": 256, "R2": 512, "ONE_S": 261, "K522": 522, "K5": 266, "K10": 271, "R2S": 517}
    neg_inverse_mod = {"INV32": 32, "INV64": 64, "PINV": 29}
    for trait, (field, _) in TRAITS[curve].items():
        p = MODULI[field]
        for const, v in got[trait].items():
            where = f"{trait}.{const} = {v:#x}"
            if const == "p":
                assert v == p, where
            elif const in power_of_two:
                assert v == pow(2, power_of_two[const], p), where
            elif const in neg_inverse_mod:
                assert v == -pow(p, -1, 2**neg_inverse_mod[const]) % 2**neg_inverse_mod[const], where
            elif const == "QC":
                assert v == 2**284 // p, where
            elif const == "WRAPS":
                assert 2**256 < v * p, where
            else:
                raise AssertionError("unchecked constant " + where)


def extract_poly_math(dst):
    """The pure-arithmetic device functions and accumulation macros of lasso_amd/csrc/poly_kernels.cuh, copied verbatim into a header a host compiler
    can include (the kernels around them need the HIP runtime).  A function is taken from its `__device__ __forceinline__` line (and a `template` line
    before it) to the closing brace in column 0; a macro to its last continuation line."""
    names = ["acc_add", "cubic_terms", "bind29_semi", "bind29", "cubic_eqw_terms", "cubic_eqw_terms2", "combine_lt", "lt_line_step", "lt_line_at", "lt_horner_step", "lt_weighted_acc", "lt_int_limbs", "lt_eq_times_r2"]
    macros = ["CUBIC_ACCUMULATE", "CUBIC_ACCUMULATE2", "LT_FOLD_EVERY"]
    lines = open(os.path.join(ROOT, "lasso_amd", "csrc", "poly_kernels.cuh")).read().split("\n")
    out = ["// generated by tests/test_host_arith_cpp.py from lasso_amd/csrc/poly_kernels.cuh — do not edit", "#pragma once"]
    found = set()
    i = 0
    while i < len(lines):
        ln = lines[i]
        hit = next((n for n in names if ln.startswith("__device__ __forceinline__") and (" " + n + "(") in ln), None)
        mac = next((m for m in macros if ln.startswith("#define " + m + "(")), None)
        if hit:
            if i and lines[i - 1].startswith("template"):
                out.append(lines[i - 1])
            while True:
                out.append(lines[i])
                if lines[i] == "}":
                    break
                i += 1
            found.add(hit)
        elif mac:
            while lines[i].rstrip().endswith("\\"):
                out.append(lines[i]); i += 1
            out.append(lines[i]); found.add(mac)
        i += 1
    assert found == set(names) | set(macros), f"not found in poly_kernels.cuh: {(set(names) | set(macros)) - found}"
    with open(dst, "w") as f:
        f.write("\n".join(out) + "\n")


@pytest.mark.parametrize("curve_flags", [[], ["-DLASSO_BN254"]], ids=["curve25519", "bn254"])
@pytest.mark.parametrize("san", [[], ["-fsanitize=undefined", "-fno-sanitize-recover=undefined"]], ids=["plain", "ubsan"])
def test_kernel_per_index_math(curve_flags, san):
    """The sumcheck kernels' per-index arithmetic (extracted from poly_kernels.cuh, not restated), driven like their per-thread loops over three
    consecutive rounds, against fr.cuh — and, under UBSan, with every limb and column magnitude checked to stay inside its container."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    extract_poly_math(os.path.join(out_dir, "poly_math_extract.hpp"))
    exe = os.path.join(out_dir, "test_poly_math" + ("_bn254" if curve_flags else "") + ("_ubsan" if san else ""))
    subprocess.check_call(["g++", "-O1", "-std=c++17", "-Wno-unknown-pragmas", "-I" + out_dir, *curve_flags, *san, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_poly_math_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=900)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    assert "OK" in res.stdout


@pytest.mark.parametrize("curve_flags", [[], ["-DLASSO_BN254"]], ids=["curve25519", "bn254"])
def test_lane_distributed_transcript(curve_flags):
    """tools/transcript_dev.cuh (Keccak-f / STROBE-128 / Merlin with the state spread over 25 lanes — the measured-and-dropped experiment of deriving challenges
    on the device, kept reproducible) against the host transcript on random schedules of appends and challenges, and the 64-byte -> Fr reduction of challenge_scalar."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_transcript_dev" + ("_bn254" if curve_flags else ""))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "lasso_amd", "csrc"), *curve_flags, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_transcript_dev_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=600)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-1000:] + res.stderr[-2000:]


def test_handoff_encodings_device_against_host():
    """The tagged result chunks and the mailbox chunks: the kernels' writer / checker and the host's checker / writer (lasso_amd/csrc/handoff_device.cuh, handoff.cuh),
    compiled for the host, accept each other's output and refuse stale, torn or corrupted chunks; and the protocol's state machine walked through every sequence the prover uses."""
    clang = "/opt/rocm/lib/llvm/bin/clang++"
    if not os.path.exists(clang):
        pytest.skip("needs clang (ext_vector_type) for the device-side helpers")
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_handoff_host")
    subprocess.check_call([clang, "-O1", "-std=c++17", "-msse2", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_handoff_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "runtime error" not in res.stderr, res.stdout[-1000:] + res.stderr[-3000:]
    assert "OK" in res.stdout



def test_product_merlin_equals_the_oracles_on_random_schedules():
    """lasso_amd/host/hashes.hpp (incl. the one-pass append of a framed record, Strobe::append_framed) against oracle/hashes.hpp on random append / challenge schedules"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_hashes_cross")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_hashes_cross.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


def test_product_byte_layer_against_published_vectors():
    """lasso_amd/host/hashes.hpp — the product's own SHAKE256 / Merlin / ChaCha (a private copy of the layer the oracle restates) — against vectors the crates
    themselves publish: rand 0.8 StdRng value stability on ark_std::test_rng()'s seed, rand_chacha's true_values_a, draft-strombergson ChaCha12, FIPS 202, merlin 3.0."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_published_vectors_host")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_published_vectors_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("flags", [[], ["-DLASSO_BN254"], ["-DLASSO_HOST_LIMBS32"]], ids=["curve25519", "bn254", "portable-fallback"])
def test_host_only_field_forms(flags):
    """field_host.hpp's host-only forms (fr_add_host / fr_sub_host, H4) == the shared arithmetic, both curves and the portable fall-back"""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_h4_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_h4_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("flags", [[], ["-DLASSO_BN254"]], ids=["curve25519", "bn254"])
def test_host_rounds_eight_at_a_time_equal_the_scalar_loop(flags):
    """field52.hpp (AVX-512 IFMA: Fr in five 52-bit limbs, eight elements per register, lazily reduced; three Montgomery products side by side) against the scalar H4 loop of
    prover.hpp host_cubic_rounds: every round's three sums, the binds, the final heads (A_c[0] recovered as A'_c[0] / w_c) — bit for bit, k = 1..16 circuits x 2..256 elements,
    edge values (0, 1, p - 1) included.  "SKIP" where the CPU has no IFMA (the prover then keeps the scalar loop)."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_field52_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.check_call(["g++", "-O2", "-march=x86-64-v3", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_field52_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and ("OK" in res.stdout or "SKIP" in res.stdout), res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("flags", [[], ["-DLASSO_BN254"]], ids=["curve25519", "bn254"])
def test_sumcheck_phase_plan(flags):
    """sumcheck_phase.hpp — the one plan linear_rounds and cubic_rounds share: tail_from, host_m_stop and host_handover against a literal restatement of the loops the two drivers
    carried (0..3 and more rounds, arrays of 2 and 4 elements, the resident kernel's capacity met exactly and exceeded by one step, a zero coordinate at the tail's first round and
    before it, 1..33 circuits against the host budgets), EqPhase's inverse prefix products, `degenerate`, and the per-round scalars against the drivers' own expressions."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_phase_plan_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", *flags, "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_phase_plan_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]


@pytest.mark.parametrize("flags", [[], ["-DLASSO_BN254"]], ids=["curve25519", "bn254"])
def test_device_launch_plans(flags):
    """csrc/launch_plan.cuh — which kernel serves an MSM or a sumcheck round, its grid and its scratch — against a literal restatement of the conditions run_msm, run_msm_direct,
    bullet_round_fused and cubic_eqw_launch_t carried inline, field for field, on both sides of every boundary (16/17, 31/32, 255/256, 1023/1024 rows; W <= 4; n_cols * W8 <= 8192;
    511/512 columns; K == 1; 64 indices per circuit; ell 14/15; nx <= LASSO_DIRECT_NX; LASSO_MSM_DIRECT_WGS 1, 3, 4, 4096, 4097 under both users' rules), with every combination of
    tables and switches; and the invariants the kernels rely on (chunks cover the columns, waves the rows, the reserved scratch whichever plan is chosen).  Under UBSan."""
    out_dir = os.path.join(ROOT, "tests", "_build")
    os.makedirs(out_dir, exist_ok=True)
    exe = os.path.join(out_dir, "test_launch_plan_host" + "".join(f.replace("-D", "_") for f in flags))
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-Wno-unknown-pragmas", "-fsanitize=undefined", "-fno-sanitize-recover=undefined", *flags, "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_launch_plan_host.cpp")])
    res = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert res.returncode == 0 and "OK" in res.stdout, res.stdout[-2000:] + res.stderr[-2000:]
