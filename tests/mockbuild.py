"""The one CPU build of the host prover (lasso_amd/host/prover_capi.cpp) against the oracle's mock of the device ABI (tests/cpp/mock_device.cpp over oracle/mock_hip.cpp),
with any set of the optional device entries (lasso_amd/_abi.py EXTENSIONS, plus "custom": caller-defined strategies can be PROVED) and, optionally, a harness linked in."""
import glob
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OUT = os.path.join(ROOT, "tests", "_build")
CPP = os.path.join(ROOT, "tests", "cpp")
EXTS = ("custom", "wire", "msm_points", "operands", "gens", "mle", "values", "poly")        # each is tests/cpp/mock_<ext>_wrap.cpp, included under -DMOCK_EXT_<EXT>
REQUIRES = {"values": ("custom",), "operands": ("custom",)}      # values calls custom's custom_g; a strategy proved from operands may be a caller-defined one
FLAGS = ["g++", "-O2", "-std=c++17", "-fPIC", "-Wno-unknown-pragmas", "-fno-gnu-unique"]    # see oracle/Makefile


def closure(ext):
    """`ext` and what its members require, sorted"""
    ext = set(ext)
    assert ext <= set(EXTS), ext - set(EXTS)
    return sorted(ext.union(*(REQUIRES.get(e, ()) for e in ext)))


def inputs(root=ROOT):
    """every file a mock build may read: the same list for every variant, so none can go stale unnoticed (a build is seconds; a missed rebuild is a wrong test)"""
    pats = ("lasso_amd/host/*.[ch]pp", "lasso_amd/csrc/*.cuh", "oracle/*.[ch]pp", "include/*.h", "tests/cpp/*.cpp", "tests/mockbuild.py")
    return sorted(f for p in pats for f in glob.glob(os.path.join(root, p)))


def stale(target, sources):
    return not os.path.exists(target) or any(os.path.getmtime(s) > os.path.getmtime(target) for s in sources)


def _run(target, cmd):
    """`cmd -o target`.  Several test processes may find a file stale at once: each writes its own, the rename is atomic"""
    os.makedirs(OUT, exist_ok=True)
    tmp = f"{target}.{os.getpid()}.tmp"
    with open(os.path.join(OUT, "build.log"), "a") as log:      # one line per compiler run
        log.write(" ".join(cmd + ["-o", target]) + "\n")
    subprocess.check_call(cmd + ["-o", tmp])
    os.replace(tmp, target)


def build_mock_prover(curve="curve25519", ext=(), harness=(), extra_flags=()):
    """tests/_build/liblasso_prover_mock[_<ext>...][_<harness>...][_bn254].so: the host prover over the mock with the entries of `ext` (and what they require) present
    — the weak references of prover_capi.cpp to them resolve, every other optional entry stays absent — and the sources `harness` (names under tests/cpp) linked in.
    prover_capi.cpp, the same in every variant, is compiled once per curve."""
    bn = curve == "bn254"
    cflags = FLAGS + (["-DLASSO_BN254", "-DORC_BN254"] if bn else [])
    suffix = "_bn254" if bn else ""
    ext = closure(ext)
    obj = os.path.join(OUT, f"prover_capi{suffix}.o")
    so = os.path.join(OUT, "_".join(["liblasso_prover_mock", *ext, *(os.path.splitext(h)[0] for h in harness)]) + suffix + ".so")
    src = inputs()
    if stale(so, src):
        if stale(obj, src):      # an intermediate, looked at only when a library needs it: a tree that brings its libraries along need not bring it
            _run(obj, cflags + ["-c", os.path.join(ROOT, "lasso_amd", "host", "prover_capi.cpp")])
        _run(so, cflags + ["-shared", "-Wl,-Bsymbolic", *extra_flags, *(f"-DMOCK_EXT_{e.upper()}" for e in ext), *(os.path.join(CPP, h) for h in harness), obj,
                           os.path.join(CPP, "mock_device.cpp")])
    return so
