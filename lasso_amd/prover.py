"""Python view of the host prover (include/lasso_prover.h): the reference's three calls — DensifiedRepresentation::from_lookup_indices,
DensifiedRepresentation::commit, SparsePolynomialEvaluationProof::prove (src/benches/bench.rs:54-66) — over liblasso_prover.so.
No CPU fallback: the default library is the HIP-backed one and loading fails loudly if it is missing."""
import ctypes as C
import os

import numpy as np

from . import _abi
from ._abi import APPEND_FN, CHALLENGE_FN, TranscriptVtbl  # noqa: F401
from .custom import strategy_ptr
from .device import LassoError

HERE = os.path.dirname(os.path.abspath(__file__))


def load_prover_library(path=None, curve="curve25519"):
    """curve = "bn254": the BN254 pair (liblasso_prover_bn254.so over liblasso_hip_bn254.so); both pairs can live in one process."""
    # LASSO_PROVER_LIB: an explicit path to another build of the SAME C ABI (the CPU tests of bench.py's multi-rank plumbing point it at the host sources linked
    # against the test mock of the device ABI).  Never set by the package itself; when unset the HIP-backed library is the only candidate and its absence is fatal.
    path = path or os.environ.get("LASSO_PROVER_LIB") or os.path.join(HERE, "liblasso_prover_bn254.so" if curve == "bn254" else "liblasso_prover.so")
    if not os.path.exists(path):
        raise LassoError(f"{path} is missing: build it with `python -c 'import __graft_entry__ as g; g.build()'` (no CPU fallback exists)")
    return C.CDLL(path)


ALLGATHER_FN = C.CFUNCTYPE(C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t)   # (user, send, recv, bytes per rank) -> 0


def declare_prover(lib):
    vp, sz, i32 = C.c_void_p, C.c_size_t, C.c_int32
    lib.lasso_host_last_error.restype = C.c_char_p
    lib.lasso_host_create.argtypes = [i32, C.POINTER(vp)]
    lib.lasso_host_destroy.argtypes = [vp]
    lib.lasso_host_ctx.argtypes = [vp]; lib.lasso_host_ctx.restype = vp
    u64p = C.POINTER(C.c_uint64)
    lib.lasso_host_mem_stats.argtypes = [vp, u64p, u64p, u64p, i32]
    lib.lasso_host_set_capacity.argtypes = [vp, i32]
    lib.lasso_host_set_throughput_mode.argtypes = [vp, i32]
    lib.lasso_host_set_comm.argtypes = [vp, i32, i32, ALLGATHER_FN, vp]
    lib.lasso_host_set_comm_shm.argtypes = [vp, i32, i32, C.c_char_p]
    lib.lasso_host_gens_new.argtypes = [vp, C.c_char_p, sz, sz, sz, sz, C.POINTER(vp)]
    lib.lasso_host_gens_from_points.argtypes = [vp, sz, sz, sz, sz, vp, sz, vp, sz, vp, sz, C.POINTER(vp)]
    lib.lasso_host_gens_prepare.argtypes = [vp]
    lib.lasso_host_gens_points.argtypes = [vp, i32, vp, sz, C.POINTER(sz)]
    lib.lasso_host_gens_free.argtypes = [vp]
    lib.lasso_host_densify.argtypes = [vp, vp, sz, sz, sz, C.POINTER(vp)]
    lib.lasso_host_dense_free.argtypes = [vp]
    lay = C.POINTER(_abi.OperandLayout)
    lib.lasso_host_operand_layout.argtypes = [C.POINTER(_abi.Strategy), lay]
    lib.lasso_host_operand_indices.argtypes = [lay, vp, vp, sz, sz, sz, vp]
    lib.lasso_host_densify_operands.argtypes = [vp, lay, vp, vp, sz, sz, sz, i32, C.POINTER(vp)]
    lib.lasso_host_densify_stats.argtypes = [vp, u64p, C.POINTER(i32), i32]
    lib.lasso_host_dense_info.argtypes = [vp, u64p, C.POINTER(C.c_int32)]
    lib.lasso_host_commit.argtypes = [vp, vp, vp, sz, C.POINTER(sz)]
    lib.lasso_host_prove.argtypes = [vp, vp, vp, C.POINTER(_abi.Strategy), vp, sz, C.c_char_p, C.c_char_p, vp, sz, C.POINTER(sz)]
    lib.lasso_host_verify.argtypes = [vp, vp, C.POINTER(_abi.Strategy), sz, vp, sz, C.c_char_p, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(i32)]
    lib.lasso_host_debug_cubic_batched.argtypes = [vp, vp, vp, C.POINTER(_abi.Strategy), sz, sz, vp, vp, vp, vp, vp, C.c_char_p, vp, sz, C.POINTER(sz)]
    vt = C.POINTER(TranscriptVtbl)
    lib.lasso_host_prove_cb.argtypes = [vp, vp, vp, C.POINTER(_abi.Strategy), vp, sz, vt, vp, vt, vp, vp, sz, C.POINTER(sz)]
    lib.lasso_host_verify_cb.argtypes = [vp, vp, C.POINTER(_abi.Strategy), sz, vp, sz, vt, vp, C.c_char_p, sz, C.c_char_p, sz, C.POINTER(i32)]
    lib.lasso_host_merlin_new.argtypes = [C.c_char_p]; lib.lasso_host_merlin_new.restype = vp
    lib.lasso_host_random_tape_new.argtypes = [C.c_char_p]; lib.lasso_host_random_tape_new.restype = vp
    lib.lasso_host_merlin_free.argtypes = [vp]
    lib.lasso_host_merlin_vtbl.argtypes = []; lib.lasso_host_merlin_vtbl.restype = vt
    lib.lasso_host_strategy_check.argtypes = [C.POINTER(_abi.Strategy)]
    lib.lasso_host_points_decompress.argtypes = [vp, vp, sz, i32, vp, vp, vp]
    lib.lasso_host_wire_stats.argtypes = [vp, u64p, C.POINTER(i32), i32]
    lib.lasso_host_msm_points.argtypes = [vp, vp, vp, sz, vp]
    lib.lasso_host_msm_stats.argtypes = [vp, u64p, C.POINTER(i32), i32]
    lib.lasso_host_points_from_candidates.argtypes = [vp, vp, vp, sz, i32, vp, vp]
    lib.lasso_host_gens_stats.argtypes = [vp, u64p, C.POINTER(i32), i32]
    lib.lasso_host_gen_indices.argtypes = [sz, sz, vp]
    lib.lasso_host_gen_random_point.argtypes = [sz, vp]
    return lib


class HostProver:
    """One lasso_host (device context + host prover). `lib` defaults to the product library; tests may inject the mock-backed build."""

    def __init__(self, lib=None, device=0, curve="curve25519"):
        self.lib = declare_prover(lib or load_prover_library(curve=curve))
        h = C.c_void_p()
        if self.lib.lasso_host_create(device, C.byref(h)) != 0:
            raise LassoError("lasso_host_create: " + self.lib.lasso_host_last_error().decode())
        self.h = h
        self.device = device

    def set_comm(self, group):
        """Slab mode (one proof sharded over the ranks of `group`, lasso_amd.parallel.Group): must precede gens()/densify()."""
        self._allgather = ALLGATHER_FN(group.allgather_callback())       # keep the callback object alive
        self._chk(self.lib.lasso_host_set_comm(self.h, group.rank, group.world, self._allgather, None))

    def set_comm_shm(self, rank, world, name):
        """Slab mode over the library's own shared-memory exchange (one node): `name` = "/something", the same on every rank."""
        self._chk(self.lib.lasso_host_set_comm_shm(self.h, rank, world, name.encode()))

    def _chk(self, rc):
        if rc != 0:
            raise LassoError(f"lasso_host error {rc}: " + self.lib.lasso_host_last_error().decode())

    def _ext(self, name):
        """the library with the optional prover header `name` (_abi.PROVER_EXTENSIONS) declared on first use; LassoError when the library does not export it"""
        return _abi.declared_ext(self, name, _abi.PROVER_EXTENSIONS, "prover", LassoError)

    def _values_fns(self):
        return self._ext("values")

    def _poly_fns(self):
        return self._ext("poly")

    def _stats(self, fn, reset, *keys):
        """one lasso_host_*_stats call as a dict: `keys` name its counters and, last, whether the device library has the entry"""
        counts, avail = [C.c_uint64() for _ in keys[:-1]], C.c_int32()
        self._chk(fn(self.h, *map(C.byref, counts), C.byref(avail), 1 if reset else 0))
        return {**{k: v.value for k, v in zip(keys, counts)}, keys[-1]: bool(avail.value)}

    def gen_indices(self, s, m, c):
        one = np.empty(s, dtype=np.uint64)
        self.lib.lasso_host_gen_indices(s, m, one.ctypes.data_as(C.c_void_p))
        return np.repeat(one[:, None], c, axis=1).copy()     # `[x; C]`: one draw per lookup, replicated (benches/bench.rs:17)

    def gen_random_point(self, bits):
        r = np.empty((max(bits, 1), 4), dtype=np.uint64)
        self.lib.lasso_host_gen_random_point(bits, r.ctypes.data_as(C.c_void_p))
        return r[:bits]

    def gens(self, c, s, num_memories, log_m, label=b"gens_sparse_poly"):
        g = C.c_void_p()
        self._chk(self.lib.lasso_host_gens_new(self.h, label, c, s, num_memories, log_m, C.byref(g)))
        return g

    def gens_prepare(self, gens):
        """build every device table a proof over `gens` reads now instead of inside the first commit / prove (lasso_host_gens_prepare)"""
        self._chk(self.lib.lasso_host_gens_prepare(gens))

    def gens_from_points(self, c, s, num_memories, log_m, l_variate, log_m_variate, derefs):
        """The caller's generators (surge.rs:119-125 `gens: &SparsePolyCommitmentGens<G>`): three arrays of shape (n + 2, 8) uint64 — affine (x, y) Montgomery limbs in the
        order G[0..n), gens_1.G[0], h (lasso_host_gens_from_points)."""
        sets = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1, 8) for a in (l_variate, log_m_variate, derefs)]
        g = C.c_void_p()
        args = []
        for a in sets:
            args += [a.ctypes.data_as(C.c_void_p), a.shape[0]]
        self._chk(self.lib.lasso_host_gens_from_points(self.h, c, s, num_memories, log_m, *args, C.byref(g)))
        return g

    def gens_points(self, gens, which):
        """the points of generator set `which` (0 l-variate, 1 log_m-variate, 2 derefs) as an (n + 2, 8) uint64 array (lasso_host_gens_points)"""
        n = C.c_size_t()
        self.lib.lasso_host_gens_points(gens, which, None, 0, C.byref(n))
        out = np.empty((n.value, 8), dtype=np.uint64)
        self._chk(self.lib.lasso_host_gens_points(gens, which, out.ctypes.data_as(C.c_void_p), n.value, C.byref(n)))
        return out

    def densify(self, indices, log_m):
        indices = np.ascontiguousarray(indices, dtype=np.uint64)
        d = C.c_void_p()
        self._chk(self.lib.lasso_host_densify(self.h, indices.ctypes.data_as(C.c_void_p), indices.shape[0], indices.shape[1], log_m, C.byref(d)))
        return d

    def operand_layout(self, strategy):
        """the operand layout of a built-in strategy (lasso_host_operand_layout): AND / OR / XOR (2, log_m / 2, 0), LT (2, log_m / 2, 1), RangeCheck (1, log_m, 0);
        LassoError for a strategy without one (the caller then passes its own _abi.OperandLayout)"""
        out = _abi.OperandLayout()
        self._chk(self.lib.lasso_host_operand_layout(strategy_ptr(strategy), C.byref(out)))
        return out

    def operand_indices(self, x, y=None, *, layout, c, log_m):
        """the (n, c) uint64 lookup indices of the operand columns x, y under `layout` (lasso_host_operand_indices): the normative CPU statement of the layout, what
        densify() takes"""
        x = np.ascontiguousarray(x, dtype=np.uint64).reshape(-1)
        y = None if y is None else np.ascontiguousarray(y, dtype=np.uint64).reshape(-1)
        if y is not None and y.shape != x.shape:
            raise LassoError("operand_indices: x and y must have the same length")
        out = np.zeros((x.shape[0], c), dtype=np.uint64)
        vpt = lambda a: None if a is None else a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.lasso_host_operand_indices(C.byref(layout), vpt(x), vpt(y), x.shape[0], c, log_m, vpt(out)))
        return out

    def densify_operands(self, x, y=None, *, layout, c, log_m):
        """densify(operand_indices(x, y)) without the index array (lasso_host_densify_operands): each dimension's addresses are formed on the device inside its densify
        pass.  x, y: numpy uint64 arrays (uploaded: 8 bytes per operand and lookup, whatever c is), or torch tensors ALREADY ON THE GPU — contiguous, one-dimensional int64
        (reinterpreted as unsigned) on the device of this host's context — which are used where they are.  y = None for a one-operand layout."""
        cols = [a for a in (x, y) if a is not None]
        on_device = [hasattr(a, "data_ptr") and hasattr(a, "is_cuda") for a in cols]
        if any(on_device) != all(on_device):
            raise LassoError("densify_operands: x and y must both be numpy arrays or both be tensors on the GPU")
        d = C.c_void_p()
        if all(on_device):
            import torch
            for a in cols:
                if not a.is_cuda or a.dtype != torch.int64 or a.dim() != 1 or not a.is_contiguous() or a.shape != cols[0].shape or a.device.index != self.device:
                    raise LassoError(f"densify_operands: tensors must be one-dimensional contiguous int64 of one length on GPU {self.device}, the device of this host's context")
            torch.cuda.current_stream(cols[0].device).synchronize()      # whatever wrote the columns has finished; the call below is synchronous, `cols` holds the references
            ptrs = [C.c_void_p(a.data_ptr()) for a in cols] + [None] * (2 - len(cols))
            self._chk(self.lib.lasso_host_densify_operands(self.h, C.byref(layout), ptrs[0], ptrs[1], cols[0].shape[0], c, log_m, 1, C.byref(d)))
            return d
        cols = [np.ascontiguousarray(a, dtype=np.uint64).reshape(-1) for a in cols]
        if len(cols) == 2 and cols[1].shape != cols[0].shape:
            raise LassoError("densify_operands: x and y must have the same length")
        ptrs = [a.ctypes.data_as(C.c_void_p) for a in cols] + [None] * (2 - len(cols))
        self._chk(self.lib.lasso_host_densify_operands(self.h, C.byref(layout), ptrs[0], ptrs[1], cols[0].shape[0], c, log_m, 0, C.byref(d)))
        return d

    def densify_stats(self, reset=False):
        """{"operand_dims_on_device": dimensions this host densified through lasso_densify_dim_operands so far, "available": whether the device library has that entry}
        (lasso_host_densify_stats)"""
        return self._stats(self.lib.lasso_host_densify_stats, reset, "operand_dims_on_device", "available")

    def dense_info(self, dense):
        """device bytes a densified representation holds, and whether dim / read are in capacity mode's compact form"""
        b, c = C.c_uint64(), C.c_int32()
        self._chk(self.lib.lasso_host_dense_info(dense, C.byref(b), C.byref(c)))
        return {"device_bytes": b.value, "compact": bool(c.value)}

    _cap = 1 << 22      # output buffer of the byte-returning calls: a proof is 0.15 MB (C = 1) to 1.3 MB (C = 16); grows, and stays grown, if a call reports more

    def _bytes_call(self, fn, *args):
        while True:
            cap = self._cap
            buf = (C.c_uint8 * cap)()
            n = C.c_size_t()
            rc = fn(*args, buf, cap, C.byref(n))
            if rc == -2 and n.value > cap:      # the call ran to the end before it knew (a proof is proved to be measured): never pay that twice for one shape
                self._cap = 2 * n.value
                continue
            self._chk(rc)
            return bytes(buf[: n.value])

    def commit(self, dense, gens):
        return self._bytes_call(self.lib.lasso_host_commit, dense, gens)

    def prove(self, dense, gens, strategy, r, transcript=b"example", tape=b"proof"):
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        return self._bytes_call(self.lib.lasso_host_prove, self.h, dense, gens, strategy_ptr(strategy), r.ctypes.data_as(C.c_void_p), r.shape[0], transcript, tape)

    def prove_with(self, dense, gens, strategy, r, transcript, tape):
        """SparsePolynomialEvaluationProof::prove against LIVE transcripts (surge.rs:119-125 `&mut Transcript`, `&mut RandomTape`): `transcript` / `tape` are
        (vtbl pointer, user pointer) pairs — lasso_host_prove_cb; see Transcript below for the library's own Merlin behind that interface"""
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        return self._bytes_call(lambda *a: self.lib.lasso_host_prove_cb(self.h, dense, gens, strategy_ptr(strategy), r.ctypes.data_as(C.c_void_p), r.shape[0], transcript[0], transcript[1], tape[0], tape[1], *a))

    def verify_with(self, gens, strategy, s, r, proof, commitment, transcript):
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int32(-1)
        self._chk(self.lib.lasso_host_verify_cb(self.h, gens, strategy_ptr(strategy), s, r.ctypes.data_as(C.c_void_p), r.shape[0], transcript[0], transcript[1], proof, len(proof), commitment, len(commitment), C.byref(ok)))
        return ok.value == 1

    def verify(self, gens, strategy, s, r, proof, commitment, transcript=b"example"):
        """SparsePolynomialEvaluationProof::verify (surge.rs:214-271) over the wire bytes: True = Ok(()), False = Err(ProofVerifyError); raises LassoError on bytes
        that do not deserialize or on shapes the reference would assert on."""
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int32(-1)
        self._chk(self.lib.lasso_host_verify(self.h, gens, strategy_ptr(strategy), s, r.ctypes.data_as(C.c_void_p), r.shape[0], transcript, proof, len(proof), commitment, len(commitment), C.byref(ok)))
        return ok.value == 1

    def points_decompress(self, wire, where=0):
        """compressed points -> (affine (n, 8) uint64, canonical (n, 32) uint8, status (n,) uint8), decoded on the host (where=0: the verifier's own decoder) or on the
        device (where=1: one launch; LassoError when the device library has no decoder) — lasso_host_points_decompress"""
        w = np.ascontiguousarray(np.frombuffer(wire, dtype=np.uint8) if isinstance(wire, (bytes, bytearray, memoryview)) else np.asarray(wire, dtype=np.uint8)).reshape(-1)
        if w.size % 32:
            raise LassoError("points_decompress: the input is not a whole number of 32-byte encodings")
        n = w.size // 32
        aff = np.zeros((n, 8), dtype=np.uint64); canon = np.zeros((n, 32), dtype=np.uint8); status = np.zeros(n, dtype=np.uint8)
        vpt = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.lasso_host_points_decompress(self.h, vpt(w), n, where, vpt(aff), vpt(canon), vpt(status)))
        return aff, canon, status

    def wire_stats(self, reset=False):
        """{"device_points": compressed points this host decoded on the device so far, "device_available": whether the device decoder exists} (lasso_host_wire_stats)"""
        return self._stats(self.lib.lasso_host_wire_stats, reset, "device_points", "device_available")

    def msm_points(self, points, scalars):
        """VariableBaseMSM::msm over the caller's own points, nothing prepared (lasso_host_msm_points): `points` = (n, 8) uint64 affine Montgomery limbs (an all-zero row
        is the identity), `scalars` = (n, 4) uint64.  Returns the 32 wire bytes of the sum; LassoError when the device library has no such entry."""
        points = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
        scalars = np.ascontiguousarray(scalars, dtype=np.uint64).reshape(-1, 4)
        if points.shape[0] != scalars.shape[0]:
            raise LassoError("msm_points: as many scalars as points are needed")
        out = np.zeros(32, dtype=np.uint8)
        vpt = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.lasso_host_msm_points(self.h, vpt(points), vpt(scalars), points.shape[0], vpt(out)))
        return out.tobytes()

    def msm_stats(self, reset=False):
        """{"points_calls": the verifier's MSMs over commitment rows that ran table-free on this host so far, "available": whether the device library has
        lasso_msm_points} (lasso_host_msm_stats)"""
        return self._stats(self.lib.lasso_host_msm_stats, reset, "points_calls", "available")

    def points_from_candidates(self, limbs, greatest, where=0):
        """candidates of a label's generator stream -> (affine (n, 8) uint64, status (n,) uint8), on the host (where=0: one after the other) or on the device (where=1:
        one launch; LassoError when the device library has no such entry) — lasso_host_points_from_candidates.  `limbs` = (n, 4) uint64, `greatest` = (n,) root choices."""
        limbs = np.ascontiguousarray(limbs, dtype=np.uint64).reshape(-1, 4)
        g = np.ascontiguousarray(np.asarray(greatest).astype(bool), dtype=np.uint8).reshape(-1)
        n = limbs.shape[0]
        if g.shape[0] != n:
            raise LassoError("points_from_candidates: as many root choices as candidates are needed")
        aff = np.zeros((n, 8), dtype=np.uint64); status = np.zeros(n, dtype=np.uint8)
        vpt = lambda a: a.ctypes.data_as(C.c_void_p)
        self._chk(self.lib.lasso_host_points_from_candidates(self.h, vpt(limbs), vpt(g), n, where, vpt(aff), vpt(status)))
        return aff, status

    def gens_stats(self, reset=False):
        """{"device_candidates": generator candidates this host handed to the device so far, "available": whether the device library has
        lasso_points_from_candidates} (lasso_host_gens_stats)"""
        return self._stats(self.lib.lasso_host_gens_stats, reset, "device_candidates", "available")

    def tables_mle(self, strategy, point, where=0):
        """SubtableStrategy::evaluate_subtable_mle for every subtable of `strategy` (any kind) at `point` = (log_m, 4) uint64: (num_subtables, 4) uint64, fully reduced.
        Built-in kinds and Spark: their closed forms.  A CustomStrategy: where=0 the host loop, where=1 one lasso_tables_mle call on the device (LassoError when the device
        library has no such entry) — lasso_host_tables_mle"""
        lib = self._ext("mle")
        point = np.ascontiguousarray(point, dtype=np.uint64).reshape(-1, 4)
        kind = strategy.desc.base.kind if hasattr(strategy, "desc") else strategy.kind
        c = strategy.c
        n = strategy.num_subtables if hasattr(strategy, "desc") else {_abi.KINDS["lt"]: 2, _abi.KINDS["range"]: 3, _abi.KINDS["spark"]: c}.get(kind, 1)
        out = np.zeros((n, 4), dtype=np.uint64)
        self._chk(lib.lasso_host_tables_mle(self.h, strategy_ptr(strategy), point.ctypes.data_as(C.c_void_p), point.shape[0], where, out.ctypes.data_as(C.c_void_p)))
        return out

    def mle_stats(self, reset=False):
        """{"device_tables": caller-defined tables this host evaluated on the device so far, "available": whether the device library has lasso_tables_mle}
        (lasso_host_mle_stats)"""
        return self._stats(self._ext("mle").lasso_host_mle_stats, reset, "device_tables", "available")

    @staticmethod
    def _values_form(form):
        if form not in ("field", "u64"):
            raise LassoError('lookup values: form is "field" or "u64"')
        return 1 if form == "u64" else 0

    def lookup_values_ref(self, strategy, indices, form="field"):
        """the lookup results v[k] = combine_lookups(T[dim(k)]) of the (n, c) uint64 `indices`, on the CPU (lasso_host_lookup_values_ref: the normative statement):
        s = next_pow2(n) elements — (s, 4) uint64 fully reduced memory words, or (s,) uint64 for form="u64" (LassoError where that form is not offered) — the rows
        behind n being the rows densify pads with (address 0)"""
        lib = self._ext("values")
        indices = np.ascontiguousarray(indices, dtype=np.uint64)
        f = self._values_form(form)
        n = indices.shape[0]
        s = 1 << max((n - 1).bit_length(), 0)
        out = np.zeros((s,) if f else (s, 4), dtype=np.uint64)
        cnt = C.c_size_t()
        self._chk(lib.lasso_host_lookup_values_ref(strategy_ptr(strategy), indices.ctypes.data_as(C.c_void_p), n, f, out.ctypes.data_as(C.c_void_p), s, C.byref(cnt)))
        return out

    def lookup_values(self, dense, strategy, form="field", out=None):
        """the same vector for a densified representation, written by the device from the representation's own address columns (lasso_host_lookup_values).  out=None: a
        numpy array as lookup_values_ref returns it.  `out`: a torch tensor ALREADY ON THE GPU of this host's context — contiguous int64 (reinterpreted as unsigned), shape
        (s,) for form="u64" or (s, 4) for "field", s the representation's padded number of lookups — which receives the vector and is returned."""
        lib = self._ext("values")
        f = self._values_form(form)
        n = C.c_size_t()
        self._chk(lib.lasso_host_dense_len(dense, C.byref(n)))
        s = n.value
        if out is None:
            host = np.zeros((s,) if f else (s, 4), dtype=np.uint64)
            self._chk(lib.lasso_host_lookup_values(self.h, dense, strategy_ptr(strategy), f, 0, host.ctypes.data_as(C.c_void_p)))
            return host
        import torch
        ok = hasattr(out, "data_ptr") and out.is_cuda and out.dtype == torch.int64 and out.is_contiguous() and out.device.index == self.device
        if not ok or tuple(out.shape) != ((s,) if f else (s, 4)) or out.data_ptr() % 16:
            raise LassoError(f"lookup_values: `out` must be a contiguous int64 tensor of shape ({s},) (u64) or ({s}, 4) (field), 16-byte aligned, on GPU {self.device}, the device of this host's context")
        torch.cuda.current_stream(out.device).synchronize()      # nothing of the caller's may still be writing `out`; the call below returns when the vector is complete
        self._chk(lib.lasso_host_lookup_values(self.h, dense, strategy_ptr(strategy), f, 1, C.c_void_p(out.data_ptr())))
        return out

    def values_evaluate(self, values, r):
        """DensePolynomial::evaluate of `values` — (s, 4) uint64 memory words as a numpy array, or an (s, 4) contiguous int64 torch tensor on this host's GPU — at
        r = (log2 s, 4) uint64: (4,) uint64, fully reduced (lasso_host_values_evaluate: one lasso_tables_mle call, no eq table)"""
        lib = self._ext("values")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        out = np.zeros(4, dtype=np.uint64)
        if hasattr(values, "data_ptr") and hasattr(values, "is_cuda"):
            import torch
            if not values.is_cuda or values.dtype != torch.int64 or not values.is_contiguous() or values.dim() != 2 or values.shape[1] != 4 or values.device.index != self.device:
                raise LassoError(f"values_evaluate: a tensor must be contiguous int64 of shape (s, 4) on GPU {self.device}, the device of this host's context")
            torch.cuda.current_stream(values.device).synchronize()
            self._chk(lib.lasso_host_values_evaluate(self.h, C.c_void_p(values.data_ptr()), 1, values.shape[0], r.ctypes.data_as(C.c_void_p), r.shape[0], out.ctypes.data_as(C.c_void_p)))
            return out
        values = np.ascontiguousarray(values, dtype=np.uint64).reshape(-1, 4)
        self._chk(lib.lasso_host_values_evaluate(self.h, values.ctypes.data_as(C.c_void_p), 0, values.shape[0], r.ctypes.data_as(C.c_void_p), r.shape[0], out.ctypes.data_as(C.c_void_p)))
        return out

    def claimed_evaluation(self, proof):
        """claimed_evaluation inside the proof bytes as (4,) uint64 memory words, fully reduced (lasso_host_proof_claimed_evaluation); LassoError on bytes that do not
        deserialize that far"""
        lib = self._ext("values")
        out = np.zeros(4, dtype=np.uint64)
        self._chk(lib.lasso_host_proof_claimed_evaluation(bytes(proof), len(proof), out.ctypes.data_as(C.c_void_p)))
        return out

    def values_stats(self, reset=False):
        """{"device_lookups": elements lasso_lookup_values wrote for this host so far, "available": whether the device library has that entry} (lasso_host_values_stats)"""
        return self._stats(self._ext("values").lasso_host_values_stats, reset, "device_lookups", "available")

    # ---- include/lasso_prover_poly.h: a commitment to the caller's vector and its opening at a point
    def poly_gens(self, num_vars, label=b"gens_poly", points=None):
        """PolyCommitmentGens::new(num_vars, label) (lasso_host_poly_gens_new), or with `points` — an (n + 2, 8) uint64 array [G[0..n), gens_1.G[0], h],
        n = 2^(num_vars - num_vars // 2) — the caller's own generators (lasso_host_poly_gens_from_points).  Release with free(poly_gens=...)."""
        lib = self._ext("poly")
        g = C.c_void_p()
        if points is None:
            self._chk(lib.lasso_host_poly_gens_new(self.h, label, num_vars, C.byref(g)))
        else:
            pts = np.ascontiguousarray(points, dtype=np.uint64).reshape(-1, 8)
            self._chk(lib.lasso_host_poly_gens_from_points(self.h, num_vars, pts.ctypes.data_as(C.c_void_p), pts.shape[0], C.byref(g)))
        return g

    def _poly_values(self, values, form):
        """(pointer, form, on_device, s, what must stay alive): numpy arrays ((s,) uint64 = "u64", (s, 4) uint64 = "field"), torch tensors ALREADY ON THE GPU of this
        host's context (contiguous int64 of those shapes, reinterpreted as unsigned, 16-byte aligned), or a DeviceVector"""
        if isinstance(values, DeviceVector):
            if values.host is not self or not values.ptr:
                raise LassoError("poly: the DeviceVector belongs to another host, or was freed")
            return C.c_void_p(values.ptr), self._values_form(values.form), 1, values.s, values
        if hasattr(values, "data_ptr") and hasattr(values, "is_cuda"):
            import torch
            f = self._values_form(form or ("u64" if values.dim() == 1 else "field"))
            ok = values.is_cuda and values.dtype == torch.int64 and values.is_contiguous() and values.device.index == self.device
            if not ok or (values.dim() != 1 if f else (values.dim() != 2 or values.shape[1] != 4)) or values.data_ptr() % 16:
                raise LassoError(f"poly: a tensor must be contiguous int64 of shape (s,) (u64) or (s, 4) (field), 16-byte aligned, on GPU {self.device}, the device of this host's context")
            torch.cuda.current_stream(values.device).synchronize()
            return C.c_void_p(values.data_ptr()), f, 1, values.shape[0], values
        a = np.ascontiguousarray(values, dtype=np.uint64)
        f = self._values_form(form or ("u64" if a.ndim == 1 else "field"))
        if (a.ndim != 1) if f else (a.ndim != 2 or a.shape[1] != 4):
            raise LassoError("poly: an array has shape (s,) (u64) or (s, 4) (field)")
        return a.ctypes.data_as(C.c_void_p), f, 0, a.shape[0], a

    def poly_commit(self, pgens, values, form=None, tape=None):
        """DensePolynomial::commit of `values` (see _poly_values for what they may be) over `pgens`: the bytes [u64 L][L x 32 B] (lasso_host_poly_commit).  The 64-bit
        form is read as it is on the device where the device library has include/lasso_hip_poly.h.  With `tape` (a live tape pair): the hiding form, commit(gens,
        Some(tape)) — (commitment, the row blinds drawn from the tape as (L, 4) uint64 memory words) (lasso_host_poly_commit_blinded)"""
        lib = self._ext("poly")
        ptr, f, on_dev, s, keep = self._poly_values(values, form)
        if tape is None:
            return self._bytes_call(lib.lasso_host_poly_commit, self.h, pgens, ptr, f, on_dev, s)
        blinds = np.zeros((1 << ((s.bit_length() - 1) // 2) if s else 1, 4), dtype=np.uint64)
        c = self._bytes_call(self._ext("blind").lasso_host_poly_commit_blinded, self.h, pgens, ptr, f, on_dev, s, tape[0], tape[1], blinds.ctypes.data_as(C.c_void_p))
        return c, blinds

    def poly_commitment_append(self, transcript, label, commitment):
        """PolyCommitment::append_to_transcript(label) against a live transcript (a (vtbl, user) pair as Transcript.pair() makes it)"""
        self._chk(self._ext("poly").lasso_host_poly_commitment_append(transcript[0], transcript[1], label, bytes(commitment), len(commitment)))

    @staticmethod
    def _blinds_arg(blinds, rows=None):
        """row blinds / one blind as the C calls take them: (pointer or None, what must stay alive)"""
        if blinds is None:
            return None, None
        a = np.ascontiguousarray(blinds, dtype=np.uint64).reshape(-1, 4)
        if rows is not None and a.shape[0] != rows:
            raise LassoError(f"blinds: {rows} row blinds of 4 words each are needed, got {a.shape[0]}")
        return a.ctypes.data_as(C.c_void_p), a

    def poly_open(self, pgens, values, r, transcript, tape, form=None, blinds=None, blind_Zr=None, committed=False):
        """PolyEvalProof::prove of `values` at r = (num_vars, 4) uint64 against live transcript and tape pairs: (proof bytes, Zr as (4,) uint64 memory words, fully
        reduced) — Zr = the polynomial's evaluation at r, computed on the way (lasso_host_poly_open).  With `blinds` (the row blinds poly_commit returned), `blind_Zr`
        ((4,) uint64) or committed=True: (proof, Zr, C_Zr) — C_Zr = Zr * G_1 + blind_Zr * h as 32 wire bytes, what poly_verify_committed takes
        (lasso_host_poly_open_blinded; a keyword left out is None: zero)"""
        lib = self._ext("poly")
        ptr, f, on_dev, s, keep = self._poly_values(values, form)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        zr = np.zeros(4, dtype=np.uint64)
        if blinds is not None or blind_Zr is not None or committed:
            bl, keep_b = self._blinds_arg(blinds, 1 << ((s.bit_length() - 1) // 2) if s else None)
            bz, keep_z = self._blinds_arg(blind_Zr, 1)
            c_zr = (C.c_uint8 * 32)()
            proof = self._bytes_call(lambda *a: self._ext("blind").lasso_host_poly_open_blinded(self.h, pgens, ptr, f, on_dev, s, r.ctypes.data_as(C.c_void_p), r.shape[0], bl, bz, transcript[0],
                                                                                                 transcript[1], tape[0], tape[1], zr.ctypes.data_as(C.c_void_p), c_zr, *a))
            return proof, zr, bytes(c_zr)
        proof = self._bytes_call(lambda *a: lib.lasso_host_poly_open(self.h, pgens, ptr, f, on_dev, s, r.ctypes.data_as(C.c_void_p), r.shape[0], transcript[0], transcript[1], tape[0], tape[1],
                                                                      zr.ctypes.data_as(C.c_void_p), *a))
        return proof, zr

    def poly_verify(self, pgens, r, zr, proof, commitment, transcript):
        """PolyEvalProof::verify_plain over the wire bytes against a live transcript pair: True = Ok(()), False = Err; LassoError on bytes that do not deserialize
        (lasso_host_poly_verify)"""
        lib = self._ext("poly")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        zr = np.ascontiguousarray(zr, dtype=np.uint64).reshape(4)
        ok = C.c_int32(-1)
        self._chk(lib.lasso_host_poly_verify(self.h, pgens, r.ctypes.data_as(C.c_void_p), r.shape[0], zr.ctypes.data_as(C.c_void_p), transcript[0], transcript[1],
                                             bytes(proof), len(proof), bytes(commitment), len(commitment), C.byref(ok)))
        return ok.value == 1

    def poly_verify_committed(self, pgens, r, c_zr, proof, commitment, transcript):
        """PolyEvalProof::verify: as poly_verify, the evaluation given as its commitment C_Zr (32 wire bytes, poly_open's third result) (lasso_host_poly_verify_committed)"""
        lib = self._ext("blind")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        if len(c_zr) != 32:
            raise LassoError("poly_verify_committed: C_Zr is 32 bytes")
        ok = C.c_int32(-1)
        self._chk(lib.lasso_host_poly_verify_committed(self.h, pgens, r.ctypes.data_as(C.c_void_p), r.shape[0], bytes(c_zr), transcript[0], transcript[1],
                                                       bytes(proof), len(proof), bytes(commitment), len(commitment), C.byref(ok)))
        return ok.value == 1

    def blind_stats(self, reset=False):
        """{"rows_device": rows this host blinded on the device (lasso_points_reduce_compress), "rows_host": rows blinded on the host (the decode route, a merge's zero
        blocks)} (lasso_host_blind_stats)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._ext("blind").lasso_host_blind_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return {"rows_device": a.value, "rows_host": b.value}

    def values_vector(self, dense, strategy):
        """the lookup results of `dense` left ON THE DEVICE as a DeviceVector: 64-bit integers where lasso_lookup_values offers that form, field elements otherwise"""
        lib = self._ext("poly"); self._ext("values")
        n = C.c_size_t()
        self._chk(lib.lasso_host_dense_len(dense, C.byref(n)))
        for form in ("u64", "field"):
            vec = DeviceVector(self, form, n.value)
            try:
                self._chk(lib.lasso_host_lookup_values(self.h, dense, strategy_ptr(strategy), self._values_form(form), 1, C.c_void_p(vec.ptr)))
                return vec
            except LassoError as e:
                vec.free()
                if form == "field" or "64-bit form" not in str(e):
                    raise

    def values_commit(self, dense, strategy, pgens, tape=None):
        """(commitment bytes, DeviceVector): the lookup results of `dense` written by the device (values_vector), never downloaded, and their commitment over `pgens`;
        pass the vector on to poly_open and free() it afterwards.  With `tape`: the hiding commitment, (commitment, DeviceVector, row blinds) (see poly_commit)"""
        vec = self.values_vector(dense, strategy)
        try:
            if tape is not None:
                c, blinds = self.poly_commit(pgens, vec, tape=tape)
                return c, vec, blinds
            return self.poly_commit(pgens, vec), vec
        except Exception:
            vec.free()
            raise

    def poly_stats(self, reset=False):
        """{"u64_commit_elements", "u64_open_elements": 64-bit elements this host committed to / opened through the device entries of include/lasso_hip_poly.h so far,
        "available": whether the device library has them} (lasso_host_poly_stats)"""
        return self._stats(self._ext("poly").lasso_host_poly_stats, reset, "u64_commit_elements", "u64_open_elements", "available")

    # ---- include/lasso_prover_polys.h: several vectors under one commitment, opened at r in one proof
    def _polys_vecs(self, vectors, s):
        """(lasso_host_poly_vec array, k, s, what must stay alive).  A vector is whatever _poly_values takes — a (s,) uint64 array ("u64"), a (s, 4) uint64 array
        ("field"), a tensor on this host's GPU, a DeviceVector — or a pair (device pointer, "u64" / "field"): s elements of that form in device memory of this host's
        context, 16-byte aligned.  All have the same length; `s` is needed only where every vector is such a pair."""
        vectors = list(vectors)
        arr, keep, lens = (_abi.PolyVec * max(len(vectors), 1))(), [], set() if s is None else {int(s)}
        for i, v in enumerate(vectors):
            if isinstance(v, tuple) and len(v) == 2 and isinstance(v[1], str):
                arr[i] = _abi.PolyVec(C.c_void_p(int(v[0])), self._values_form(v[1]), 1)
                continue
            ptr, f, on_dev, n, alive = self._poly_values(v, None)
            arr[i] = _abi.PolyVec(ptr, f, on_dev); keep.append(alive); lens.add(n)
        if len(lens) > 1:
            raise LassoError(f"polys: the vectors must have one length, got {sorted(lens)}")
        if not lens and vectors:
            raise LassoError("polys: `s` is needed where every vector is a (device pointer, form) pair")
        return arr, len(vectors), (lens.pop() if lens else 0), keep

    @staticmethod
    def _polys_rows(k, s):
        """rows of the merged matrix of k vectors of s values: 2^((log2 s + kappa) / 2)"""
        return 1 << (((max(s, 1).bit_length() - 1) + (max(k, 1) - 1).bit_length()) // 2)

    def polys_commit(self, pgens, vectors, s=None, tape=None):
        """DensePolynomial::merge(vectors).commit over `pgens` — a poly_gens for log2(s) + log2(next_pow2(k)) variables: the bytes [u64 L'][L' x 32 B]
        (lasso_host_polys_commit; see _polys_vecs for what a vector may be).  The merge is never made: every vector is read where it lies.  With `tape` (a live tape
        pair): the hiding form, (commitment, the L' row blinds of one draw as (L', 4) uint64) — every row blinded, the zero blocks' too (lasso_host_polys_commit_blinded)"""
        lib = self._ext("polys")
        arr, k, s, keep = self._polys_vecs(vectors, s)
        if tape is None:
            return self._bytes_call(lib.lasso_host_polys_commit, self.h, pgens, arr, k, s)
        blinds = np.zeros((self._polys_rows(k, s), 4), dtype=np.uint64)
        c = self._bytes_call(self._ext("blind").lasso_host_polys_commit_blinded, self.h, pgens, arr, k, s, tape[0], tape[1], blinds.ctypes.data_as(C.c_void_p))
        return c, blinds

    def polys_open(self, pgens, vectors, r, transcript, tape, s=None, blinds=None):
        """CombinedTableEvalProof::prove of the merged `vectors` at r = (log2 s, 4) uint64 against live transcript and tape pairs: (proof bytes, evals as (k, 4) uint64
        memory words, fully reduced), evals[b] = MLE(vectors[b])(r) (lasso_host_polys_open).  `blinds`: the row blinds polys_commit returned with a tape
        (lasso_host_polys_open_blinded); the evaluations stay in the clear and polys_verify takes the opening as it stands"""
        lib = self._ext("polys")
        arr, k, s, keep = self._polys_vecs(vectors, s)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        evals = np.zeros((max(k, 1), 4), dtype=np.uint64)
        if blinds is not None:
            bl, keep_b = self._blinds_arg(blinds, self._polys_rows(k, s))
            proof = self._bytes_call(lambda *a: self._ext("blind").lasso_host_polys_open_blinded(self.h, pgens, arr, k, s, r.ctypes.data_as(C.c_void_p), r.shape[0], bl, transcript[0], transcript[1],
                                                                                                  tape[0], tape[1], evals.ctypes.data_as(C.c_void_p), *a))
            return proof, evals[:k]
        proof = self._bytes_call(lambda *a: lib.lasso_host_polys_open(self.h, pgens, arr, k, s, r.ctypes.data_as(C.c_void_p), r.shape[0], transcript[0], transcript[1], tape[0], tape[1],
                                                                       evals.ctypes.data_as(C.c_void_p), *a))
        return proof, evals[:k]

    def polys_verify(self, pgens, r, evals, proof, commitment, transcript):
        """CombinedTableEvalProof::verify over the wire bytes against a live transcript pair; evals = (k, 4) uint64: True = Ok(()), False = Err; LassoError on bytes
        that do not deserialize (lasso_host_polys_verify)"""
        lib = self._ext("polys")
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        evals = np.ascontiguousarray(evals, dtype=np.uint64).reshape(-1, 4)
        ok = C.c_int32(-1)
        self._chk(lib.lasso_host_polys_verify(self.h, pgens, r.ctypes.data_as(C.c_void_p), r.shape[0], evals.ctypes.data_as(C.c_void_p), evals.shape[0], transcript[0], transcript[1],
                                              bytes(proof), len(proof), bytes(commitment), len(commitment), C.byref(ok)))
        return ok.value == 1

    def polys_evaluate(self, vectors, r, s=None):
        """evals[b] = MLE(vectors[b])(r) as (k, 4) uint64, by the opening's own pass over the vectors, without generators or transcript (lasso_host_polys_evaluate):
        what a verifier computes of the public columns"""
        lib = self._ext("polys")
        arr, k, s, keep = self._polys_vecs(vectors, s)
        r = np.ascontiguousarray(r, dtype=np.uint64).reshape(-1, 4)
        evals = np.zeros((max(k, 1), 4), dtype=np.uint64)
        self._chk(lib.lasso_host_polys_evaluate(self.h, arr, k, s, r.ctypes.data_as(C.c_void_p), r.shape[0], evals.ctypes.data_as(C.c_void_p)))
        return evals[:k]

    def polys_stats(self, reset=False):
        """{"vectors_committed", "vectors_opened"}: vectors this host took through polys_commit / polys_open so far (lasso_host_polys_stats)"""
        a, b = C.c_uint64(), C.c_uint64()
        self._chk(self._ext("polys").lasso_host_polys_stats(self.h, C.byref(a), C.byref(b), 1 if reset else 0))
        return {"vectors_committed": a.value, "vectors_opened": b.value}

    def strategy_check(self, strategy):
        """validate a strategy descriptor without proving (lasso_host_strategy_check): raises LassoError with the reason"""
        self._chk(self.lib.lasso_host_strategy_check(strategy_ptr(strategy)))

    def debug_cubic_batched(self, dense, gens, strategy, A, B, rand, coeffs, claim, transcript=b"test"):
        """test support: prove_cubic_batched on caller arrays with a scripted eq point (lasso_host_debug_cubic_batched)"""
        A = np.ascontiguousarray(A, dtype=np.uint64); B = np.ascontiguousarray(B, dtype=np.uint64)     # (k, 2^ell, 4)
        k, n = A.shape[0], A.shape[1]; ell = n.bit_length() - 1
        rand = np.ascontiguousarray(rand, dtype=np.uint64).reshape(-1, 4); coeffs = np.ascontiguousarray(coeffs, dtype=np.uint64).reshape(-1, 4)
        claim = np.ascontiguousarray(claim, dtype=np.uint64).reshape(4)
        assert rand.shape[0] == ell and coeffs.shape[0] == k and B.shape == A.shape
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        return self._bytes_call(self.lib.lasso_host_debug_cubic_batched, self.h, dense, gens, strategy_ptr(strategy), k, ell, vp(A), vp(B), vp(rand), vp(coeffs), vp(claim), transcript)

    def free(self, dense=None, gens=None, poly_gens=None):
        if dense:
            self.lib.lasso_host_dense_free(dense)
        if gens:
            self.lib.lasso_host_gens_free(gens)
        if poly_gens:
            self._ext("poly").lasso_host_poly_gens_free(poly_gens)

    def close(self):
        if self.h:
            self.lib.lasso_host_destroy(self.h)
            self.h = None

    def ctx(self):
        return self.lib.lasso_host_ctx(self.h)

    def mem_stats(self, reset=False):
        """device bytes held by this host now / at most, and the most the prover itself had in use (lasso_host_mem_stats)"""
        live, peak, used = C.c_uint64(), C.c_uint64(), C.c_uint64()
        self._chk(self.lib.lasso_host_mem_stats(self.h, C.byref(live), C.byref(peak), C.byref(used), 1 if reset else 0))
        return {"live_bytes": live.value, "peak_bytes": peak.value, "prover_peak_bytes": used.value}

    def set_throughput_mode(self, on=True):
        """this host is one of several proving concurrently on the GPU: no kernel of it waits on the device for its host thread (lasso_host_set_throughput_mode)"""
        self._chk(self.lib.lasso_host_set_throughput_mode(self.h, 1 if on else 0))

    def set_capacity(self, on=True):
        """capacity mode (lasso_host_set_capacity): large buffers go back to the driver on release; the per-rank high-water mark is the live peak"""
        self._chk(self.lib.lasso_host_set_capacity(self.h, 1 if on else 0))


class DeviceVector:
    """s elements in device memory of a HostProver's context ("u64": 8 bytes each, "field": 32), allocated here and released by free(): what
    HostProver.values_vector returns and poly_commit / poly_open take without a download"""

    def __init__(self, host, form, s):
        lib = host._ext("poly")
        lib.lasso_alloc.argtypes = [C.c_void_p, C.c_size_t, C.POINTER(C.c_void_p)]       # the device library's, reached through the prover library that is linked against it
        lib.lasso_free.argtypes = [C.c_void_p, C.c_void_p]
        p = C.c_void_p()
        if lib.lasso_alloc(C.c_void_p(host.ctx()), s * (8 if form == "u64" else 32), C.byref(p)) != 0:
            raise LassoError("DeviceVector: lasso_alloc failed")
        self.host, self.form, self.s, self.ptr = host, form, s, p.value

    def free(self):
        if self.ptr:
            self.host.lib.lasso_free(C.c_void_p(self.host.ctx()), C.c_void_p(self.ptr)); self.ptr = None


class Transcript:
    """The library's own Merlin transcript as an object that lives across calls (lasso_host_merlin_new / lasso_host_random_tape_new): `pair()` is what
    HostProver.prove_with / verify_with take.  tape=True builds RandomTape::new(label) (utils/random.rs:15-31) instead of Transcript::new(label)."""

    def __init__(self, lib, label, tape=False):
        self.lib = lib
        self.m = (lib.lasso_host_random_tape_new if tape else lib.lasso_host_merlin_new)(label)
        if not self.m:
            raise LassoError("lasso_host_merlin_new failed")
        self.vt = lib.lasso_host_merlin_vtbl()

    def append_message(self, label, msg):
        lb = (C.c_uint8 * len(label)).from_buffer_copy(label); mb = (C.c_uint8 * max(len(msg), 1)).from_buffer_copy(msg or b"\0")
        self.vt.contents.append_message(self.m, lb, len(label), mb, len(msg))

    def challenge_bytes(self, label, n):
        lb = (C.c_uint8 * len(label)).from_buffer_copy(label); out = (C.c_uint8 * n)()
        self.vt.contents.challenge_bytes(self.m, lb, len(label), out, n)
        return bytes(out)

    def pair(self):
        return (self.vt, C.c_void_p(self.m))

    def close(self):
        if self.m:
            self.lib.lasso_host_merlin_free(self.m); self.m = None
