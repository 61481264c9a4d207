"""Caller-defined subtable strategies: the reference's `SubtableStrategy` trait (src/subtables/mod.rs:31-93) as data.

    materialize_subtables      -> `tables`: one array per subtable, 2^log_m entries each
    evaluate_subtable_mle      -> nothing to write: the verifier evaluates the table's MLE itself
    combine_lookups            -> `terms`: g(v) = sum of coeff * product of v[memory] over each term's memory list
    g_poly_degree              -> the longest term
    memory_to_subtable_index / memory_to_dimension_index -> `memory_subtable` / `memory_dimension` (default: i % num_subtables, i // num_subtables)

The object owns every array the C descriptor points to and is accepted wherever an `_abi.Strategy` is (HostProver.prove / prove_with / verify / verify_with,
and — through `.ptr()` — lasso_sumcheck_combine_round / lasso_combine_claim of the device library)."""
import ctypes as C

import numpy as np

from . import _abi

FR_MODULUS = {
    "curve25519": 2**252 + 27742317777372353535851937790883648493,
    "bn254": 21888242871839275222246405745257275088548364400416034343698204186575808495617,
}


def fr_words(values, curve="curve25519"):
    """field elements (Python ints, any sign) -> (n, 4) uint64 memory words (lasso_fr: value * 2^256 mod p, little-endian limbs)"""
    p = FR_MODULUS[curve]
    out = np.empty((len(values), 4), dtype=np.uint64)
    for i, v in enumerate(values):
        w = (int(v) % p) * (1 << 256) % p
        out[i] = [(w >> (64 * k)) & (2**64 - 1) for k in range(4)]
    return out


class CustomStrategy:
    def __init__(self, c, log_m, tables, terms, num_memories=None, memory_subtable=None, memory_dimension=None, curve="curve25519"):
        """tables: all 1-D integer arrays (values < 2^32: the integer shortcuts of the built-in strategies apply) or all (2^log_m, 4) uint64 arrays of memory
        words (fr_words).  terms: [(coeff, [memory, ...]), ...] with integer coefficients taken mod p (-1 is p - 1); a memory may repeat; [] is a constant."""
        tables = [np.asarray(t) for t in tables]
        if not tables:
            raise ValueError("a strategy needs at least one subtable")
        field = tables[0].ndim == 2
        if any((t.ndim == 2) != field for t in tables):
            raise ValueError("all tables of one strategy use the same form (integers or field elements)")
        m = 1 << log_m
        if field:
            self.tables = [np.ascontiguousarray(t, dtype=np.uint64) for t in tables]
            if any(t.shape != (m, 4) for t in self.tables):
                raise ValueError("a field-element table is a (2^log_m, 4) uint64 array")
        else:
            if any(t.shape != (m,) for t in tables) or any(t.size and (int(t.min()) < 0 or int(t.max()) >= 2**32) for t in tables):
                raise ValueError("an integer table has 2^log_m entries in [0, 2^32)")
            self.tables = [np.ascontiguousarray(t, dtype=np.uint32) for t in tables]
        self.curve, self.c, self.log_m, self.field = curve, c, log_m, field
        self.num_subtables = len(self.tables)
        self.num_memories = int(num_memories) if num_memories is not None else c * self.num_subtables
        self.terms = [(int(cf) % FR_MODULUS[curve], [int(x) for x in mems]) for cf, mems in terms]
        self._ptrs = (C.c_void_p * self.num_subtables)(*[t.ctypes.data for t in self.tables])
        self._coeff = fr_words([cf for cf, _ in self.terms], curve)
        starts = [0]
        for _, mems in self.terms:
            starts.append(starts[-1] + len(mems))
        self._start = np.array(starts, dtype=np.uint32)
        self._mem = np.array([x for _, mems in self.terms for x in mems] or [0], dtype=np.uint32)
        if (memory_subtable is None) != (memory_dimension is None):
            raise ValueError("memory_subtable and memory_dimension are given together")
        self._msub = None if memory_subtable is None else np.ascontiguousarray(memory_subtable, dtype=np.uint32)
        self._mdim = None if memory_dimension is None else np.ascontiguousarray(memory_dimension, dtype=np.uint32)
        if self._msub is not None and (len(self._msub) != self.num_memories or len(self._mdim) != self.num_memories):
            raise ValueError("the memory maps have one entry per memory")
        d = _abi.StrategyCustom()
        d.base = _abi.Strategy(_abi.KINDS["custom"], c, log_m, 0)
        d.num_subtables, d.num_memories = self.num_subtables, self.num_memories
        d.tables_u32 = None if field else C.cast(self._ptrs, C.POINTER(C.c_void_p))
        d.tables_fr = C.cast(self._ptrs, C.POINTER(C.c_void_p)) if field else None
        d.memory_subtable = None if self._msub is None else self._msub.ctypes.data
        d.memory_dimension = None if self._mdim is None else self._mdim.ctypes.data
        d.num_terms, d.reserved = len(self.terms), 0
        d.coeff, d.term_start, d.term_mem = self._coeff.ctypes.data, self._start.ctypes.data, self._mem.ctypes.data
        self.desc = d

    @property
    def degree(self):
        """sumcheck_poly_degree(): the longest term + 1"""
        return max(len(mems) for _, mems in self.terms) + 1

    @property
    def linear(self):
        return all(len(mems) == 1 for _, mems in self.terms)

    def memory_map(self, i):
        """(subtable, dimension) of memory i"""
        if self._msub is not None:
            return int(self._msub[i]), int(self._mdim[i])
        return i % self.num_subtables, i // self.num_subtables

    def ptr(self):
        """the `const lasso_strategy*` every entry point takes: a pointer to the descriptor's first member"""
        return C.cast(C.pointer(self.desc), C.POINTER(_abi.Strategy))


def strategy_ptr(strategy):
    """an `_abi.Strategy` or a CustomStrategy -> what the C ABI's `const lasso_strategy*` parameters take"""
    return strategy.ptr() if isinstance(strategy, CustomStrategy) else C.byref(strategy)
