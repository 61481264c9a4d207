"""Guard-band harness for the device ABI: every buffer a test hands to a `lasso_*` call lives inside ONE device allocation that is filled with a position-dependent pattern,
so that "what else did the call touch" becomes a question the host can answer by reading memory back.

  ArenaDevice(Device)   one lasso_alloc of ARENA_BYTES; alloc() is a bump allocation at deliberately poor alignment with patterned gaps of at least MIN_GAP bytes between
                        buffers; upload() writes through to a host shadow of the arena; free() only marks a buffer dead (nothing is reused within a case).
  LibProxy              what the device is created with and what `d.lib` returns.  Every `lasso_*` call is normalised to plain Python values, tests/writecontract.py is asked for
                        the byte ranges that call may write, and those join the case's allowed set.  A call without a contract entry fails the case.
  audit()               (context idle) downloads the used extent plus AUDIT_TAIL bytes and requires equality with the shadow everywhere outside the allowed set.

The same classes run over the oracle's mock, whose device memory is host memory (tests/test_write_contract_cpu.py).

The library's own scratch, sort and big-result buffers are held by the library itself: under LASSO_SCRATCH_GUARD=1 (lasso_amd/csrc/device_switches.cuh) each request has a guard of
64 KiB directly behind its requested size and lasso_sync reports a damaged one, which is why a case ends with sync() before audit().

What those buffers and every other allocation of the library hold BEFORE a call is varied by LASSO_POISON=1 (the same table): each new allocation — scratch, sort and
big-result buffers, generator tables, term lists, mapped result buffers, lasso_alloc — starts as the 32-bit word 0x00000001 repeated, and the first request a public call makes
of one of the three buffers fills its requested range with the word in stream order.  A kernel that reads a partial, a bucket or a table entry this call did not store then
computes with the word, not with zeros or with what an identical call left there, and the case's own parity assertion fails.

NOT covered: stray WRITES into the generator tables, the mapped result buffers and every other allocation the library owns outside those three buffers; stray READS that do not
change a result (of the word, or of caller memory); a stray write that happens to store the pattern's own bytes at that position; the collectives of slab mode."""
import ctypes as C

import numpy as np

from lasso_amd import Device
from lasso_amd.device import LassoError
import writecontract

ARENA_BYTES = 640 << 20     # sized for the largest cases: test_cubic_round_launched_ahead at n = 2^20 and test_layer_enqueued_ahead_of_its_point at 2^18 x 9 circuits run twice over
                            # the arena (nothing is reused within a case), about 300 MiB each
AUDIT_TAIL = 1 << 20        # bytes audited beyond the last buffer of a case
MIN_GAP = 4096 + 64         # smallest distance between two buffers (gap k is 4096 + 64 * (1 + 37 k mod 61) bytes, then rounded up to the next offset of the wanted residue)
# the switch settings under which the tables' rows run once more (tests/arena_cases.py test_tab_row, one child process each in tests/test_gpu_write_contract.py): those that move
# partials, result areas and scratch layouts
SETTINGS = [{}, {"LASSO_CUBIC_WIDE": "0"}, {"LASSO_DIRECT_NX": "64"}, {"LASSO_CUBIC_NX": "17"}, {"LASSO_REDUCE_NX": "3"}, {"LASSO_MSM_DIRECT": "0"}, {"LASSO_MSM_FULL8": "1"},
            {"LASSO_MSM_ROWS8W_WAVES": "400"}, {"LASSO_MSM_PIP_MIN_COLS": "32", "LASSO_MSM_PIP_SCRATCH_MB": "16"}, {"LASSO_TAGGED_RESULTS": "0"}]
_BYREF = type(C.byref(C.c_int()))
_MUL = np.uint64(0x9E3779B97F4A7C15)
_ADD = np.uint64(0xD1B54A32D192ED03)

# interior offsets are no more aligned than the element type needs: (residue, modulus) of the ADDRESS
ALIGN = {"fr": (32, 64),     # field elements, points, raw alloc(): fr_t / fq_t are alignas(16) structs and nothing in lasso_amd/csrc reads caller memory through a wider type
         "u32": (4, 16),
         "u64": (8, 16)}


def pattern(word0, nwords):
    """the arena's fill: 64-bit word i (arena-relative) holds i * odd + odd mod 2^64, so a run copied from anywhere else in the arena differs from what belongs there"""
    with np.errstate(over="ignore"):
        return np.arange(word0, word0 + nwords, dtype=np.uint64) * _MUL + _ADD


def kind_of(arr):
    """the alignment rule of an upload: 32-bit integers, 1-D / index 64-bit integers (operand columns, lookup indices), everything else as field elements"""
    if arr.dtype == np.uint32:
        return "u32"
    if arr.dtype == np.uint64 and not (arr.ndim == 2 and arr.shape[1] in (4, 8, 16)):
        return "u64"
    return "fr"


class WriteViolation(AssertionError):
    pass


class _Buf:
    __slots__ = ("idx", "lo", "hi", "kind", "live", "died_at")

    def __init__(self, idx, lo, hi, kind):
        self.idx, self.lo, self.hi, self.kind, self.live, self.died_at = idx, lo, hi, kind, True, None

    def __repr__(self):
        return f"buffer #{self.idx} ({self.kind}, arena [{self.lo:#x}, {self.hi:#x}), {self.hi - self.lo} bytes, {'live' if self.live else 'freed after call %d' % self.died_at})"


def _norm(arg):
    """one raw ctypes argument -> int (addresses, integers), list of int (pointer tables) or the object itself (structs by reference)"""
    if arg is None:
        return 0
    if isinstance(arg, (int, np.integer)):
        return int(arg)
    if isinstance(arg, C.c_void_p):
        return arg.value or 0
    if isinstance(arg, C.Array):
        if arg._type_ is C.c_void_p:
            return [v or 0 for v in arg]
        return arg
    if isinstance(arg, C._SimpleCData):
        return arg.value
    if isinstance(arg, _BYREF):        # byref(x): the object behind it
        return _norm(arg._obj) if isinstance(arg._obj, C.c_void_p) else arg._obj
    if isinstance(arg, C._Pointer):
        return arg.contents if arg else 0
    return arg


class LibProxy:
    """the device library behind a recorder: attribute access returns the library's own function for anything that is not `lasso_*`"""

    def __init__(self, raw, contract=None):
        self._raw = raw
        self._contract = writecontract.CONTRACT if contract is None else contract
        self._arena = None
        self._fns = {}

    def __getattr__(self, name):
        fn = getattr(self._raw, name)
        if not name.startswith("lasso_"):
            return fn
        w = self._fns.get(name)
        if w is None:
            w = self._fns[name] = self._wrap(name, fn)
        return w

    def _wrap(self, name, fn):
        return _Recorded(self, name, fn)


class _Recorded:
    """one `lasso_*` function behind the recorder.  Prototypes set on it (lasso_amd._abi.declare_* assign restype / argtypes to what `lib.name` returns) reach the library's own
    function: without them ctypes would pass every integer as a C int"""

    def __init__(self, proxy, name, fn):
        object.__setattr__(self, "_proxy", proxy); object.__setattr__(self, "_name", name); object.__setattr__(self, "_fn", fn)

    def __setattr__(self, key, value):
        setattr(self._fn, key, value)

    def __getattr__(self, key):
        return getattr(self._fn, key)

    def __call__(self, *args):
        proxy, name = self._proxy, self._name
        entry = proxy._contract.get(name)
        if entry is None:
            raise WriteViolation(f"no write contract for {name}")
        a = [_norm(x) for x in args]
        arena = proxy._arena
        ranges = [(int(p), int(nb)) for p, nb in entry(a, proxy._raw) if p and nb > 0]
        if arena is not None:
            arena._record(name, a, ranges)
        rc = self._fn(*args)
        if arena is not None and name == "lasso_upload" and rc == 0:
            arena._shadow_upload(a[1], args[2], a[3])
        return rc


class ArenaDevice(Device):
    def __init__(self, device=0, lib=None, curve="curve25519", contract=None):
        from lasso_amd import load_device_library
        raw = lib if lib is not None else load_device_library(curve=curve)
        proxy = LibProxy(raw, contract)
        super().__init__(device, lib=proxy, curve=curve)
        self.raw = raw
        p = C.c_void_p()
        rc = raw.lasso_alloc(self.ctx, ARENA_BYTES, C.byref(p))
        if rc != 0:
            raise LassoError(f"the arena's lasso_alloc of {ARENA_BYTES} bytes failed ({rc})")
        self.base = p.value
        self.shadow = pattern(0, ARENA_BYTES // 8)
        self._raw_upload(0, self.shadow)
        self.used = 0
        self.bufs = []
        self.calls = []
        self.allowed = []          # (lo, hi, call number) arena-relative
        self.problems = []         # contract ranges that do not lie in one live buffer
        self.max_used = 0
        proxy._arena = self

    def close(self):
        if getattr(self, "ctx", None) and getattr(self, "base", None):
            self.raw.lasso_free(self.ctx, C.c_void_p(self.base))
            self.base = None
        super().close()

    # ---- raw transfers that the recorder does not see
    def _raw_upload(self, off, arr):
        arr = np.ascontiguousarray(arr)
        if arr.nbytes:
            rc = self.raw.lasso_upload(self.ctx, C.c_void_p(self.base + off), arr.ctypes.data_as(C.c_void_p), arr.nbytes)
            assert rc == 0, f"arena upload failed ({rc}): {self.raw.lasso_last_error(self.ctx).decode()}"

    def _raw_download(self, off, nbytes):
        out = np.empty(nbytes, dtype=np.uint8)
        rc = self.raw.lasso_download(self.ctx, out.ctypes.data_as(C.c_void_p), C.c_void_p(self.base + off), nbytes)
        assert rc == 0, f"arena download failed ({rc}): {self.raw.lasso_last_error(self.ctx).decode()}"
        return out

    # ---- memory (Device's interface)
    def alloc(self, nbytes, kind="fr"):
        """bump allocation; the bytes handed out still hold the pattern (the arena is patterned once and reset() re-patterns whatever a case used), so no transfer is made here —
        an allocation is legal wherever the library's own lasso_alloc is, also while a launch waits on the device"""
        res, mod = ALIGN[kind]
        k = len(self.bufs)
        lo = self.used + 4096 + 64 * (1 + 37 * k % 61)
        lo += (res - (self.base + lo)) % mod
        hi = lo + max(int(nbytes), 1)
        if hi + AUDIT_TAIL > ARENA_BYTES:
            raise LassoError(f"the arena of {ARENA_BYTES} bytes is too small for this case (wanted up to {hi + AUDIT_TAIL}): raise tests/arenautil.py ARENA_BYTES")
        self.bufs.append(_Buf(k, lo, hi, kind))
        self.used = hi
        self.max_used = max(self.max_used, hi)
        return self.base + lo

    def free(self, ptr):
        b = self._owner(ptr - self.base)
        assert isinstance(b, _Buf) and b.lo == ptr - self.base and b.live, f"free of {ptr:#x}: not the base of a live arena buffer"
        b.live, b.died_at = False, len(self.calls)

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.alloc(arr.nbytes, kind_of(arr))
        if arr.nbytes:
            self._chk(self.lib.lasso_upload(self.ctx, C.c_void_p(p), arr.ctypes.data_as(C.c_void_p), arr.nbytes))
        return p

    def materialize_subtable_u32(self, strategy, sub):
        from lasso_amd.custom import strategy_ptr
        m = 1 << strategy.log_m
        p = self.alloc(4 * m, "u32")
        self._chk(self.lib.lasso_materialize_subtable_u32(self.ctx, strategy_ptr(strategy), sub, C.c_void_p(p)))
        out = self.download(p, (m,), dtype=np.uint32)
        self.free(p)
        return out

    # ---- the recorder's side
    def _owner(self, off):
        """the buffer that holds arena offset `off`, or the pair of buffers around the gap it lies in"""
        prev = None
        for b in self.bufs:
            if b.lo <= off < b.hi:
                return b
            if off < b.lo:
                return (prev, b)
            prev = b
        return (prev, None)

    def _describe(self, off):
        o = self._owner(off)
        if isinstance(o, _Buf):
            return f"{o}, {off - o.lo} bytes from its start, {o.hi - off} before its end"
        prev, nxt = o
        left = f"{off - prev.hi} bytes past the end of {prev}" if prev else "before the first buffer"
        right = f"{nxt.lo - off} bytes before the start of {nxt}" if nxt else "behind the last buffer"
        return f"a gap: {left}; {right}"

    def _record(self, name, a, ranges):
        n = len(self.calls)
        self.calls.append(name)
        for p, nb in ranges:
            lo, hi = p - self.base, p - self.base + nb
            if name == "lasso_upload" or not (0 <= lo and hi <= ARENA_BYTES):
                if name != "lasso_upload":
                    self.problems.append(f"call {n} {name}: its contract names [{p:#x}, +{nb}), which is not arena memory")
                continue
            b = self._owner(lo)
            if not (isinstance(b, _Buf) and hi <= b.hi and b.live):
                self.problems.append(f"call {n} {name}: its contract lets it write arena [{lo:#x}, {hi:#x}), which is not inside one live buffer — starts in {self._describe(lo)}")
            self.allowed.append((lo, hi, n))

    def _shadow_upload(self, dst, src, nbytes):
        lo = dst - self.base
        if not (0 <= lo and lo + nbytes <= ARENA_BYTES):
            self.problems.append(f"lasso_upload to [{dst:#x}, +{nbytes}): not arena memory")
            return
        b = self._owner(lo)
        if not (isinstance(b, _Buf) and lo + nbytes <= b.hi and b.live):
            self.problems.append(f"lasso_upload to arena [{lo:#x}, {lo + nbytes:#x}): not inside one live buffer — starts in {self._describe(lo)}")
        addr = src.value if isinstance(src, C.c_void_p) else C.cast(src, C.c_void_p).value
        self.shadow.view(np.uint8)[lo:lo + nbytes] = np.frombuffer((C.c_uint8 * nbytes).from_address(addr), dtype=np.uint8)

    # ---- per case
    def reset(self):
        """between cases: the used extent holds the pattern again, on the device and in the shadow"""
        n = min((self.used + AUDIT_TAIL + 7) // 8, ARENA_BYTES // 8) if self.used else 0
        if n:
            self.shadow[:n] = pattern(0, n)
            self._raw_upload(0, self.shadow[:n])
        self.used = 0
        self.bufs, self.calls, self.allowed, self.problems = [], [], [], []

    def violations(self):
        """the context must be idle.  Returns the list of findings (strings); empty = the case wrote only what its calls' contracts allow"""
        found = list(self.problems)
        self.runs = []             # (lo, hi, bytes that differ) of every damaged run of the last audit
        n = min(self.used + AUDIT_TAIL, ARENA_BYTES) if self.used else 0
        if not n:
            return found
        dev = self._raw_download(0, n)
        diff = dev != self.shadow.view(np.uint8)[:n]
        for lo, hi, _ in self.allowed:
            diff[lo:hi] = False
        bad = np.flatnonzero(diff)
        if bad.size:
            # runs of damaged bytes (a gap of up to 64 clean bytes does not start a new run), the first few reported
            cuts = np.flatnonzero(np.diff(bad) > 64)
            starts = np.concatenate([[0], cuts + 1]); ends = np.concatenate([cuts, [bad.size - 1]])
            self.runs = [(int(bad[s]), int(bad[e]) + 1, int(e - s + 1)) for s, e in zip(starts, ends)]
            for lo, hi, _ in self.runs[:8]:
                near = min((min(abs(lo - ahi), abs(alo - hi)) if not (alo < hi and lo < ahi) else 0, f"[{alo:#x}, {ahi:#x}) of call {c} {self.calls[c]}") for alo, ahi, c in self.allowed) if self.allowed else None
                dist = f"{near[0]} bytes from the nearest allowed range {near[1]}" if near else "no call of the case may write anything"
                found.append(f"stray write at arena [{lo:#x}, {hi:#x}) ({int(diff[lo:hi].sum())} bytes differ): in {self._describe(lo)}; {dist}")
            if len(starts) > 8:
                found.append(f"... and {len(starts) - 8} more damaged runs, {bad.size} bytes in all")
        return found

    def audit(self):
        found = self.violations()
        if found:
            raise WriteViolation("\n".join(found + ["calls of the case: " + ", ".join(f"{i} {c}" for i, c in enumerate(self.calls))]))
