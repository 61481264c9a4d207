"""The suite's device calls once more, over tests/arenautil.py's ArenaDevice: every case fails for wrong bytes (the imported tests' own assertions keep running) or for a write
outside what tests/writecontract.py allows its calls.  Not collected by name: tests/test_write_contract_cpu.py runs it over the oracle's mock (LASSO_ARENA_OVER=mock),
tests/test_gpu_write_contract.py on the device, one child process per group and switch setting.

Groups (the prefix of a case's name; `-k` selects them):
  test_k_    every test of tests/test_gpu_kernels.py that takes `devs`, minus EXCLUDED
  test_fe_   tests/test_gpu_field_edges.py, the same way (device only)
  test_op_   the densify-level tests of tests/test_gpu_operands.py (device only: the mock has no operand entry point)
  test_mp_   the kernel-level tests of tests/test_gpu_msm_points.py (device only), without its 2^17 case
  test_wp_   the kernel-level tests of tests/test_gpu_wire_points.py and
  test_gd_   of tests/test_gpu_gens_device.py (device only; the tests that take `pair`, on the build under test): their calls pass host memory, so nothing of theirs lives in the
             arena; what holds them is LASSO_SCRATCH_GUARD, behind the 129 n and 98 n bytes their scratch layouts ask for
  test_tab_  the rows of roundvariants / passvariants / msmvariants TABLE whose setting is SETTINGS[LASSO_ARENA_SETTING]
  test_sens_ the harness's own sensitivity: planted writes and shrunk contracts must be reported, with the right owner

On the device every child runs with LASSO_SCRATCH_GUARD=1 (tests/test_gpu_write_contract.py): the library puts a guard of 64 KiB directly behind the REQUESTED size of every request
of its scratch, sort and big-result buffers, and the lasso_sync before the audit fails the case that damaged one.

They also run with LASSO_POISON=1: every allocation of the library (scratch, sort and big-result buffers, generator tables, mapped result buffers, lasso_alloc) starts as the
word 0x00000001 repeated, and the first request a call makes of one of the three buffers fills the requested range with it, so a kernel that reads what this call did not store
fails the case's own parity assertion.  The last two test_sens_ cases show that the switch is live in the child.

NOT covered (tests/arenautil.py): stray writes into the generator tables, the mapped result buffers and every other allocation the library owns outside those three buffers,
stray reads that do not change a result, a stray write of the pattern's own bytes, the collectives of slab mode."""
import inspect
import os

import numpy as np
import pytest

import arenautil
import msmvariants as MV
import passvariants as PV
import roundvariants as RV
import test_gpu_field_edges as FE
import test_gpu_gens_device as GD
import test_gpu_kernels as K
import test_gpu_msm_points as MP
import test_gpu_operands as OP
import test_gpu_wire_points as WP
from fieldref import CURVE
from gpuutil import load_mock, rand_fr

OVER_MOCK = os.environ.get("LASSO_ARENA_OVER") == "mock"
pytestmark = [] if OVER_MOCK else [pytest.mark.gpu]

# tests of tests/test_gpu_kernels.py that take `devs` and are NOT re-collected: they test protocol state or accounting, not a computation
EXCLUDED = {
    "test_abort_releases_a_waiting_tail_kernel": "protocol: ends in lasso_abort with a resident kernel waiting; what the kernel had written by then is not defined",
    "test_abort_releases_a_waiting_linear_tail_kernel": "protocol: the same for the linear tail",
    "test_layer_enqueued_ahead_and_never_posted_is_aborted_quickly": "protocol: a layer that never gets its point, released by lasso_abort",
    "test_launch_wait_protocol_errors": "protocol: only refusals (return codes) are asserted",
    "test_protocol_refusals_unchanged": "protocol: the table of refusals in every state",
    "test_rccl_two_ranks_on_one_device": "RCCL: two contexts of its own and a collective between them (slab-mode collectives are out of scope)",
    # without `devs`, listed for the record: test_mem_stats_accounts_allocations_tables_and_peak (accounting of a context of its own),
    # test_big_eq_tables_formed_inside_round0_in_their_own_process (starts its own process)
}
# over the mock (CPU) only: what the mock does not implement, or serves too slowly for a CPU test.  tests/test_gpu_field_edges.py as a whole is left to the device as well: its
# cases require the same result from lazily reduced inputs, which the device library promises and the mock's field type does not
MOCK_LACKS = {"test_slab_commitment_exchange_on_device": "needs librccl and the kernels' own point rows",
              "test_hyrax_commit_full_width_wide_windows": "three serial commitments of up to 512 x 300 full-width scalars: 10 to 45 s a case over the mock",
              "test_cubic_round_launched_ahead": "asserts the refusals of the device library while a kernel waits on the device; the mock has nothing to wait for"}

SETTINGS = arenautil.SETTINGS
SETTING = SETTINGS[int(os.environ.get("LASSO_ARENA_SETTING", "0"))]


@pytest.fixture(scope="module")
def devs():
    from lasso_amd import Device
    mock_lib = load_mock()
    real = arenautil.ArenaDevice(0, lib=mock_lib) if OVER_MOCK else arenautil.ArenaDevice(0, curve=CURVE)
    if OVER_MOCK:
        real._dry_run_mock = True      # tests/test_gpu_kernels.py test_layer_enqueued_ahead_of_its_point: devs[0] is a mock too, it refuses nothing while a launch waits
    mock = Device(0, lib=mock_lib)
    yield real, mock
    print(f"\n[arena] largest extent used by a case: {real.max_used} of {arenautil.ARENA_BYTES} bytes")
    real.close(); mock.close()


@pytest.fixture(autouse=True)
def arena_case(devs):
    """the arena holds the pattern before the case; once the case is over and the context idle, nothing outside its calls' write sets may have changed"""
    arena = devs[0]
    arena.reset()
    yield
    arena.sync()
    arena.audit()


@pytest.fixture(scope="module")
def pair_parts(devs):
    """what the `pair` fixtures of tests/test_gpu_wire_points.py and tests/test_gpu_gens_device.py build beside the device, for the build under test"""
    import wireutil
    from lasso_amd import HostProver
    hp = HostProver(curve=CURVE)
    yield hp, [b for _, b, _ in wireutil.crafted(CURVE)], wireutil.random_valid(CURVE, 300, seed=11)
    hp.close()


@pytest.fixture
def pair(request, devs, pair_parts):
    """those modules' `pair`, with the arena device in the device's place"""
    hp, crafted, valid = pair_parts
    return (CURVE, devs[0], hp, crafted, valid) if request.function.__module__ == WP.__name__ else (CURVE, devs[0], hp)


def _collect(module, prefix, skip=(), takes="devs"):
    n = 0
    for name, fn in vars(module).items():
        if not (name.startswith("test_") and inspect.isfunction(fn) and takes in inspect.signature(fn).parameters):
            continue
        if name in skip:
            continue
        globals()[prefix + name[5:]] = fn
        n += 1
    return n


gens_300 = K.gens_300
COUNTS = {"k": _collect(K, "test_k_", skip=set(EXCLUDED) | (set(MOCK_LACKS) if OVER_MOCK else set())),
          }
if not OVER_MOCK:
    COUNTS["fe"] = _collect(FE, "test_fe_")
    prover_lib, points = OP.prover_lib, MP.points
    COUNTS["op"] = _collect(OP, "test_op_")
    COUNTS["mp"] = _collect(MP, "test_mp_", skip={"test_2p17_points_scratch_is_counted_and_bounded"})      # long, and about lasso_mem_stats (tests/test_gpu_bn254.py leaves it out too)
    COUNTS["wp"] = _collect(WP, "test_wp_", takes="pair")      # not the verifier's end-to-end test (processes of its own); the largest batch is 8449 points
    COUNTS["gd"] = _collect(GD, "test_gd_", takes="pair")      # not the route test (proofs in processes of its own); the largest batch is 16500 candidates


# ---- the three tables

def _table_rows():
    rows = [("round", r) for r in RV.rows_of(SETTING)] + [("pass", r) for r in PV.rows_of(SETTING)] + [("msm", r) for r in MV.rows_of(SETTING)]
    if OVER_MOCK:      # a caller-defined strategy has a mock of its own (passvariants.mock_for); the mock has no lasso_hyrax_commit_rows_dev
        rows = [(t, r) for t, r in rows if not (t == "pass" and r.args.get("kind") == "custom") and not (t == "msm" and r.entry == "hyrax_commit_rows_dev")]
    return rows


_REF = {}


def _reference(table, row, mock):
    key = (table,) + tuple([RV, PV, MV][["round", "pass", "msm"].index(table)].reference_key(row))
    if key not in _REF:
        if table == "round":
            _REF[key] = RV.reference(mock, row)
        elif table == "msm":
            _REF[key] = MV.reference(mock, row)
        else:
            from lasso_amd import Device
            lib = PV.mock_for(row)
            m = mock if lib is mock.lib else Device(0, lib=lib)
            _REF[key] = PV.printable(PV.run_row(m, row, reduced=True))
            if m is not mock:
                m.close()
    return _REF[key]


@pytest.mark.parametrize("table,row", _table_rows(), ids=[f"{t}-{r.id}".replace(" ", "") for t, r in _table_rows()])
def test_tab_row(devs, table, row):
    arena, mock = devs
    assert all(os.environ.get(k) == v for k, v in SETTING.items()), f"the process does not run under {SETTING}"
    want = _reference(table, row, mock)
    if table == "round":
        got = RV.comparable(RV.run_row(arena, row))
    elif table == "msm":
        got = MV.as_wire(mock.lib, MV.run_row(arena, row, mock.lib))
    else:
        got = PV.printable(PV.run_row(arena, row))
    assert set(got) == set(want)
    for name, w in want.items():
        g = got[name]
        assert (g == w) if isinstance(w, str) else np.array_equal(np.asarray(g).reshape(np.shape(w)), w), f"{row.id}: `{name}` differs from the mock's"


# ---- sensitivity: the harness must see what it is there to see.  Nothing here touches a kernel: a saboteur writes 32 bytes with the library's own lasso_upload, past the shadow.

def _plant(arena, off):
    """32 bytes at arena offset `off`, every one of them different from what belongs there"""
    bad = ~arena.shadow.view(np.uint8)[off:off + 32]
    arena._raw_upload(off, bad)


def _off(arena, ptr):
    return ptr - arena.base


def _expect_one(arena, lo, owner_text, planted=True):
    """exactly one finding: the element at arena offset `lo`, with the right owner.  planted: all 32 bytes differ (the saboteur sees to that); a kernel's own element may share
    a byte or two with the pattern"""
    found, runs = arena.violations(), arena.runs
    arena.reset()
    assert len(found) == 1 and len(runs) == 1, found
    rlo, rhi, count = runs[0]
    assert lo <= rlo and rhi <= lo + 32 and count >= (32 if planted else 24), (runs, lo)
    assert f"stray write at arena [{rlo:#x}, {rhi:#x})" in found[0] and owner_text in found[0], found[0]
    return found[0]


def _bind_case(arena, n=64):
    """one lasso_bind_top over a field array with a 32-bit neighbour and a table nobody writes: -> (z, u32 neighbour, input) pointers"""
    rng = np.random.default_rng(n)
    pz = arena.upload(rand_fr(rng, n)); pu = arena.upload(rng.integers(0, 1 << 32, size=n, dtype=np.uint32)); pin = arena.upload(rand_fr(rng, n))
    arena.bind_top([pz], n, rand_fr(rng, 1, edge=False)[0])
    arena.sync()
    return pz, pu, pin


def test_sens_clean_case_has_no_finding(devs):
    arena = devs[0]
    _bind_case(arena)
    assert arena.violations() == []


def test_sens_one_element_past_an_outputs_end(devs):
    arena = devs[0]
    ell = 6
    p = arena.alloc(32 << ell)
    arena.eq_evals(rand_fr(np.random.default_rng(1), ell, edge=False), p)
    arena.sync()
    lo = _off(arena, p) + (32 << ell)
    _plant(arena, lo)
    text = _expect_one(arena, lo, "a gap: 0 bytes past the end of buffer #0")
    assert "0 bytes from the nearest allowed range" in text and "lasso_eq_evals" in text


def test_sens_one_element_before_an_outputs_start(devs):
    arena = devs[0]
    ell = 6
    arena.upload(rand_fr(np.random.default_rng(2), 8))
    p = arena.alloc(32 << ell)
    arena.eq_evals(rand_fr(np.random.default_rng(1), ell, edge=False), p)
    arena.sync()
    lo = _off(arena, p) - 32
    _plant(arena, lo)
    _expect_one(arena, lo, "32 bytes before the start of buffer #1")


def test_sens_upper_half_of_a_bound_array(devs):
    arena = devs[0]
    n = 64
    pz, _, _ = _bind_case(arena, n)
    lo = _off(arena, pz) + 32 * (n // 2)
    _plant(arena, lo)
    text = _expect_one(arena, lo, f"in buffer #0 (fr,")
    assert f"{32 * (n // 2)} bytes from its start" in text and "0 bytes from the nearest allowed range" in text and "lasso_bind_top" in text


def test_sens_an_input_array(devs):
    arena = devs[0]
    pz, pu, pin = _bind_case(arena)
    lo = _off(arena, pin) + 32 * 5
    _plant(arena, lo)
    _expect_one(arena, lo, "in buffer #2 (fr,")


def test_sens_middle_of_a_gap(devs):
    arena = devs[0]
    pz, pu, pin = _bind_case(arena)
    b1, b2 = arena.bufs[1], arena.bufs[2]
    lo = (b1.hi + (b2.lo - b1.hi) // 2) & ~7
    assert lo - b1.hi >= 2000 and b2.lo - lo >= 2000
    _plant(arena, lo)
    text = _expect_one(arena, lo, f"a gap: {lo - b1.hi} bytes past the end of buffer #1 (u32,")
    assert f"{b2.lo - lo} bytes before the start of buffer #2" in text


def test_sens_the_u32_neighbour_of_a_field_array(devs):
    arena = devs[0]
    pz, pu, pin = _bind_case(arena)
    assert pu % 16 == 4 and pz % 64 == 32
    lo = _off(arena, pu)
    _plant(arena, lo)
    _expect_one(arena, lo, "in buffer #1 (u32,")


def test_sens_a_freed_buffer_is_still_watched(devs):
    arena = devs[0]
    pz, pu, pin = _bind_case(arena)
    arena.free(pin)
    lo = _off(arena, pin)
    _plant(arena, lo)
    text = _expect_one(arena, lo, "in buffer #2 (fr,")
    assert "freed after call" in text


def test_sens_a_call_without_a_contract_fails(devs):
    arena = devs[0]
    saved = arena.lib._contract
    arena.lib._contract = {k: v for k, v in saved.items() if k != "lasso_gp_build"}
    try:
        with pytest.raises(arenautil.WriteViolation, match="no write contract for lasso_gp_build"):
            arena.gp_build(arena.alloc(64 * 8), 8)
    finally:
        arena.lib._contract = saved


def _with_contract(arena, name, entry):
    saved = arena.lib._contract
    arena.lib._contract = dict(saved, **{name: entry})
    return saved


def test_sens_gp_build_contract_shrunk_by_one_element(devs):
    """[n, 2n - 3) instead of [n, 2n - 2): the tree's last layer-element written is a finding"""
    arena = devs[0]
    n = 64
    tree = np.zeros((2 * n, 4), dtype=np.uint64); tree[:n] = rand_fr(np.random.default_rng(3), n)
    saved = _with_contract(arena, "lasso_gp_build", lambda a, lib: [(a[1] + 32 * a[2], 32 * (a[2] - 3))])
    try:
        p = arena.upload(tree)
        arena.gp_build(p, n)
        arena.sync()
    finally:
        arena.lib._contract = saved
    lo = _off(arena, p) + 32 * (2 * n - 3)
    text = _expect_one(arena, lo, "in buffer #0 (fr,", planted=False)
    assert "lasso_gp_build" in text


def test_sens_densify_contract_shrunk_by_one_element(devs):
    """d_final minus its last element"""
    arena = devs[0]
    full = arena.lib._contract["lasso_densify_dim"]
    n_lookups, c, log_m = 100, 2, 4
    s, m = 128, 1 << log_m
    idx = np.random.default_rng(4).integers(0, m, size=(n_lookups, c), dtype=np.uint64)
    idx[:3, 0] = m - 1      # the last address is used: its final timestamp is not what the zero-filled buffer holds
    saved = _with_contract(arena, "lasso_densify_dim", lambda a, lib: full(a, lib)[:3] + [(a[10], 32 * ((1 << a[6]) - 1))])
    try:
        pi = arena.upload(idx)
        outs = [arena.alloc(4 * s), arena.alloc(32 * s), arena.alloc(32 * s), arena.alloc(32 * m)]
        arena.densify_dim(pi, n_lookups, c, 0, s, log_m, *outs)
        arena.sync()
    finally:
        arena.lib._contract = saved
    lo = _off(arena, outs[3]) + 32 * (m - 1)
    text = _expect_one(arena, lo, "in buffer #4 (fr,", planted=False)
    assert "lasso_densify_dim" in text


# ---- LASSO_POISON (device only: the children of tests/test_gpu_write_contract.py set it): the switch is live in this process.  Every case above then ran with the library's own
# allocations, and the requested range of each call's first scratch / sort / big-result request, holding the fill word instead of zeros or an earlier call's bytes.

POISON_WORD = 0x00000001      # lasso_amd/csrc/device_switches.cuh POISON_WORD


def _raw_alloc_bytes(arena, nbytes):
    """a lasso_alloc of the library's own (not the arena's bump allocation), read back before anything is written to it"""
    import ctypes as C
    p = C.c_void_p()
    assert arena.raw.lasso_alloc(arena.ctx, nbytes, C.byref(p)) == 0 and p.value
    try:
        out = np.empty(nbytes, dtype=np.uint8)
        assert arena.raw.lasso_download(arena.ctx, out.ctypes.data_as(C.c_void_p), p, nbytes) == 0
    finally:
        arena.raw.lasso_free(arena.ctx, p)
    return out


def _assert_fill(got):
    want = np.zeros(len(got), dtype=np.uint8); want[::4] = POISON_WORD      # little-endian 0x00000001 repeated; an odd tail gets the word's first bytes
    bad = np.flatnonzero(got != want)
    assert len(bad) == 0, f"{len(bad)} of {len(got)} bytes of a fresh lasso_alloc do not hold the fill word, the first at offset {bad[0]}: {got[bad[0] & ~3:(bad[0] & ~3) + 8]}"


def _live_bytes(arena):
    import ctypes as C
    live, peak = C.c_uint64(), C.c_uint64()
    assert arena.raw.lasso_mem_stats(arena.ctx, C.byref(live), C.byref(peak), 0) == 0
    return live.value


if not OVER_MOCK:
    def test_sens_fresh_allocation_holds_the_fill_word(devs):
        assert os.environ.get("LASSO_POISON") == "1", "the child runs without LASSO_POISON=1"
        for nbytes in (4096, 8192, 6001, 1):
            _assert_fill(_raw_alloc_bytes(devs[0], nbytes))

    def test_sens_zz_allocation_after_growth_and_trim_holds_the_fill_word(devs):
        """the last case of its child: after the cases above, and after this one has grown the scratch beyond its floor with live data, trimmed it and grown it again, an
        allocation of the size just freed (what the allocator hands back first) and small ones hold the fill word, not what the scratch held"""
        arena = devs[0]
        assert os.environ.get("LASSO_POISON") == "1", "the child runs without LASSO_POISON=1"
        n = 1 << 18
        src = arena.upload(rand_fr(np.random.default_rng(18), n))
        arena.sync()
        assert arena.raw.lasso_trim(arena.ctx) == 0      # the scratch at its floor, whatever the cases before left
        live0 = _live_bytes(arena)
        for rep in range(2):
            arena.fr_to_bytes(src, n)      # 8 MiB of scratch: twice its floor
            arena.sync()
            grown = _live_bytes(arena)
            assert grown >= live0 + (4 << 20), (live0, grown)
            assert arena.raw.lasso_trim(arena.ctx) == 0
            assert _live_bytes(arena) <= grown - (4 << 20)
            for nbytes in (8 << 20, 4096, 8192 + 2):
                _assert_fill(_raw_alloc_bytes(arena, nbytes))
