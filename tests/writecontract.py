"""The write contract of the device ABI: for every exported function of include/*.h, the byte ranges of CALLER DEVICE memory the call may write, as a function of its C arguments.

An entry is `f(a, lib) -> [(address, nbytes), ...]`: `a` holds the call's arguments in C order (a[0] = the context) as tests/arenautil.py normalises them — addresses and integers
as int (NULL = 0), a host table of device pointers as a list of int, a struct passed by reference as the ctypes object — and `lib` is the library itself, for the two extents that
depend on it (lasso_point_row_bytes, the communicator's world size).  An empty list: the call writes nothing there (its results go to host memory, or it only changes the
context).  The headers are the source of every extent; where a header was silent the kernel was read and the header now says it.

tests/test_write_contract_cpu.py requires exactly one entry per exported symbol."""
import ctypes as C

FR, U32 = 32, 4      # sizeof(lasso_fr), sizeof(uint32_t)


def _none(a, lib):
    return []


def _one(p, nbytes):
    return [(p, nbytes)] if p and nbytes > 0 else []


def _each(ptrs, count, nbytes):
    return [(p, nbytes) for p in list(ptrs)[:count] if p and nbytes > 0] if ptrs else []


def _strategy(s):
    """a `const lasso_strategy*` argument as the struct"""
    if hasattr(s, "c") and hasattr(s, "log_m"):
        return s
    if hasattr(s, "base"):
        return s.base
    return C.cast(s, C.POINTER(_Strategy())).contents


def _Strategy():
    from lasso_amd import _abi
    return _abi.Strategy


def _lower_halves(tables, count_at, n_at):
    """the rounds that bind: the lower n/2 elements of every array of the named pointer tables (n = the length before the bind)"""
    def f(a, lib):
        out = []
        for t in tables:
            out += _each(a[t], a[count_at], FR * (a[n_at] // 2))
        return out
    return f


def _lt_prescale(a, lib):                     # (ctx, s, d_src, d_polys, n)
    c = _strategy(a[1]).c
    if a[2]:                                   # out of place: all 2C polynomials land in d_polys (the scaled ones and the plain copies)
        return _each(a[3], 2 * c, FR * a[4])
    return [(a[3][2 * m], FR * a[4]) for m in range(c - 1) if a[3][2 * m]]     # in place: LT_m for m < C - 1; LT_{C-1} and every EQ_m are not touched


def _bullet_folding(aout, bout, wout, n_at, nk_at):
    def f(a, lib):
        nk = a[nk_at]
        return _one(a[aout], FR * nk) + _one(a[bout], FR * nk) + _one(a[wout], FR * (a[n_at] // nk))
    return f


def _densify(u32_at, world_at, s_at, logm_at):
    def f(a, lib):
        w = a[world_at] if world_at is not None else 1
        s, m = a[s_at] // w, (1 << a[logm_at]) // w
        return _one(a[u32_at], U32 * s) + _one(a[u32_at + 1], FR * s) + _one(a[u32_at + 2], FR * s) + _one(a[u32_at + 3], FR * m)
    return f


def _fingerprint(out_at, elems):
    return lambda a, lib: _one(a[out_at], FR * elems(a)) + _one(a[out_at + 1], FR * elems(a))


CONTRACT = {
    # ---- context, memory, accounting: nothing but a transfer's own destination
    "lasso_ctx_create": _none, "lasso_ctx_create_background": _none, "lasso_ctx_device_uuid": _none, "lasso_ctx_destroy": _none, "lasso_last_error": _none,
    "lasso_alloc": _none, "lasso_free": _none, "lasso_mem_stats": _none, "lasso_trim": _none, "lasso_sync": _none, "lasso_abort": _none, "lasso_stream": _none,
    "lasso_upload": lambda a, lib: _one(a[1], a[3]),
    "lasso_download": _none,
    "lasso_copy": lambda a, lib: _one(a[1], a[3]),
    "lasso_zero": lambda a, lib: _one(a[1], a[2]),
    "lasso_prof_enable": _none, "lasso_prof_reset": _none, "lasso_prof_get": _none, "lasso_prof_get_large": _none, "lasso_prof_get_units": _none, "lasso_wait_stats": _none,
    # ---- polynomial kernels
    "lasso_fr_from_u32": lambda a, lib: _one(a[3], FR * a[2]),
    "lasso_fr_to_u32": lambda a, lib: _one(a[3], U32 * a[2]),
    "lasso_gather": lambda a, lib: _one(a[4], FR * a[3]),
    "lasso_eq_evals": lambda a, lib: _one(a[3], FR << a[2]),
    "lasso_eq_evals_scaled": lambda a, lib: _one(a[4], FR << a[2]),
    "lasso_bind_top": _lower_halves([1], 2, 3),
    "lasso_sumcheck_cubic_round": _none, "lasso_sumcheck_cubic_eqw_round": _none,
    "lasso_sumcheck_cubic_eqw_round_fused": _lower_halves([1, 2], 3, 5),
    "lasso_sumcheck_cubic_eqw2_begin": lambda a, lib: _lower_halves([1, 2], 3, 5)(a, lib) if a[6] else [],      # r == NULL: evaluation only
    "lasso_result_wait": _none, "lasso_defer_next": _none,
    "lasso_sumcheck_cubic_eqw2_begin_eq": lambda a, lib: _one(a[4], FR * (a[5] // 2)),
    "lasso_sumcheck_cubic_tail_begin": _none, "lasso_sumcheck_cubic_tail_begin_eq": _none, "lasso_sumcheck_cubic_tail_next": _none, "lasso_sumcheck_linear_tail_begin": _none,
    "lasso_tail_handover_next": _none, "lasso_sumcheck_tail_capacity": _none,
    "lasso_rounds_ahead_ok": _none, "lasso_layer_ahead_ok": _none,
    "lasso_sumcheck_cubic_eqw2_begin_ahead": _lower_halves([1, 2], 3, 5),
    "lasso_challenge_post": _none,
    "lasso_sumcheck_linear_eqw_round_fused_ahead": _lower_halves([1], 2, 4),
    "lasso_sumcheck_cubic_tail_begin_ahead": _none,
    "lasso_sumcheck_cubic_eqw2_begin_eq_ahead": lambda a, lib: _one(a[4], FR * (a[5] // 2)),
    "lasso_sumcheck_cubic_tail_begin_eq_ahead": _none, "lasso_point_post": _none, "lasso_point_cancel": _none,
    "lasso_sumcheck_combine_round": _none, "lasso_sumcheck_combine_round_lt_scaled": _none, "lasso_sumcheck_combine_round_lt_u32": _none, "lasso_combine_claim": _none,
    "lasso_lt_prescale": _lt_prescale,
    "lasso_sumcheck_linear_eqw_round": _none, "lasso_sumcheck_linear_eqw_round_u32": _none,
    "lasso_sumcheck_linear_eqw_round_fused": _lower_halves([1], 2, 4),
    "lasso_sumcheck_linear_eqw_round_fused_from": _lower_halves([2], 3, 5),          # nothing of d_src where it is a different array
    "lasso_sumcheck_linear_eqw_round_fused_from_u32": _lower_halves([2], 3, 5),
    "lasso_multi_dot": _none, "lasso_read_heads": _none, "lasso_read_runs": _none,
    "lasso_gp_build": lambda a, lib: _one(a[1] + FR * a[2], FR * (a[2] - 2)) if a[1] else [],                 # layers 1.. of the tree: [n, 2n - 2)
    "lasso_fingerprint_ops": _fingerprint(7, lambda a: a[4]),
    "lasso_fingerprint_ops_gp": _fingerprint(7, lambda a: 2 * a[4] - 2),
    "lasso_fingerprint_ops_gp_upper": _fingerprint(7, lambda a: a[4] - 2),
    "lasso_fingerprint_ops_gp_upper_u32": _fingerprint(7, lambda a: a[4] - 2),
    "lasso_fingerprint_ops_strips": _fingerprint(10, lambda a: 2 * a[7] * a[9]),
    "lasso_fingerprint_ops_strips_u32": _fingerprint(10, lambda a: 2 * a[7] * a[9]),
    "lasso_fingerprint_mem": _fingerprint(6, lambda a: a[3]),
    "lasso_fingerprint_mem_slab": _fingerprint(8, lambda a: a[3]),
    "lasso_matvec_left": _none,
    "lasso_matvec_left_dev": lambda a, lib: _one(a[5], FR * a[4]),
    "lasso_fr_to_bytes": _none,
    # ---- densify: also on the call that fails with an out-of-range index
    "lasso_densify_dim": _densify(7, None, 5, 6),
    "lasso_densify_dim_slab": _densify(9, 7, 5, 6),
    "lasso_densify_dim_operands": _densify(11, 9, 7, 8),
    # ---- curve kernels
    "lasso_bases_create": _none, "lasso_bases_create_opt": _none, "lasso_bases_destroy": _none, "lasso_bases_prepare": _none, "lasso_bases_has_direct": _none,
    "lasso_hyrax_commit": _none, "lasso_hyrax_commit_compressed": _none, "lasso_hyrax_commit_compressed_u32": _none,
    "lasso_rccl_available": _none, "lasso_rccl_unique_id": _none, "lasso_rccl_init": _none, "lasso_rccl_shutdown": _none, "lasso_rccl_ready": _none, "lasso_rccl_selftest": _none,
    "lasso_rccl_allgather": lambda a, lib: _one(a[2], a[3] * max(lib.lasso_rccl_ready(C.c_void_p(a[0])), 1)),
    "lasso_point_row_bytes": _none,
    "lasso_hyrax_commit_rows_dev": lambda a, lib: _one(a[5], a[2] * lib.lasso_point_row_bytes()),
    "lasso_points_reduce_compress": _none,
    "lasso_materialize_subtable_u32": lambda a, lib: _one(a[3], U32 << _strategy(a[1]).log_m),
    "lasso_gather_u32": lambda a, lib: _one(a[4], U32 * a[3]),
    "lasso_msm": _none, "lasso_msm_dev": _none, "lasso_msm_dev_scaled": _none, "lasso_msm_dev_slab": _none,
    "lasso_msm_points": _none, "lasso_msm_points_dev": _none,                        # include/lasso_hip_msm.h: points and scalars are only read
    "lasso_points_decompress": _none, "lasso_points_from_candidates": _none,         # include/lasso_hip_wire.h, lasso_hip_gens.h: host memory in, host memory out
    # ---- the opening
    "lasso_inner_products_lr": _none, "lasso_bullet_lr": _none,
    "lasso_bullet_round": lambda a, lib: _bullet_folding(6, 7, 8, 2, 9)(a, lib) if a[10] else [],             # u == NULL: the *_out pointers are ignored
    "lasso_bullet_round_slab": lambda a, lib: _bullet_folding(8, 9, 10, 2, 11)(a, lib) if a[12] else [],
    "lasso_bullet_ahead_ok": _none, "lasso_bullet_tail_ahead_ok": _none, "lasso_bullet_post": _none,
    "lasso_bullet_round_ahead": _bullet_folding(6, 7, 8, 2, 9),
    "lasso_bullet_tail_ahead": lambda a, lib: _one(a[3], FR) + _one(a[4], FR) + _one(a[7], FR * 2 * a[6]),   # the last fold: a[0], b[0] and the 2 nw folded weights
    "lasso_bullet_fold": lambda a, lib: _one(a[1], FR * (a[3] // 2)) + _one(a[2], FR * (a[3] // 2)) + _one(a[6], FR * 2 * a[5]),
}

# include/lasso_prover.h: the host prover owns its device memory; none of its entry points takes a caller's device pointer
for _n in ("commit create ctx debug_cubic_batched dense_free dense_info densify densify_operands densify_stats destroy gen_indices gen_random_point gens_free gens_from_points "
           "gens_new gens_points gens_prepare gens_stats last_error mem_stats merlin_free merlin_new merlin_vtbl msm_points msm_stats operand_indices operand_layout "
           "points_decompress points_from_candidates prove prove_cb random_tape_new set_capacity set_comm set_comm_shm set_throughput_mode strategy_check verify verify_cb "
           "wire_stats").split():
    CONTRACT["lasso_host_" + _n] = _none
