"""ctypes prototypes for include/lasso_hip.h (shared by the real device library and, in tests, the oracle's mock)."""
import ctypes as C
import functools

u64 = C.c_uint64
u32 = C.c_uint32
i32 = C.c_int32
sz = C.c_size_t
vp = C.c_void_p


class Strategy(C.Structure):
    _fields_ = [("kind", i32), ("c", u32), ("log_m", u32), ("log_r", u32)]


class StrategyCustom(C.Structure):
    """include/lasso_hip.h lasso_strategy_custom: a caller-defined strategy; passed as a pointer to its first member (see lasso_amd.custom.CustomStrategy)"""
    _fields_ = [("base", Strategy), ("num_subtables", u32), ("num_memories", u32), ("tables_u32", C.POINTER(vp)), ("tables_fr", C.POINTER(vp)),
                ("memory_subtable", vp), ("memory_dimension", vp), ("num_terms", u32), ("reserved", u32), ("coeff", vp), ("term_start", vp), ("term_mem", vp)]


class OperandLayout(C.Structure):
    """include/lasso_hip_operands.h lasso_operand_layout: how an operand pair becomes the C table addresses of one lookup"""
    _fields_ = [("operands", u32), ("chunk_bits", u32), ("msb_first", u32)]

    def __repr__(self):
        return f"OperandLayout({self.operands}, {self.chunk_bits}, {self.msb_first})"


class PolyVec(C.Structure):
    """include/lasso_prover_polys.h lasso_host_poly_vec: one vector of a call that takes several"""
    _fields_ = [("values", vp), ("form", i32), ("on_device", i32)]


KINDS = {"and": 0, "or": 1, "xor": 2, "lt": 3, "range": 4, "spark": 5, "custom": 6}   # "spark" = LASSO_SPARK_UNCONFIRMED (include/lasso_hip.h): not in the reference snapshot
CUSTOM_MAX_TERMS, CUSTOM_MAX_FACTORS, CUSTOM_MAX_DEGREE = 256, 2048, 17
K_BIND, K_CUBIC, K_COMBINE, K_EQ, K_GP, K_FINGERPRINT, K_DOT, K_MATVEC, K_MSM, K_MISC, K_MSM_DIRECT, K_COUNT = range(12)
KERNEL_NAMES = ["bind_top(+fused linear round)", "sumcheck_cubic_round(+fused bind)", "sumcheck_combine", "eq_evals", "gp_build", "fingerprint", "multi_dot", "matvec_left", "msm_commit(bucket)", "misc", "msm_opening(direct)"]


def declare(lib):
    P = C.POINTER
    sig = {
        "lasso_ctx_create": (i32, [i32, P(vp)]),
        "lasso_ctx_create_background": (i32, [i32, i32, P(vp)]),
        "lasso_ctx_destroy": (None, [vp]),
        "lasso_last_error": (C.c_char_p, [vp]),
        "lasso_alloc": (i32, [vp, sz, P(vp)]),
        "lasso_free": (i32, [vp, vp]),
        "lasso_upload": (i32, [vp, vp, vp, sz]),
        "lasso_download": (i32, [vp, vp, vp, sz]),
        "lasso_copy": (i32, [vp, vp, vp, sz]),
        "lasso_zero": (i32, [vp, vp, sz]),
        "lasso_sync": (i32, [vp]),
        "lasso_abort": (i32, [vp]),
        "lasso_stream": (vp, [vp]),
        "lasso_prof_enable": (i32, [vp, i32]),
        "lasso_prof_reset": (i32, [vp]),
        "lasso_prof_get": (i32, [vp, i32, P(u64), P(C.c_double), P(C.c_double)]),
        "lasso_prof_get_large": (i32, [vp, i32, P(u64), P(C.c_double), P(C.c_double)]),
        "lasso_prof_get_units": (i32, [vp, i32, i32, P(C.c_double)]),
        "lasso_wait_stats": (i32, [vp, P(u64), P(C.c_double), i32]),
        "lasso_mem_stats": (i32, [vp, P(u64), P(u64), i32]),
        "lasso_trim": (i32, [vp]),
        "lasso_fr_from_u32": (i32, [vp, vp, sz, vp]),
        "lasso_fr_to_u32": (i32, [vp, vp, sz, vp, vp]),
        "lasso_gather": (i32, [vp, vp, vp, sz, vp]),
        "lasso_eq_evals": (i32, [vp, vp, u32, vp]),
        "lasso_eq_evals_scaled": (i32, [vp, vp, u32, vp, vp]),
        "lasso_bind_top": (i32, [vp, P(vp), u32, sz, vp]),
        "lasso_sumcheck_cubic_round": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_cubic_eqw_round": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_cubic_eqw_round_fused": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp, vp]),
        "lasso_sumcheck_cubic_eqw2_begin": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp]),
        "lasso_result_wait": (i32, [vp, vp, sz]),
        "lasso_defer_next": (i32, [vp]),
        "lasso_sumcheck_cubic_tail_begin": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_cubic_tail_next": (i32, [vp, vp]),
        "lasso_sumcheck_linear_tail_begin": (i32, [vp, P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_combine_round": (i32, [vp, P(Strategy), P(vp), vp, sz, u32, vp]),
        "lasso_sumcheck_combine_round_lt_scaled": (i32, [vp, P(Strategy), P(vp), vp, sz, u32, vp]),
        "lasso_lt_prescale": (i32, [vp, P(Strategy), P(vp), P(vp), sz]),
        "lasso_sumcheck_combine_round_lt_u32": (i32, [vp, P(Strategy), P(vp), vp, sz, u32, vp]),
        "lasso_sumcheck_linear_eqw_round": (i32, [vp, P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_linear_eqw_round_fused": (i32, [vp, P(vp), u32, vp, sz, vp, vp]),
        "lasso_sumcheck_linear_eqw_round_fused_from": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp, vp]),
        "lasso_sumcheck_linear_eqw_round_u32": (i32, [vp, P(vp), u32, vp, sz, vp]),
        "lasso_sumcheck_linear_eqw_round_fused_from_u32": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp, vp]),
        "lasso_combine_claim": (i32, [vp, P(Strategy), P(vp), vp, sz, vp]),
        "lasso_multi_dot": (i32, [vp, P(vp), u32, vp, sz, vp]),
        "lasso_read_heads": (i32, [vp, P(vp), u32, vp]),
        "lasso_read_runs": (i32, [vp, P(vp), u32, u32, vp]),
        "lasso_tail_handover_next": (i32, [vp, u32]),
        "lasso_rounds_ahead_ok": (i32, [vp]),
        "lasso_layer_ahead_ok": (i32, [vp]),
        "lasso_sumcheck_cubic_eqw2_begin_eq_ahead": (i32, [vp, P(vp), P(vp), u32, vp, sz, u32]),
        "lasso_sumcheck_cubic_tail_begin_eq_ahead": (i32, [vp, P(vp), P(vp), u32, sz, u32]),
        "lasso_point_post": (i32, [vp, vp, u32, vp]),
        "lasso_point_cancel": (i32, [vp]),
        "lasso_sumcheck_cubic_eqw2_begin_ahead": (i32, [vp, P(vp), P(vp), u32, vp, sz]),
        "lasso_challenge_post": (i32, [vp, vp]),
        "lasso_sumcheck_linear_eqw_round_fused_ahead": (i32, [vp, P(vp), u32, vp, sz]),
        "lasso_sumcheck_cubic_tail_begin_ahead": (i32, [vp, P(vp), P(vp), u32, vp, sz]),
        "lasso_gp_build": (i32, [vp, vp, sz]),
        "lasso_fingerprint_ops": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_fingerprint_ops_gp": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_fingerprint_ops_gp_upper": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_fingerprint_ops_strips": (i32, [vp, vp, vp, vp, sz, vp, vp, u32, sz, sz, vp, vp]),
        "lasso_fingerprint_ops_gp_upper_u32": (i32, [vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_fingerprint_ops_strips_u32": (i32, [vp, vp, vp, vp, sz, vp, vp, u32, sz, sz, vp, vp]),
        "lasso_fingerprint_mem": (i32, [vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_fingerprint_mem_slab": (i32, [vp, vp, vp, sz, u32, u32, vp, vp, vp, vp]),
        "lasso_densify_dim_slab": (i32, [vp, vp, sz, sz, sz, sz, u32, u32, u32, vp, vp, vp, vp]),
        "lasso_matvec_left_dev": (i32, [vp, vp, vp, sz, sz, vp]),
        "lasso_fr_to_bytes": (i32, [vp, vp, sz, vp]),
        "lasso_msm_dev_scaled": (i32, [vp, vp, vp, sz, vp, vp, vp]),
        "lasso_densify_dim": (i32, [vp, vp, sz, sz, sz, sz, u32, vp, vp, vp, vp]),
        "lasso_matvec_left": (i32, [vp, vp, vp, sz, sz, vp]),
        "lasso_bases_create": (i32, [vp, vp, sz, P(vp)]),
        "lasso_bases_create_opt": (i32, [vp, vp, sz, i32, P(vp)]),
        "lasso_bases_destroy": (None, [vp, vp]),
        "lasso_hyrax_commit": (i32, [vp, vp, sz, sz, vp, vp]),
        "lasso_hyrax_commit_compressed": (i32, [vp, vp, sz, sz, vp, vp]),
        "lasso_hyrax_commit_compressed_u32": (i32, [vp, vp, u32, sz, sz, vp, vp]),
        "lasso_bases_has_direct": (i32, [vp]),
        "lasso_bullet_round_slab": (i32, [vp, vp, sz, u32, u32, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_msm_dev_slab": (i32, [vp, vp, vp, sz, u32, u32, vp, vp, vp]),
        "lasso_sumcheck_tail_capacity": (u32, []),
        "lasso_sumcheck_cubic_eqw2_begin_eq": (i32, [vp, P(vp), P(vp), u32, vp, sz, vp, u32, vp]),
        "lasso_sumcheck_cubic_tail_begin_eq": (i32, [vp, P(vp), P(vp), u32, sz, vp, u32, vp]),
        "lasso_rccl_available": (i32, []),
        "lasso_rccl_unique_id": (i32, [vp]),
        "lasso_rccl_init": (i32, [vp, i32, i32, vp]),
        "lasso_rccl_ready": (i32, [vp]),
        "lasso_rccl_shutdown": (i32, [vp]),
        "lasso_rccl_selftest": (i32, [vp]),
        "lasso_ctx_device_uuid": (i32, [vp, vp]),
        "lasso_bullet_tail_ahead_ok": (i32, [vp, vp]),
        "lasso_bullet_tail_ahead": (i32, [vp, vp, sz, vp, vp, vp, sz, vp, vp, vp]),
        "lasso_bases_prepare": (i32, [vp, vp, u32]),
        "lasso_rccl_allgather": (i32, [vp, vp, vp, sz]),
        "lasso_point_row_bytes": (sz, []),
        "lasso_hyrax_commit_rows_dev": (i32, [vp, vp, sz, sz, vp, vp]),
        "lasso_points_reduce_compress": (i32, [vp, vp, u32, sz, vp]),
        "lasso_gather_u32": (i32, [vp, vp, vp, sz, vp]),
        "lasso_materialize_subtable_u32": (i32, [vp, P(Strategy), u32, vp]),
        "lasso_msm": (i32, [vp, vp, vp, sz, vp]),
        "lasso_msm_dev": (i32, [vp, vp, vp, sz, vp]),
        "lasso_inner_products_lr": (i32, [vp, vp, vp, sz, vp]),
        "lasso_bullet_lr": (i32, [vp, vp, sz, vp, sz, vp, vp, vp]),
        "lasso_bullet_round": (i32, [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp, vp, vp, vp]),
        "lasso_bullet_ahead_ok": (i32, [vp, vp]),
        "lasso_bullet_round_ahead": (i32, [vp, vp, sz, vp, vp, vp, vp, vp, vp, sz, vp]),
        "lasso_bullet_post": (i32, [vp, vp, vp]),
        "lasso_bullet_fold": (i32, [vp, vp, vp, sz, vp, sz, vp, vp, vp]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)   # AttributeError here = the library does not export what the header declares
        fn.restype = res
        fn.argtypes = args
    return sorted(sig)


WIRE_STATUS = ["ok", "ok-identity", "non-canonical", "bad-flags", "not-on-curve", "not-in-subgroup"]   # include/lasso_hip_wire.h lasso_wire_status
CAND_STATUS = ["ok", "non-canonical", "no-point"]   # include/lasso_hip_gens.h lasso_cand_status
VALUES_FR, VALUES_U64 = 0, 1   # include/lasso_hip_values.h lasso_values_form

# include/lasso_prover.h lasso_transcript_vtbl: merlin::Transcript as append_message / challenge_bytes callbacks (labels are pointer + length)
APPEND_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t)
CHALLENGE_FN = C.CFUNCTYPE(None, C.c_void_p, C.POINTER(C.c_uint8), C.c_size_t, C.POINTER(C.c_uint8), C.c_size_t)


class TranscriptVtbl(C.Structure):
    _fields_ = [("append_message", APPEND_FN), ("challenge_bytes", CHALLENGE_FN)]


_P, _vt = C.POINTER, C.POINTER(TranscriptVtbl)
# The OPTIONAL parts of the device ABI: extension -> (its header beside include/lasso_hip.h, {function: argument types}); every function returns int32_t.  They are declared
# apart from declare() (declare_ext), on first use: an implementation of lasso_hip.h alone (the tests' mock) has none of them.  The first function of an extension is the one
# error messages name.  The same rows as EXTS in lasso_amd/host/prover_capi.cpp.
EXTENSIONS = {
    "wire": ("lasso_hip_wire.h", {"lasso_points_decompress": [vp, vp, sz, vp, vp, vp]}),                      # the device decoder of compressed points
    "msm_points": ("lasso_hip_msm.h", {"lasso_msm_points": [vp, vp, vp, sz, vp], "lasso_msm_points_dev": [vp, vp, vp, sz, vp]}),   # the MSM over the caller's own points, no lasso_bases
    "operands": ("lasso_hip_operands.h", {"lasso_densify_dim_operands": [vp, vp, vp, sz, _P(OperandLayout), sz, sz, sz, u32, u32, u32, vp, vp, vp, vp]}),   # densify from operand columns
    "gens": ("lasso_hip_gens.h", {"lasso_points_from_candidates": [vp, vp, vp, sz, vp, vp]}),                 # stream candidates to generator points
    "mle": ("lasso_hip_mle.h", {"lasso_tables_mle": [vp, _P(vp), _P(vp), u32, u32, vp, vp], "lasso_tables_mle_dev": [vp, _P(vp), _P(vp), u32, u32, vp, vp]}),   # the MLEs of caller-defined tables at a point
    "values": ("lasso_hip_values.h", {"lasso_lookup_values": [vp, vp, _P(vp), _P(vp), _P(vp), sz, i32, vp]}),   # the lookup results as a vector
    "poly": ("lasso_hip_poly.h", {"lasso_matvec_left_u64_dev": [vp, vp, vp, sz, sz, vp], "lasso_u64_or": [vp, vp, sz, _P(u64)],   # a vector of 64-bit integers as a polynomial
                                  "lasso_hyrax_commit_compressed_u64": [vp, vp, u64, sz, sz, vp, vp]}),
}
# The optional headers of the host prover's ABI (beside include/lasso_prover.h), in the same shape: a prover library built before a header existed does not export it.
PROVER_EXTENSIONS = {
    "mle": ("lasso_prover_mle.h", {"lasso_host_tables_mle": [vp, _P(Strategy), vp, sz, i32, vp], "lasso_host_mle_stats": [vp, _P(u64), _P(i32), i32]}),
    "values": ("lasso_prover_values.h", {"lasso_host_lookup_values": [vp, vp, _P(Strategy), i32, i32, vp], "lasso_host_lookup_values_ref": [_P(Strategy), vp, sz, i32, vp, sz, _P(sz)],
                                         "lasso_host_values_evaluate": [vp, vp, i32, sz, vp, sz, vp], "lasso_host_proof_claimed_evaluation": [C.c_char_p, sz, vp],
                                         "lasso_host_values_stats": [vp, _P(u64), _P(i32), i32], "lasso_host_dense_len": [vp, _P(sz)]}),
    "poly": ("lasso_prover_poly.h", {"lasso_host_poly_commit": [vp, vp, vp, i32, i32, sz, vp, sz, _P(sz)], "lasso_host_poly_gens_new": [vp, C.c_char_p, sz, _P(vp)],
                                     "lasso_host_poly_gens_from_points": [vp, sz, vp, sz, _P(vp)], "lasso_host_poly_gens_free": [vp],
                                     "lasso_host_poly_commitment_append": [_vt, vp, C.c_char_p, C.c_char_p, sz],
                                     "lasso_host_poly_open": [vp, vp, vp, i32, i32, sz, vp, sz, _vt, vp, _vt, vp, vp, vp, sz, _P(sz)],
                                     "lasso_host_poly_verify": [vp, vp, vp, sz, vp, _vt, vp, C.c_char_p, sz, C.c_char_p, sz, _P(i32)],
                                     "lasso_host_poly_stats": [vp, _P(u64), _P(u64), _P(i32), i32]}),
    "polys": ("lasso_prover_polys.h", {"lasso_host_polys_commit": [vp, vp, _P(PolyVec), sz, sz, vp, sz, _P(sz)],
                                       "lasso_host_polys_open": [vp, vp, _P(PolyVec), sz, sz, vp, sz, _vt, vp, _vt, vp, vp, vp, sz, _P(sz)],
                                       "lasso_host_polys_verify": [vp, vp, vp, sz, vp, sz, _vt, vp, C.c_char_p, sz, C.c_char_p, sz, _P(i32)],
                                       "lasso_host_polys_evaluate": [vp, _P(PolyVec), sz, sz, vp, sz, vp], "lasso_host_polys_stats": [vp, _P(u64), _P(u64), i32]}),
    "blind": ("lasso_prover_blind.h", {"lasso_host_poly_commit_blinded": [vp, vp, vp, i32, i32, sz, _vt, vp, vp, vp, sz, _P(sz)],
                                       "lasso_host_poly_open_blinded": [vp, vp, vp, i32, i32, sz, vp, sz, vp, vp, _vt, vp, _vt, vp, vp, vp, vp, sz, _P(sz)],
                                       "lasso_host_poly_verify_committed": [vp, vp, vp, sz, C.c_char_p, _vt, vp, C.c_char_p, sz, C.c_char_p, sz, _P(i32)],
                                       "lasso_host_polys_commit_blinded": [vp, vp, _P(PolyVec), sz, sz, _vt, vp, vp, vp, sz, _P(sz)],
                                       "lasso_host_polys_open_blinded": [vp, vp, _P(PolyVec), sz, sz, vp, sz, vp, _vt, vp, _vt, vp, vp, vp, sz, _P(sz)],
                                       "lasso_host_blind_stats": [vp, _P(u64), _P(u64), i32]}),
}


def declare_ext(lib, name, table=EXTENSIONS):
    """the prototypes of extension `name` of `table`; returns its function names, sorted.  AttributeError = the library does not export it."""
    sig = table[name][1]
    for fn_name, args in sig.items():
        fn = getattr(lib, fn_name)
        fn.restype = i32
        fn.argtypes = args
    return sorted(sig)


# the names the extensions' own tests and tools declare them by: each is declare_ext for one row of EXTENSIONS
declare_wire = functools.partial(declare_ext, name="wire")
declare_msm_points = functools.partial(declare_ext, name="msm_points")
declare_operands = functools.partial(declare_ext, name="operands")
declare_gens = functools.partial(declare_ext, name="gens")
declare_mle = functools.partial(declare_ext, name="mle")
declare_values = functools.partial(declare_ext, name="values")
declare_poly = functools.partial(declare_ext, name="poly")


def declared_ext(owner, name, table, what, error):
    """owner.lib with extension `name` declared on first use; a library without it is an error (`error`, naming the extension's first function), not a fall-back"""
    done = owner.__dict__.setdefault("_exts", set())
    if name not in done:
        try:
            declare_ext(owner.lib, name, table)
        except AttributeError:
            raise error(f"this {what} library does not export {next(iter(table[name][1]))} (include/{table[name][0]})") from None
        done.add(name)
    return owner.lib
