"""ctypes binding of the HIP library (include/llda_gibbs.h).

The product path has NO CPU fallback: if ``libllda_gibbs.so`` is missing this module raises, and
every device entry point raises on a non-zero return code.
"""
import ctypes
import os

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("LLDA_GIBBS_LIB") or os.path.join(_HERE, "libllda_gibbs.so")   # (override: ablation builds, tools/)

MAX_K = 7688            # LLDA_MAX_K: every K up to here has <= 64 pairwise leaves
MAX_KP = 8192
MAX_LEAVES = 8          # narrow layouts
MAX_WIDE_LEAVES = 64
MAX_ROUNDS = 4
ABI_VERSION = 22

_c_i32, _c_i64, _c_u32, _c_u64 = ctypes.c_int32, ctypes.c_int64, ctypes.c_uint32, ctypes.c_uint64
_c_p, _c_d = ctypes.c_void_p, ctypes.c_double


class LldaLayout(ctypes.Structure):
    """struct llda_layout (include/llda_gibbs.h)."""
    _fields_ = [("K", _c_i32), ("n_leaves", _c_i32), ("G", _c_i32), ("T", _c_i32), ("KP", _c_i32),
                ("tail", _c_i32), ("tail_row", _c_i32), ("n_rounds", _c_i32), ("wide", _c_i32), ("tiers", _c_i32),
                ("leaf_start", _c_i32 * MAX_WIDE_LEAVES), ("leaf_len", _c_i32 * MAX_WIDE_LEAVES),
                ("rounds", (_c_i32 * MAX_LEAVES) * MAX_ROUNDS),
                ("comb_dst", _c_i32 * MAX_WIDE_LEAVES), ("comb_src", _c_i32 * MAX_WIDE_LEAVES),
                ("topic_pos", _c_i32 * MAX_KP), ("pos_topic", _c_i32 * MAX_KP),
                ("pos_lane", _c_i32 * MAX_KP), ("pos_slot", _c_i32 * MAX_KP)]


class LldaFoldinArgs(ctypes.Structure):
    """struct llda_foldin_args (include/llda_gibbs.h)."""
    _fields_ = [("doc_off", _c_p), ("word", _c_p), ("init_idx", _c_p), ("freq", _c_p), ("ph", _c_p),
                ("init_rows", _c_p), ("slot_valid", _c_p), ("z", _c_p), ("n_dk", _c_p), ("th", _c_p),
                ("status", _c_p), ("D", _c_i64), ("doc_base", _c_i64), ("K", _c_i32), ("iters", _c_i32),
                ("thinning", _c_i32), ("beta_fallback", _c_i32), ("avg_mode", _c_i32), ("exact_only", _c_i32),
                ("alpha", _c_d), ("beta", _c_d), ("c_init", _c_d), ("c_loop", _c_d), ("seed", _c_u64),
                ("stream_id", _c_u32), ("reserved2", _c_u32), ("doc_ids", _c_p), ("n_sites", _c_i64),
                ("ph_base", _c_p), ("doc_stream", _c_p)]


class LldaSweepArgs(ctypes.Structure):
    """struct llda_sweep_args (include/llda_gibbs.h)."""
    _fields_ = [("doc_off", _c_p), ("doc_order", _c_p), ("word", _c_p), ("freq", _c_p), ("z", _c_p),
                ("lab_mask", _c_p), ("n_dk", _c_p), ("n_kw", _c_p), ("n_kw_delta", _c_p),
                ("n_k", _c_p), ("n_k_delta", _c_p), ("status", _c_p),
                ("D", _c_i64), ("V", _c_i64), ("K", _c_i32), ("docs_per_group", _c_i32),
                ("dense_mask", _c_i32), ("debug_margin", _c_i32), ("alpha", _c_d), ("beta", _c_d), ("seed", _c_u64), ("sweep", _c_u32),
                ("stream_id", _c_u32), ("doc_base", _c_i64),
                ("live_off", _c_p), ("live_pos", _c_p), ("scratch", _c_p), ("scratch_bytes", _c_i64),
                ("live_max", _c_i32), ("max_doc_tokens", _c_i32), ("csc_pos", _c_p), ("commit_log", _c_p),
                ("n_sites", _c_i64), ("site_rec", _c_p), ("n_kw16", _c_p), ("site_row", _c_p),
                ("n_kw_img", _c_p), ("img_bits", _c_i32), ("reserved_img", _c_i32), ("row16", _c_p), ("img_col", _c_p)]


class LldaBatchArgs(ctypes.Structure):
    """struct llda_batch_args (include/llda_gibbs.h)."""
    _fields_ = [("inst_off", _c_p), ("order", _c_p), ("n_inst", _c_i64), ("word", _c_p), ("freq", _c_p), ("z", _c_p),
                ("inst_prob", _c_p), ("inst_doc", _c_p), ("live_off", _c_p), ("live_pos", _c_p), ("ndk_off", _c_p),
                ("n_dk", _c_p), ("kw_off", _c_p), ("nk_off", _c_p), ("kp", _c_p), ("prob_stream", _c_p), ("k", _c_p), ("counts", _c_p),
                ("delta", _c_p),
                ("status", _c_p), ("V", _c_i64), ("lanes", _c_i32), ("debug_margin", _c_i32), ("alpha", _c_d),
                ("beta", _c_d), ("seed", _c_u64), ("sweep", _c_u32), ("reserved", _c_u32)]


class LldaRankArgs(ctypes.Structure):
    """struct llda_rank_args (include/llda_gibbs.h)."""
    _fields_ = [("score", _c_p), ("truth", _c_p), ("D", _c_i64), ("ld", _c_i64), ("K", _c_i32), ("first", _c_i32),
                ("top_n", _c_i32), ("reserved", _c_i32), ("top_idx", _c_p), ("top_val", _c_p), ("n_thr", _c_p), ("auc", _c_p),
                ("f1", _c_p), ("hit_rank", _c_p), ("flags", _c_p)]


class LldaHeldoutArgs(ctypes.Structure):
    """struct llda_heldout_args (include/llda_gibbs.h)."""
    _fields_ = [("doc_off", _c_p), ("word", _c_p), ("freq", _c_p), ("theta", _c_p), ("phi_t", _c_p), ("D", _c_i64), ("V", _c_i64),
                ("ld_theta", _c_i64), ("ld_phi", _c_i64), ("K", _c_i32), ("reserved", _c_i32), ("mant", _c_p), ("expo", _c_p),
                ("tok", _c_p), ("bad", _c_p)]


class LldaAttrArgs(ctypes.Structure):
    """struct llda_attr_args (include/llda_gibbs.h)."""
    _fields_ = [("doc_off", _c_p), ("word", _c_p), ("freq", _c_p), ("theta", _c_p), ("phi_t", _c_p), ("D", _c_i64), ("V", _c_i64),
                ("ld_theta", _c_i64), ("ld_phi", _c_i64), ("ld_out", _c_i64), ("ld_credit", _c_i64), ("K", _c_i32), ("iters", _c_i32),
                ("top_m", _c_i32), ("reserved", _c_i32), ("alpha", _c_d), ("theta_out", _c_p), ("credit", _c_p), ("site_idx", _c_p),
                ("site_val", _c_p), ("tok", _c_p), ("bad", _c_p)]


class LldaLeftrightArgs(ctypes.Structure):
    """struct llda_leftright_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("R", _c_i32), ("max_doc_tokens", _c_i32), ("doc_off", _c_p), ("word", _c_p),
                ("phi_t", _c_p), ("allowed", _c_p), ("doc_ids", _c_p), ("D", _c_i64), ("V", _c_i64), ("ld_phi", _c_i64),
                ("ld_allowed", _c_i64), ("doc_base", _c_i64), ("alpha", _c_d), ("seed", _c_u64), ("stream_id", _c_u32),
                ("reserved", _c_u32), ("mant", _c_p), ("expo", _c_p), ("tok", _c_p), ("bad", _c_p), ("status", _c_p)]


class LldaNearestArgs(ctypes.Structure):
    """struct llda_nearest_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("L", _c_i32), ("n", _c_i32), ("chunks", _c_i32), ("a", _c_p), ("b", _c_p), ("exclude", _c_p),
                ("Q", _c_i64), ("D", _c_i64), ("lda", _c_i64), ("ldb", _c_i64), ("row_base", _c_i64), ("top_idx", _c_p),
                ("top_val", _c_p), ("n_nan", _c_p), ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaLabelArgs(ctypes.Structure):
    """struct llda_label_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("first", _c_i32), ("n_labels", _c_i32), ("chunk", _c_i32), ("reserved", _c_i32),
                ("score", _c_p), ("truth", _c_p), ("D", _c_i64), ("ld", _c_i64), ("n_pos", _c_p), ("n_thr", _c_p), ("auc_num", _c_p),
                ("auc", _c_p), ("thr_tp", _c_p), ("thr_fp", _c_p), ("f1", _c_p), ("thr", _c_p), ("flags", _c_p), ("order", _c_p),
                ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaSetsArgs(ctypes.Structure):
    """struct llda_sets_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("first", _c_i32), ("at_least_one", _c_i32), ("score", _c_p), ("thr", _c_p),
                ("truth", _c_p), ("D", _c_i64), ("ld", _c_i64), ("mask", _c_p), ("n_pred", _c_p), ("n_hit", _c_p), ("n_true", _c_p),
                ("tp", _c_p), ("fp", _c_p), ("fn", _c_p)]


class LldaScoredArgs(ctypes.Structure):
    """struct llda_scored_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("n", _c_i32), ("a", _c_i32), ("n_kw", _c_p), ("n_k", _c_p), ("den", _c_p),
                ("mat", _c_p), ("wdiv", _c_p), ("V", _c_i64), ("ld", _c_i64), ("beta", _c_d), ("top_idx", _c_p), ("top_score", _c_p),
                ("n_nan", _c_p), ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaEcdfArgs(ctypes.Structure):
    """struct llda_ecdf_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("first", _c_i32), ("n_labels", _c_i32), ("chunk", _c_i32), ("mode", _c_i32),
                ("mat", _c_p), ("cand", _c_p), ("V", _c_i64), ("ld", _c_i64), ("rank", _c_p), ("value", _c_p), ("n_cand", _c_p),
                ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaFrexArgs(ctypes.Structure):
    """struct llda_frex_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("n_labels", _c_i32), ("n", _c_i32), ("m", _c_i32), ("s", _c_i32), ("t", _c_i32),
                ("rank_f", _c_p), ("rank_e", _c_p), ("probe", _c_p), ("V", _c_i64), ("Vc", _c_i64), ("top_idx", _c_p),
                ("top_rank_f", _c_p), ("top_rank_e", _c_p), ("probe_rank_f", _c_p), ("probe_rank_e", _c_p), ("scratch", _c_p),
                ("scratch_bytes", _c_i64)]


class LldaWcreditArgs(ctypes.Structure):
    """struct llda_wcredit_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("chunk", _c_i32), ("reserved", _c_i32), ("word_off", _c_p), ("site_doc", _c_p),
                ("freq", _c_p), ("theta", _c_p), ("phi_t", _c_p), ("D", _c_i64), ("V", _c_i64), ("S", _c_i64), ("ld_theta", _c_i64),
                ("ld_phi", _c_i64), ("ld_credit", _c_i64), ("credit_w", _c_p), ("tok", _c_p), ("bad", _c_p), ("scratch", _c_p),
                ("scratch_bytes", _c_i64)]


class LldaPhistepArgs(ctypes.Structure):
    """struct llda_phistep_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("cw", _c_p), ("phi_t_out", _c_p), ("den", _c_p), ("V", _c_i64), ("ld", _c_i64),
                ("ld_out", _c_i64), ("beta", _c_d), ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaAttrSparseArgs(ctypes.Structure):
    """struct llda_attr_sparse_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("max_labels", _c_i32), ("iters", _c_i32), ("top_m", _c_i32), ("reserved", _c_i32),
                ("doc_off", _c_p), ("word", _c_p), ("freq", _c_p), ("lab_off", _c_p), ("lab", _c_p), ("theta_s", _c_p), ("phi_t", _c_p),
                ("D", _c_i64), ("V", _c_i64), ("NL", _c_i64), ("ld_phi", _c_i64), ("alpha", _c_d), ("theta_out", _c_p), ("credit", _c_p),
                ("site_idx", _c_p), ("site_val", _c_p), ("tok", _c_p), ("bad", _c_p)]


class LldaWcreditSparseArgs(ctypes.Structure):
    """struct llda_wcredit_sparse_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("chunk", _c_i32), ("max_labels", _c_i32), ("word_off", _c_p), ("site_doc", _c_p),
                ("freq", _c_p), ("lab_off", _c_p), ("lab", _c_p), ("theta_s", _c_p), ("phi_t", _c_p), ("D", _c_i64), ("V", _c_i64),
                ("S", _c_i64), ("NL", _c_i64), ("ld_phi", _c_i64), ("ld_credit", _c_i64), ("credit_w", _c_p), ("tok", _c_p), ("bad", _c_p),
                ("scratch", _c_p), ("scratch_bytes", _c_i64)]


class LldaHeldoutSparseArgs(ctypes.Structure):
    """struct llda_heldout_sparse_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("max_labels", _c_i32), ("reserved", _c_i32), ("doc_off", _c_p), ("word", _c_p),
                ("freq", _c_p), ("lab_off", _c_p), ("lab", _c_p), ("theta_s", _c_p), ("phi_t", _c_p), ("D", _c_i64), ("V", _c_i64),
                ("NL", _c_i64), ("ld_phi", _c_i64), ("mant", _c_p), ("expo", _c_p), ("tok", _c_p), ("bad", _c_p)]


class LldaLeftrightSparseArgs(ctypes.Structure):
    """struct llda_leftright_sparse_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("R", _c_i32), ("max_doc_tokens", _c_i32), ("doc_off", _c_p), ("word", _c_p),
                ("phi_t", _c_p), ("lab_off", _c_p), ("lab", _c_p), ("doc_ids", _c_p), ("D", _c_i64), ("V", _c_i64), ("ld_phi", _c_i64),
                ("NL", _c_i64), ("doc_base", _c_i64), ("alpha", _c_d), ("seed", _c_u64), ("stream_id", _c_u32), ("max_labels", _c_i32),
                ("mant", _c_p), ("expo", _c_p), ("tok", _c_p), ("bad", _c_p), ("status", _c_p)]


class LldaFoldinSparseArgs(ctypes.Structure):
    """struct llda_foldin_sparse_args (include/llda_gibbs.h)."""
    _fields_ = [("struct_bytes", _c_u32), ("K", _c_i32), ("max_labels", _c_i32), ("iters", _c_i32), ("thinning", _c_i32),
                ("stream_id", _c_u32), ("doc_off", _c_p), ("word", _c_p), ("freq", _c_p), ("phi_t", _c_p), ("lab_off", _c_p), ("lab", _c_p),
                ("doc_ids", _c_p), ("D", _c_i64), ("V", _c_i64), ("NL", _c_i64), ("ld_phi", _c_i64), ("doc_base", _c_i64), ("alpha", _c_d),
                ("c_init", _c_d), ("c_loop", _c_d), ("seed", _c_u64), ("z", _c_p), ("n_dk_s", _c_p), ("th_s", _c_p), ("status", _c_p)]


EXPORTS = ("llda_abi_version", "llda_build_info", "llda_strerror", "llda_last_hip_error", "llda_struct_size", "llda_layout_init",
           "llda_sweep_scratch_bytes", "llda_rows16_ok", "llda_quad_ok", "llda_pack_rows16", "llda_pack_rows16_all", "llda_pack_image", "llda_pack_image_cols",

           "llda_sweep", "llda_sweep_batch", "llda_commit_log", "llda_apply_rows", "llda_apply_delta", "llda_count_init", "llda_loglik", "llda_foldin",
           "llda_readout_phi", "llda_readout_theta", "llda_selftest_div", "llda_count_hist", "llda_rank_labels",
           "llda_top_words_scratch_bytes", "llda_top_words", "llda_word_cooc", "llda_window_cooc", "llda_heldout_loglik", "llda_attribute",
           "llda_leftright_struct_bytes", "llda_left_to_right",
           "llda_nearest_struct_bytes", "llda_nearest_scratch_bytes", "llda_nearest_rows",
           "llda_label_struct_bytes", "llda_label_scratch_bytes", "llda_label_metrics", "llda_sets_struct_bytes", "llda_label_sets",
           "llda_scored_struct_bytes", "llda_scored_words_scratch_bytes", "llda_scored_words",
           "llda_ecdf_struct_bytes", "llda_ecdf_scratch_bytes", "llda_ecdf_ranks",
           "llda_frex_struct_bytes", "llda_frex_scratch_bytes", "llda_frex_select",
           "llda_wcredit_struct_bytes", "llda_credit_words_scratch_bytes", "llda_credit_words",
           "llda_phistep_struct_bytes", "llda_phi_step_scratch_bytes", "llda_phi_step",
           "llda_attr_sparse_struct_bytes", "llda_attribute_sparse",
           "llda_wcredit_sparse_struct_bytes", "llda_credit_words_sparse_scratch_bytes", "llda_credit_words_sparse",
           "llda_heldout_sparse_struct_bytes", "llda_heldout_loglik_sparse",
           "llda_leftright_sparse_struct_bytes", "llda_left_to_right_sparse",
           "llda_foldin_sparse_struct_bytes", "llda_foldin_sparse")

_LIB = None


class NativeError(RuntimeError):
    pass


def lib():
    """Load the HIP library; raise if it is not built (no fallback)."""
    global _LIB
    if _LIB is not None:
        return _LIB
    if not os.path.exists(LIB_PATH):
        raise NativeError("HIP extension %s is missing: run `python -c 'import __graft_entry__ as g; "
                          "g.build()'` (or make -C lda_thesis_amd/csrc). There is no CPU fallback."
                          % LIB_PATH)
    # torch ships its own libamdhip64 / libhsa-runtime64: import it first so this library binds to
    # the SAME HIP runtime instance as the tensors and streams it is handed (loading ours first pulls
    # in /opt/rocm's copy and kernel launches then fail with hipErrorNoDevice).
    import torch  # noqa: F401
    L = ctypes.CDLL(LIB_PATH)
    L.llda_abi_version.restype = ctypes.c_int
    L.llda_abi_version.argtypes = []
    L.llda_build_info.restype = ctypes.c_int
    L.llda_build_info.argtypes = []
    L.llda_strerror.restype = ctypes.c_char_p
    L.llda_strerror.argtypes = [ctypes.c_int]
    L.llda_last_hip_error.restype = ctypes.c_int
    L.llda_last_hip_error.argtypes = []
    L.llda_layout_init.restype = ctypes.c_int
    L.llda_layout_init.argtypes = [_c_i32, ctypes.POINTER(LldaLayout)]
    L.llda_sweep.restype = ctypes.c_int
    L.llda_sweep.argtypes = [ctypes.POINTER(LldaSweepArgs), _c_p]
    L.llda_sweep_scratch_bytes.restype = _c_i64
    L.llda_sweep_scratch_bytes.argtypes = [_c_i32, _c_i64]
    L.llda_rows16_ok.restype = ctypes.c_int
    L.llda_rows16_ok.argtypes = [_c_i32]
    L.llda_quad_ok.restype = ctypes.c_int
    L.llda_quad_ok.argtypes = [_c_i32]
    L.llda_pack_rows16.restype = ctypes.c_int
    L.llda_pack_rows16.argtypes = [_c_p, _c_p, _c_i64, _c_i32, _c_p, _c_p, _c_p]
    L.llda_pack_rows16_all.restype = ctypes.c_int
    L.llda_pack_rows16_all.argtypes = [_c_p, _c_i64, _c_i32, _c_p, _c_p, _c_p]
    L.llda_pack_image_cols.restype = ctypes.c_int
    L.llda_pack_image_cols.argtypes = [_c_p, _c_i64, _c_i32, _c_i32, _c_p, _c_p, _c_p]
    L.llda_pack_image.restype = ctypes.c_int
    L.llda_pack_image.argtypes = [_c_p, _c_i64, _c_i32, _c_p, _c_p]
    L.llda_sweep_batch.restype = ctypes.c_int
    L.llda_sweep_batch.argtypes = [ctypes.POINTER(LldaBatchArgs), _c_p]
    L.llda_commit_log.restype = ctypes.c_int
    L.llda_commit_log.argtypes = [_c_p, _c_p, _c_p, _c_i64, _c_p, _c_p, _c_i32, _c_p, _c_p, _c_p, _c_p, _c_p]
    L.llda_apply_rows.restype = ctypes.c_int
    L.llda_apply_rows.argtypes = [_c_p, _c_p, _c_i64, _c_i32, _c_p, _c_p]
    L.llda_apply_delta.restype = ctypes.c_int
    L.llda_apply_delta.argtypes = [_c_p, _c_p, _c_i64, _c_p]
    L.llda_count_init.restype = ctypes.c_int
    L.llda_count_init.argtypes = [_c_p, _c_p, _c_p, _c_p, _c_i64, _c_i32, _c_p, _c_p, _c_p, _c_p]
    L.llda_count_hist.restype = ctypes.c_int
    L.llda_count_hist.argtypes = [_c_p, _c_i64, _c_i32, _c_p, _c_i32, _c_i32, _c_p, _c_p, _c_i64, _c_p, _c_p]
    L.llda_loglik.restype = ctypes.c_int
    L.llda_loglik.argtypes = [_c_p, _c_p, _c_p, _c_p, _c_p, _c_p, _c_i64, _c_i64, _c_i32, _c_d, _c_d,
                              _c_p, _c_p]
    L.llda_foldin.restype = ctypes.c_int
    L.llda_foldin.argtypes = [ctypes.POINTER(LldaFoldinArgs), _c_p]
    L.llda_readout_phi.restype = ctypes.c_int
    L.llda_readout_phi.argtypes = [_c_p, _c_p, _c_p, _c_i64, _c_i32, _c_d, _c_i32, _c_d, _c_d, _c_p, _c_p, _c_p]
    L.llda_readout_theta.restype = ctypes.c_int
    L.llda_readout_theta.argtypes = [_c_p, _c_p, _c_i64, _c_i32, _c_d, _c_i32, _c_d, _c_d, _c_p, _c_p]
    L.llda_rank_labels.restype = ctypes.c_int
    L.llda_rank_labels.argtypes = [ctypes.POINTER(LldaRankArgs), _c_p]
    L.llda_top_words_scratch_bytes.restype = _c_i64
    L.llda_top_words_scratch_bytes.argtypes = [_c_i64, _c_i32, _c_i32]
    L.llda_top_words.restype = ctypes.c_int
    L.llda_top_words.argtypes = [_c_p, _c_i64, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_i64, _c_p]
    L.llda_word_cooc.restype = ctypes.c_int
    L.llda_word_cooc.argtypes = [_c_p, _c_p, _c_i64, _c_i64, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p]
    L.llda_window_cooc.restype = ctypes.c_int
    L.llda_window_cooc.argtypes = [_c_p, _c_p, _c_i64, _c_i64, _c_i32, _c_i32, _c_i32, _c_p, _c_p, _c_p, _c_p]
    L.llda_heldout_loglik.restype = ctypes.c_int
    L.llda_heldout_loglik.argtypes = [ctypes.POINTER(LldaHeldoutArgs), _c_p]
    L.llda_attribute.restype = ctypes.c_int
    L.llda_attribute.argtypes = [ctypes.POINTER(LldaAttrArgs), _c_p]
    L.llda_leftright_struct_bytes.restype = ctypes.c_int
    L.llda_leftright_struct_bytes.argtypes = []
    L.llda_left_to_right.restype = ctypes.c_int
    L.llda_left_to_right.argtypes = [ctypes.POINTER(LldaLeftrightArgs), _c_p]
    L.llda_nearest_struct_bytes.restype = ctypes.c_int
    L.llda_nearest_struct_bytes.argtypes = []
    L.llda_nearest_scratch_bytes.restype = _c_i64
    L.llda_nearest_scratch_bytes.argtypes = [_c_i64, _c_i64, _c_i32, _c_i32]
    L.llda_nearest_rows.restype = ctypes.c_int
    L.llda_nearest_rows.argtypes = [ctypes.POINTER(LldaNearestArgs), _c_p]
    L.llda_label_struct_bytes.restype = ctypes.c_int
    L.llda_label_struct_bytes.argtypes = []
    L.llda_label_scratch_bytes.restype = _c_i64
    L.llda_label_scratch_bytes.argtypes = [_c_i64, _c_i32, _c_i32]
    L.llda_label_metrics.restype = ctypes.c_int
    L.llda_label_metrics.argtypes = [ctypes.POINTER(LldaLabelArgs), _c_p]
    L.llda_sets_struct_bytes.restype = ctypes.c_int
    L.llda_sets_struct_bytes.argtypes = []
    L.llda_label_sets.restype = ctypes.c_int
    L.llda_label_sets.argtypes = [ctypes.POINTER(LldaSetsArgs), _c_p]
    L.llda_scored_struct_bytes.restype = ctypes.c_int
    L.llda_scored_struct_bytes.argtypes = []
    L.llda_scored_words_scratch_bytes.restype = _c_i64
    L.llda_scored_words_scratch_bytes.argtypes = [_c_i64, _c_i32, _c_i32]
    L.llda_scored_words.restype = ctypes.c_int
    L.llda_scored_words.argtypes = [ctypes.POINTER(LldaScoredArgs), _c_p]
    L.llda_ecdf_struct_bytes.restype = ctypes.c_int
    L.llda_ecdf_struct_bytes.argtypes = []
    L.llda_ecdf_scratch_bytes.restype = _c_i64
    L.llda_ecdf_scratch_bytes.argtypes = [_c_i64, _c_i32, _c_i32]
    L.llda_ecdf_ranks.restype = ctypes.c_int
    L.llda_ecdf_ranks.argtypes = [ctypes.POINTER(LldaEcdfArgs), _c_p]
    L.llda_frex_struct_bytes.restype = ctypes.c_int
    L.llda_frex_struct_bytes.argtypes = []
    L.llda_frex_scratch_bytes.restype = _c_i64
    L.llda_frex_scratch_bytes.argtypes = [_c_i64, _c_i32, _c_i32]
    L.llda_frex_select.restype = ctypes.c_int
    L.llda_frex_select.argtypes = [ctypes.POINTER(LldaFrexArgs), _c_p]
    L.llda_wcredit_struct_bytes.restype = ctypes.c_int
    L.llda_wcredit_struct_bytes.argtypes = []
    L.llda_credit_words_scratch_bytes.restype = _c_i64
    L.llda_credit_words_scratch_bytes.argtypes = [_c_i64, _c_i64, _c_i32, _c_i32]
    L.llda_credit_words.restype = ctypes.c_int
    L.llda_credit_words.argtypes = [ctypes.POINTER(LldaWcreditArgs), _c_p]
    L.llda_phistep_struct_bytes.restype = ctypes.c_int
    L.llda_phistep_struct_bytes.argtypes = []
    L.llda_phi_step_scratch_bytes.restype = _c_i64
    L.llda_phi_step_scratch_bytes.argtypes = [_c_i64, _c_i32]
    L.llda_phi_step.restype = ctypes.c_int
    L.llda_phi_step.argtypes = [ctypes.POINTER(LldaPhistepArgs), _c_p]
    L.llda_attr_sparse_struct_bytes.restype = ctypes.c_int
    L.llda_attr_sparse_struct_bytes.argtypes = []
    L.llda_attribute_sparse.restype = ctypes.c_int
    L.llda_attribute_sparse.argtypes = [ctypes.POINTER(LldaAttrSparseArgs), _c_p]
    L.llda_wcredit_sparse_struct_bytes.restype = ctypes.c_int
    L.llda_wcredit_sparse_struct_bytes.argtypes = []
    L.llda_credit_words_sparse_scratch_bytes.restype = _c_i64
    L.llda_credit_words_sparse_scratch_bytes.argtypes = [_c_i64, _c_i64, _c_i32, _c_i32]
    L.llda_credit_words_sparse.restype = ctypes.c_int
    L.llda_credit_words_sparse.argtypes = [ctypes.POINTER(LldaWcreditSparseArgs), _c_p]
    L.llda_heldout_sparse_struct_bytes.restype = ctypes.c_int
    L.llda_heldout_sparse_struct_bytes.argtypes = []
    L.llda_heldout_loglik_sparse.restype = ctypes.c_int
    L.llda_heldout_loglik_sparse.argtypes = [ctypes.POINTER(LldaHeldoutSparseArgs), _c_p]
    L.llda_leftright_sparse_struct_bytes.restype = ctypes.c_int
    L.llda_leftright_sparse_struct_bytes.argtypes = []
    L.llda_left_to_right_sparse.restype = ctypes.c_int
    L.llda_left_to_right_sparse.argtypes = [ctypes.POINTER(LldaLeftrightSparseArgs), _c_p]
    L.llda_foldin_sparse_struct_bytes.restype = ctypes.c_int
    L.llda_foldin_sparse_struct_bytes.argtypes = []
    L.llda_foldin_sparse.restype = ctypes.c_int
    L.llda_foldin_sparse.argtypes = [ctypes.POINTER(LldaFoldinSparseArgs), _c_p]
    L.llda_selftest_div.restype = ctypes.c_int
    L.llda_selftest_div.argtypes = [_c_u64, _c_i64, _c_p, _c_p]
    if L.llda_abi_version() != ABI_VERSION:
        raise NativeError("libllda_gibbs.so ABI %d != binding ABI %d" % (L.llda_abi_version(), ABI_VERSION))
    L.llda_struct_size.restype = ctypes.c_int
    L.llda_struct_size.argtypes = [ctypes.c_int]
    for which, struct in enumerate((LldaLayout, LldaSweepArgs, LldaBatchArgs, LldaFoldinArgs, LldaRankArgs, LldaHeldoutArgs,
                                    LldaAttrArgs)):
        if L.llda_struct_size(which) != ctypes.sizeof(struct):
            raise NativeError("%s: binding has %d bytes, the library %d" % (struct.__name__, ctypes.sizeof(struct),
                                                                           L.llda_struct_size(which)))
    if L.llda_leftright_struct_bytes() != ctypes.sizeof(LldaLeftrightArgs):
        raise NativeError("LldaLeftrightArgs: binding has %d bytes, the library %d" % (ctypes.sizeof(LldaLeftrightArgs),
                                                                                       L.llda_leftright_struct_bytes()))
    if L.llda_nearest_struct_bytes() != ctypes.sizeof(LldaNearestArgs):
        raise NativeError("LldaNearestArgs: binding has %d bytes, the library %d" % (ctypes.sizeof(LldaNearestArgs),
                                                                                     L.llda_nearest_struct_bytes()))
    for name, struct, size in (("LldaLabelArgs", LldaLabelArgs, L.llda_label_struct_bytes()), ("LldaSetsArgs", LldaSetsArgs, L.llda_sets_struct_bytes()),
                               ("LldaScoredArgs", LldaScoredArgs, L.llda_scored_struct_bytes()),
                               ("LldaEcdfArgs", LldaEcdfArgs, L.llda_ecdf_struct_bytes()), ("LldaFrexArgs", LldaFrexArgs, L.llda_frex_struct_bytes()),
                               ("LldaWcreditArgs", LldaWcreditArgs, L.llda_wcredit_struct_bytes()),
                               ("LldaPhistepArgs", LldaPhistepArgs, L.llda_phistep_struct_bytes()),
                               ("LldaAttrSparseArgs", LldaAttrSparseArgs, L.llda_attr_sparse_struct_bytes()),
                               ("LldaWcreditSparseArgs", LldaWcreditSparseArgs, L.llda_wcredit_sparse_struct_bytes()),
                               ("LldaHeldoutSparseArgs", LldaHeldoutSparseArgs, L.llda_heldout_sparse_struct_bytes()),
                               ("LldaLeftrightSparseArgs", LldaLeftrightSparseArgs, L.llda_leftright_sparse_struct_bytes()),
                               ("LldaFoldinSparseArgs", LldaFoldinSparseArgs, L.llda_foldin_sparse_struct_bytes())):
        if size != ctypes.sizeof(struct):
            raise NativeError("%s: binding has %d bytes, the library %d" % (name, ctypes.sizeof(struct), size))
    _LIB = L
    return L


BUILD_SWITCHES = ("LLDA_MARGIN0", "LLDA_WAVES", "LLDA_MARGIN0_WIDE", "ABL_NOLOAD", "ABL_NOCOMMIT", "ABL_WIDE_NOROW",
                  "ABL_WIDE_NOADDLOAD", "ABL_NOFMA", "ABL_EXTRA_LDS_BYTES", "QUAD_PROFILE", "LLDA_BUDGET_MARKS", "LLDA_QUAD_PRIO")      # bit i of llda_build_info()


def build_info():
    """llda_build_info: (bits, names of the compile-time switches the loaded library was built with); (0, []) = production."""
    bits = int(lib().llda_build_info())
    return bits, [n for i, n in enumerate(BUILD_SWITCHES) if bits >> i & 1]


def require_device():
    """Raise unless a HIP device is visible (the product has no CPU path)."""
    import torch
    if not torch.cuda.is_available():
        raise NativeError("no HIP device visible: the sampler has no CPU fallback")


def check(rc, what):
    if rc != 0:
        L = lib()
        raise NativeError("%s failed: %s (code %d, hipError %d)"
                          % (what, L.llda_strerror(rc).decode(), rc, L.llda_last_hip_error()))


def layout_init(K):
    """llda_layout_init -> dict of numpy arrays / ints (host only, needs no device)."""
    out = LldaLayout()
    check(lib().llda_layout_init(int(K), ctypes.byref(out)), "llda_layout_init(K=%d)" % K)
    return dict(K=out.K, n_leaves=out.n_leaves, G=out.G, T=out.T, KP=out.KP, tail=out.tail,
                tail_row=out.tail_row, n_rounds=out.n_rounds, wide=out.wide, tiers=out.tiers,
                comb=[(out.comb_dst[i], out.comb_src[i]) for i in range(out.n_leaves - 1)],
                leaf_start=np.array(out.leaf_start[:out.n_leaves]),
                leaf_len=np.array(out.leaf_len[:out.n_leaves]),
                rounds=np.array([list(r) for r in out.rounds])[:out.n_rounds],
                topic_pos=np.array(out.topic_pos[:out.K], dtype=np.int32),
                pos_topic=np.array(out.pos_topic[:out.KP], dtype=np.int32),
                pos_lane=np.array(out.pos_lane[:out.KP], dtype=np.int32),
                pos_slot=np.array(out.pos_slot[:out.KP], dtype=np.int32))


def _ptr(t):
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _launch(ref, fn, what, *args):
    """call the enqueue-only entry point ``fn(*args, stream)`` on the device that holds the tensor ``ref``: that
    device is made current for the call and the stream is torch's current stream OF THAT DEVICE (not of whichever
    device happens to be current), so the kernels are ordered with the torch ops on the tensors they touch."""
    import torch
    dev = ref.device
    with torch.cuda.device(dev):
        check(fn(*args, ctypes.c_void_p(torch.cuda.current_stream(dev).cuda_stream)), what)


def sweep(*, doc_off, doc_order, word, freq, z, lab_mask, n_dk, n_kw, n_kw_delta, n_k, n_k_delta,
          status, D, V, K, alpha, beta, seed, sweep, stream_id=0, doc_base=0, docs_per_group=0,
          dense_mask=False, debug_margin=0, live_off=None, live_pos=None, live_max=0, csc_pos=None, commit_log=None,
          n_sites=None, site_rec=None, max_doc_tokens=0, scratch=None, n_kw16=None, site_row=None, n_kw_img=None, row16=None,
          img_col=None):
    """llda_sweep on the current torch stream.  All array arguments are torch CUDA tensors.  n_sites = the sites
    the D documents span (default: all of ``word``); scratch = a uint8 tensor of sweep_scratch_bytes(K, D) bytes (wide
    layouts) or None; n_kw16 = the 16-bit image written by pack_rows16 (then csc_pos carries the row flags in bit 31 and site_row the row starts) or None;
    n_kw_img = the saturating uint8 / int16 image written by pack_image (sparse label sets) or None; row16 = the per-word flags
    written by pack_rows16_all (with n_kw16, without site_row: the four-documents-per-wavefront kernel of K = 512) or None."""
    img_bits = 0 if n_kw_img is None else 8 * n_kw_img.element_size()
    a = LldaSweepArgs(_ptr(doc_off), _ptr(doc_order), _ptr(word), _ptr(freq), _ptr(z), _ptr(lab_mask),
                      _ptr(n_dk), _ptr(n_kw), _ptr(n_kw_delta), _ptr(n_k), _ptr(n_k_delta), _ptr(status),
                      int(D), int(V), int(K), int(docs_per_group), 1 if dense_mask else 0, int(debug_margin),
                      float(alpha), float(beta),
                      int(seed) & 0xFFFFFFFFFFFFFFFF, int(sweep) & 0xFFFFFFFF,
                      int(stream_id) & 0xFFFFFFFF, int(doc_base), _ptr(live_off), _ptr(live_pos), _ptr(scratch),
                      0 if scratch is None else int(scratch.numel() * scratch.element_size()), int(live_max), int(max_doc_tokens),
                      _ptr(csc_pos), _ptr(commit_log), int(word.numel() if n_sites is None else n_sites), _ptr(site_rec),
                      _ptr(n_kw16), _ptr(site_row), _ptr(n_kw_img), img_bits, 0, _ptr(row16), _ptr(img_col))
    _launch(z, lib().llda_sweep, "llda_sweep", ctypes.byref(a))


def sweep_scratch_bytes(K, D):
    """llda_sweep_scratch_bytes: bytes of work space that let llda_sweep take its fastest kernel (0: none needed)."""
    return int(lib().llda_sweep_scratch_bytes(int(K), int(D)))


def rows16_ok(K):
    """llda_rows16_ok: can llda_sweep read 16-bit rows for K topics?"""
    return bool(lib().llda_rows16_ok(int(K)))


def quad_ok(K):
    """llda_quad_ok: does llda_sweep take the per-sweep row flags (llda_sweep_args.row16: K / 32 lanes x 32 slots per document)?"""
    return bool(lib().llda_quad_ok(int(K)))


def pack_rows16(n_kw, row16, K, n_kw16, status):
    """llda_pack_rows16 on the current torch stream: the 16-bit image of the rows of n_kw flagged in row16 (uint8 [V])."""
    _launch(n_kw, lib().llda_pack_rows16, "llda_pack_rows16", _ptr(n_kw), _ptr(row16), int(row16.numel()), int(K),
            _ptr(n_kw16), _ptr(status))


def pack_rows16_all(n_kw, K, n_kw16, row16):
    """llda_pack_rows16_all on the current torch stream: the 16-bit image of EVERY row of n_kw and, in row16 (uint8 [V]), whether
    all counts of the row fit 16 bits."""
    _launch(n_kw, lib().llda_pack_rows16_all, "llda_pack_rows16_all", _ptr(n_kw), int(row16.numel()), int(K), _ptr(n_kw16), _ptr(row16))


def pack_image_cols(n_kw, K, col_src, img):
    """llda_pack_image_cols: the saturating image with its columns in the order col_src (int32 [KP] on the device)."""
    _launch(n_kw, lib().llda_pack_image_cols, "llda_pack_image_cols", _ptr(n_kw), int(n_kw.shape[0]), int(K), 8 * img.element_size(),
            _ptr(col_src), _ptr(img))


def pack_image(n_kw, img):
    """llda_pack_image on the current torch stream: img (uint8 or int16, as many elements as n_kw) = n_kw saturated at 255 / 65535."""
    _launch(n_kw, lib().llda_pack_image, "llda_pack_image", _ptr(n_kw), int(n_kw.numel()), 8 * img.element_size(), _ptr(img))


def sweep_batch(*, inst_off, order, word, freq, z, inst_prob, inst_doc, live_off, live_pos, ndk_off, n_dk, kw_off,
                nk_off, kp, prob_stream, k, counts, delta, status, V, lanes, alpha, beta, seed, sweep, debug_margin=0):
    """llda_sweep_batch on the current torch stream: one sweep of the instances in ``order`` (each with at most
    ``lanes`` allowed topics) of an ensemble of small problems."""
    a = LldaBatchArgs(_ptr(inst_off), _ptr(order), int(order.numel()), _ptr(word), _ptr(freq), _ptr(z),
                      _ptr(inst_prob), _ptr(inst_doc), _ptr(live_off), _ptr(live_pos), _ptr(ndk_off), _ptr(n_dk),
                      _ptr(kw_off), _ptr(nk_off), _ptr(kp), _ptr(prob_stream), _ptr(k), _ptr(counts), _ptr(delta), _ptr(status), int(V),
                      int(lanes), int(debug_margin), float(alpha), float(beta), int(seed) & 0xFFFFFFFFFFFFFFFF,
                      int(sweep) & 0xFFFFFFFF, 0)
    _launch(z, lib().llda_sweep_batch, "llda_sweep_batch", ctypes.byref(a))


def commit_log(item_begin, item_len, item_word, commit_log, freq_csc, K, target, n_k=None, n_k_delta=None,
               row_off=None):
    """llda_commit_log: fold the word-major commit log of a sweep into ``target`` (n_kw, its delta buffer, or --
    with ``row_off`` -- the exchange rows, int16 pairs where the offset is negative)."""
    _launch(target, lib().llda_commit_log, "llda_commit_log", _ptr(item_begin), _ptr(item_len), _ptr(item_word),
            int(item_len.numel()), _ptr(commit_log), _ptr(freq_csc), int(K), _ptr(row_off), _ptr(target), _ptr(n_k),
            _ptr(n_k_delta))


def apply_rows(row_off, rows, K, counts):
    """llda_apply_rows: counts[r] += row r of the exchange rows (pairs decoded), rows cleared."""
    _launch(rows, lib().llda_apply_rows, "llda_apply_rows", _ptr(row_off), _ptr(rows), int(row_off.numel()), int(K),
            _ptr(counts))


def apply_delta(counts, delta):
    _launch(counts, lib().llda_apply_delta, "llda_apply_delta", _ptr(counts), _ptr(delta), counts.numel())


def count_init(doc_off, word, freq, z, D, K, n_dk, n_kw, n_k):
    _launch(n_kw, lib().llda_count_init, "llda_count_init", _ptr(doc_off), _ptr(word), _ptr(freq), _ptr(z), int(D), int(K),
            _ptr(n_dk), _ptr(n_kw), _ptr(n_k))


def count_hist(counts, K, lab_mask, mask_per_row, hist, over_val, over_n, over_cap=None):
    """llda_count_hist on the current torch stream: hist (int64 [n_bins]) += how many allowed entries of ``counts`` (int32 (rows, KP),
    device order) hold every value; values outside 0 .. n_bins-1 are appended to over_val (int32 [over_cap]) and counted in over_n
    (int64 [1]).  lab_mask: the lane masks of the rows ((rows, G), mask_per_row=True) or one mask row ((G,), False); over_cap: how
    many values over_val may take (default: all it holds)."""
    _launch(hist, lib().llda_count_hist, "llda_count_hist", _ptr(counts), int(counts.shape[0]), int(K), _ptr(lab_mask), 1 if mask_per_row else 0,
            int(hist.numel()), _ptr(hist), _ptr(over_val), int(over_val.numel() if over_cap is None else over_cap), _ptr(over_n))


RANK_NO_POSITIVE, RANK_NO_NEGATIVE, RANK_ONE_THRESHOLD, RANK_ALL_ZERO, RANK_NAN = 1, 2, 4, 8, 16
RANK_MAX_TOP_N = 16


def rank_labels(score, truth, D, K, first, top_n, *, ld=None, top_idx=None, top_val=None, n_thr=None, auc=None, f1=None,
                hit_rank=None, flags=None):
    """llda_rank_labels on the current torch stream: score (D, ld) float64 in reference topic order, truth (D, K) uint8 or None;
    every output tensor may be None."""
    a = LldaRankArgs(_ptr(score), _ptr(truth), int(D), int(score.stride(0) if ld is None else ld), int(K), int(first), int(top_n), 0,
                     _ptr(top_idx), _ptr(top_val), _ptr(n_thr), _ptr(auc), _ptr(f1), _ptr(hit_rank), _ptr(flags))
    _launch(score, lib().llda_rank_labels, "llda_rank_labels", ctypes.byref(a))


TOPW_MAX_N = 16
TOPW_CHUNK_ROWS = 256   # LLDA_TOPW_CHUNK_ROWS: llda_top_words cuts the vocabulary into chunks of so many words
COOC_MAX_WAVES = 8192   # LLDA_COOC_MAX_WAVES: wavefront i of llda_word_cooc takes the documents i, i + 8192, ... in turn ...
COOC_AGG_MIN_DOCS = 32768   # ... LLDA_COOC_AGG_MIN_DOCS: in calls of fewer documents; larger calls count in LDS first


def top_words_scratch_bytes(V, K, n):
    """llda_top_words_scratch_bytes: bytes of work space llda_top_words needs (host only)."""
    r = int(lib().llda_top_words_scratch_bytes(int(V), int(K), int(n)))
    if r < 0:
        check(r, "llda_top_words_scratch_bytes(V=%d, K=%d, n=%d)" % (V, K, n))
    return r


def top_words(n_kw, V, K, n, top_idx, top_cnt, scratch):
    """llda_top_words on the current torch stream: top_idx / top_cnt (K, n) int32 (either may be None) = the n words of every
    topic with the largest counts in n_kw (int32 (V, KP), device order), ties by word id ascending; scratch = a uint8 tensor of
    top_words_scratch_bytes(V, K, n) bytes."""
    _launch(n_kw, lib().llda_top_words, "llda_top_words", _ptr(n_kw), int(V), int(K), int(n), _ptr(top_idx), _ptr(top_cnt),
            _ptr(scratch), int(scratch.numel() * scratch.element_size()))


SCORED_MAX_A = 8        # llda_scored_args.a: the largest power


def scored_words_scratch_bytes(V, K, n):
    """llda_scored_words_scratch_bytes: bytes of work space llda_scored_words needs for either source (host only)."""
    r = int(lib().llda_scored_words_scratch_bytes(int(V), int(K), int(n)))
    if r < 0:
        check(r, "llda_scored_words_scratch_bytes(V=%d, K=%d, n=%d)" % (V, K, n))
    return r


def scored_words(V, K, n, a, scratch, *, n_kw=None, n_k=None, den=None, beta=0.0, mat=None, ld=None, wdiv=None, top_idx=None,
                 top_score=None, n_nan=None):
    """llda_scored_words on the current torch stream: the n words of every topic with the best P_a(x) / wdiv.  x comes from n_kw
    (int32 (V, KP), device order, with beta and n_k (int32 [KP]) or den (float64 [KP])) or from mat (float64 (V, ld), reference
    topic order); wdiv float64 [V] or None; top_idx (K, n) int32, top_score (K, n) float64, n_nan (K,) int32 the outputs, each may be
    None; scratch = a uint8 tensor of scored_words_scratch_bytes(V, K, n) bytes."""
    args = LldaScoredArgs(ctypes.sizeof(LldaScoredArgs), int(K), int(n), int(a), _ptr(n_kw), _ptr(n_k), _ptr(den), _ptr(mat), _ptr(wdiv),
                          int(V), int((0 if mat is None else mat.stride(0)) if ld is None else ld), float(beta), _ptr(top_idx),
                          _ptr(top_score), _ptr(n_nan), _ptr(scratch), int(scratch.numel() * scratch.element_size()))
    _launch(scratch, lib().llda_scored_words, "llda_scored_words", ctypes.byref(args))


ECDF_MAX_V = 1 << 30          # LLDA_ECDF_MAX_V
FREX_MAX_N = 16               # LLDA_FREX_MAX_N
FREX_MAX_T = 64               # LLDA_FREX_MAX_T: the largest denominator of the weight
FREX_CHUNK = 16384            # LLDA_FREX_CHUNK: words of a partial list of llda_frex_select


def ecdf_scratch_bytes(V, n_labels, chunk=0):
    """llda_ecdf_scratch_bytes: bytes of work space llda_ecdf_ranks needs (host only)."""
    r = int(lib().llda_ecdf_scratch_bytes(int(V), int(n_labels), int(chunk)))
    if r < 0:
        check(r, "llda_ecdf_scratch_bytes(V=%d, n_labels=%d, chunk=%d)" % (V, n_labels, chunk))
    return r


def ecdf_ranks(mat, V, K, mode, first, n_labels, rank, scratch, *, ld=None, chunk=0, cand=None, value=None, n_cand=None):
    """llda_ecdf_ranks on the current torch stream: mat (V, ld) float64 in reference topic order, cand (V,) uint8 or None; rank
    (n_labels, V) int32, value (n_labels, V) float64 or None, n_cand (1,) int64 or None the outputs; scratch = a uint8 tensor of
    ecdf_scratch_bytes(V, n_labels, chunk) bytes."""
    a = LldaEcdfArgs(ctypes.sizeof(LldaEcdfArgs), int(K), int(first), int(n_labels), int(chunk), int(mode), _ptr(mat), _ptr(cand), int(V),
                     int(mat.stride(0) if ld is None else ld), _ptr(rank), _ptr(value), _ptr(n_cand), _ptr(scratch),
                     int(scratch.numel() * scratch.element_size()))
    _launch(mat, lib().llda_ecdf_ranks, "llda_ecdf_ranks", ctypes.byref(a))


def frex_scratch_bytes(V, n_labels, n):
    """llda_frex_scratch_bytes: bytes of work space llda_frex_select needs (host only)."""
    r = int(lib().llda_frex_scratch_bytes(int(V), int(n_labels), int(n)))
    if r < 0:
        check(r, "llda_frex_scratch_bytes(V=%d, n_labels=%d, n=%d)" % (V, n_labels, n))
    return r


def frex_select(rank_f, rank_e, V, Vc, n_labels, s, t, n, scratch, *, probe=None, m=0, top_idx=None, top_rank_f=None, top_rank_e=None,
                probe_rank_f=None, probe_rank_e=None):
    """llda_frex_select on the current torch stream: rank_f, rank_e (n_labels, V) int32; the weight s / t; top_idx, top_rank_f,
    top_rank_e (n_labels, n) int32 and, with probe (n_labels, m) int32, probe_rank_f, probe_rank_e (n_labels, m) int32 the outputs,
    each may be None; scratch = a uint8 tensor of frex_scratch_bytes(V, n_labels, n) bytes."""
    a = LldaFrexArgs(ctypes.sizeof(LldaFrexArgs), int(n_labels), int(n), int(m), int(s), int(t), _ptr(rank_f), _ptr(rank_e), _ptr(probe),
                     int(V), int(Vc), _ptr(top_idx), _ptr(top_rank_f), _ptr(top_rank_e), _ptr(probe_rank_f), _ptr(probe_rank_e),
                     _ptr(scratch), int(scratch.numel() * scratch.element_size()))
    _launch(scratch, lib().llda_frex_select, "llda_frex_select", ctypes.byref(a))


def word_cooc(doc_off, word, D, V, K, n, memb_off, memb, co):
    """llda_word_cooc on the current torch stream: co (int64 (K, n, n), accumulates) += the document and co-document frequencies
    of the words the membership table (memb_off int32 [V+1], memb int32 [M] of topic*16 + rank) lists, over the D documents of
    the CSR doc_off (int64, at least D+1 entries) / word (int32)."""
    _launch(co, lib().llda_word_cooc, "llda_word_cooc", _ptr(doc_off), _ptr(word), int(D), int(V), int(K), int(n), _ptr(memb_off),
            _ptr(memb), _ptr(co))


WINDOW_MAX = 65535   # LLDA_WINDOW_MAX: the widest sliding window of llda_window_cooc
WINDOW_MAX_WAVES = 8192   # LLDA_WINDOW_MAX_WAVES: wavefront i of llda_window_cooc takes the documents i, i + 8192, ... in turn ...
WINDOW_AGG_MIN_DOCS = 32768   # ... LLDA_WINDOW_AGG_MIN_DOCS: in calls of fewer documents; larger calls add to LDS counters first


def window_cooc(tok_off, tok, D, V, K, n, window, memb_off, memb, co):
    """llda_window_cooc on the current torch stream: co (int64 (K, n, n), accumulates) += in how many sliding windows of ``window``
    tokens (0 = the whole document) the words of the membership table meet, over the D documents tok_off (int64, at least D+1
    entries) / tok (int32 token ids in reading order; an id outside 0 .. V-1 holds its place and matches nothing)."""
    _launch(co, lib().llda_window_cooc, "llda_window_cooc", _ptr(tok_off), _ptr(tok), int(D), int(V), int(K), int(n), int(window),
            _ptr(memb_off), _ptr(memb), _ptr(co))


HELDOUT_MAX_FREQ = 2 ** 23 - 1   # LLDA_HELDOUT_MAX_FREQ


def heldout_loglik(doc_off, word, freq, theta, phi_t, D, V, K, *, ld_theta=None, ld_phi=None, mant=None, expo=None, tok=None, bad=None):
    """llda_heldout_loglik on the current torch stream: doc_off (int64 [D+1]), word (int32 [S]), freq (int32 [S] or None = all 1)
    the sites to score; theta (D, ld_theta) and phi_t (V, ld_phi) float64 in reference topic order; mant (float64 [D]), expo, tok, bad
    (int64 [D]) the outputs, each may be None."""
    a = LldaHeldoutArgs(_ptr(doc_off), _ptr(word), _ptr(freq), _ptr(theta), _ptr(phi_t), int(D), int(V),
                        int(theta.stride(0) if ld_theta is None else ld_theta), int(phi_t.stride(0) if ld_phi is None else ld_phi),
                        int(K), 0, _ptr(mant), _ptr(expo), _ptr(tok), _ptr(bad))
    _launch(theta, lib().llda_heldout_loglik, "llda_heldout_loglik", ctypes.byref(a))


ATTR_MIN_P = 2.0 ** -960       # LLDA_ATTR_MIN_P: a site whose p is below it (or not finite) is not attributed
ATTR_MAX_TOP = 4               # LLDA_ATTR_MAX_TOP


def attribute(doc_off, word, freq, theta, phi_t, D, V, K, *, iters=0, alpha=0.0, top_m=0, ld_theta=None, ld_phi=None, ld_out=None,
              ld_credit=None, theta_out=None, credit=None, site_idx=None, site_val=None, tok=None, bad=None):
    """llda_attribute on the current torch stream: the CSR and the two matrices as heldout_loglik takes them; iters EM steps with
    alpha; theta_out (D, ld_out) and credit (D, ld_credit) float64, site_idx (S, top_m) int32, site_val (S, top_m) float64, tok, bad
    (int64 [D]) the outputs, each may be None."""
    a = LldaAttrArgs(_ptr(doc_off), _ptr(word), _ptr(freq), _ptr(theta), _ptr(phi_t), int(D), int(V),
                     int(theta.stride(0) if ld_theta is None else ld_theta), int(phi_t.stride(0) if ld_phi is None else ld_phi),
                     int(K if theta_out is None else theta_out.stride(0)) if ld_out is None else int(ld_out),
                     int(K if credit is None else credit.stride(0)) if ld_credit is None else int(ld_credit),
                     int(K), int(iters), int(top_m), 0, float(alpha), _ptr(theta_out), _ptr(credit), _ptr(site_idx), _ptr(site_val),
                     _ptr(tok), _ptr(bad))
    _launch(theta, lib().llda_attribute, "llda_attribute", ctypes.byref(a))


COLSUM_ROWS = 256              # LLDA_COLSUM_ROWS: words of a block of llda_phi_step's column sums


def credit_words_scratch_bytes(V, S, K, chunk):
    """llda_credit_words_scratch_bytes: bytes of work space llda_credit_words needs (host only)."""
    r = int(lib().llda_credit_words_scratch_bytes(int(V), int(S), int(K), int(chunk)))
    if r < 0:
        check(r, "llda_credit_words_scratch_bytes(V=%d, S=%d, K=%d, chunk=%d)" % (V, S, K, chunk))
    return r


def credit_words(word_off, site_doc, freq, theta, phi_t, D, V, S, K, chunk, scratch, *, ld_theta=None, ld_phi=None, ld_credit=None,
                 credit_w=None, tok=None, bad=None):
    """llda_credit_words on the current torch stream: word_off (int64 [V+1]) / site_doc (int32 [S]) / freq (int32 [S] or None) the
    sites in word-major order; theta (D, ld_theta) and phi_t (V, ld_phi) float64; credit_w (V, ld_credit) float64, tok, bad (int64
    [V]) the outputs, each may be None; scratch = a uint8 tensor of credit_words_scratch_bytes(V, S, K, chunk) bytes (None: S = 0)."""
    a = LldaWcreditArgs(ctypes.sizeof(LldaWcreditArgs), int(K), int(chunk), 0, _ptr(word_off), _ptr(site_doc), _ptr(freq), _ptr(theta),
                        _ptr(phi_t), int(D), int(V), int(S), int(theta.stride(0) if ld_theta is None else ld_theta),
                        int(phi_t.stride(0) if ld_phi is None else ld_phi),
                        int(K if credit_w is None else credit_w.stride(0)) if ld_credit is None else int(ld_credit),
                        _ptr(credit_w), _ptr(tok), _ptr(bad), _ptr(scratch), 0 if scratch is None else int(scratch.numel()))
    _launch(phi_t, lib().llda_credit_words, "llda_credit_words", ctypes.byref(a))


def phi_step_scratch_bytes(V, K):
    """llda_phi_step_scratch_bytes: bytes of work space llda_phi_step needs (host only)."""
    r = int(lib().llda_phi_step_scratch_bytes(int(V), int(K)))
    if r < 0:
        check(r, "llda_phi_step_scratch_bytes(V=%d, K=%d)" % (V, K))
    return r


def phi_step(cw, V, K, beta, out, scratch, *, ld=None, ld_out=None, den=None):
    """llda_phi_step on the current torch stream: cw (V, ld) float64 the word credit, out (V, ld_out) float64 the new phi_t (may be
    cw), den (float64 [K]) or None; scratch = a uint8 tensor of phi_step_scratch_bytes(V, K) bytes."""
    a = LldaPhistepArgs(ctypes.sizeof(LldaPhistepArgs), int(K), _ptr(cw), _ptr(out), _ptr(den), int(V),
                        int(cw.stride(0) if ld is None else ld), int(out.stride(0) if ld_out is None else ld_out), float(beta),
                        _ptr(scratch), int(scratch.numel()))
    _launch(cw, lib().llda_phi_step, "llda_phi_step", ctypes.byref(a))


SPARSE_MAX_LABELS = 32         # LLDA_SPARSE_MAX_LABELS: labels of a document in the sparse-label entry points at most


def attribute_sparse(doc_off, word, freq, lab_off, lab, theta_s, phi_t, D, V, K, NL, max_labels, *, iters=0, alpha=0.0, top_m=0,
                     ld_phi=None, theta_out=None, credit=None, site_idx=None, site_val=None, tok=None, bad=None):
    """llda_attribute_sparse on the current torch stream: the CSR of the sites as ``attribute`` takes it; lab_off (int64 [D+1]) / lab
    (int32 [NL]) the label sets, theta_s (float64 [NL]) the loads per slot; phi_t (V, ld_phi) float64; theta_out, credit (float64
    [NL]), site_idx (S, top_m) int32, site_val (S, top_m) float64, tok, bad (int64 [D]) the outputs, each may be None."""
    a = LldaAttrSparseArgs(ctypes.sizeof(LldaAttrSparseArgs), int(K), int(max_labels), int(iters), int(top_m), 0, _ptr(doc_off), _ptr(word),
                           _ptr(freq), _ptr(lab_off), _ptr(lab), _ptr(theta_s), _ptr(phi_t), int(D), int(V), int(NL),
                           int(phi_t.stride(0) if ld_phi is None else ld_phi), float(alpha), _ptr(theta_out), _ptr(credit), _ptr(site_idx),
                           _ptr(site_val), _ptr(tok), _ptr(bad))
    _launch(phi_t, lib().llda_attribute_sparse, "llda_attribute_sparse", ctypes.byref(a))


def credit_words_sparse_scratch_bytes(V, S, K, chunk):
    """llda_credit_words_sparse_scratch_bytes: bytes of work space llda_credit_words_sparse needs (host only)."""
    r = int(lib().llda_credit_words_sparse_scratch_bytes(int(V), int(S), int(K), int(chunk)))
    if r < 0:
        check(r, "llda_credit_words_sparse_scratch_bytes(V=%d, S=%d, K=%d, chunk=%d)" % (V, S, K, chunk))
    return r


def credit_words_sparse(word_off, site_doc, freq, lab_off, lab, theta_s, phi_t, D, V, S, K, NL, max_labels, chunk, scratch, *, ld_phi=None,
                        ld_credit=None, credit_w=None, tok=None, bad=None):
    """llda_credit_words_sparse on the current torch stream: the word-major sites as ``credit_words`` takes them, the label sets and
    the loads per slot as ``attribute_sparse`` does; credit_w (V, ld_credit) float64, tok, bad (int64 [V]) the outputs, each may be
    None; scratch = a uint8 tensor of credit_words_sparse_scratch_bytes(V, S, K, chunk) bytes (None: S = 0)."""
    a = LldaWcreditSparseArgs(ctypes.sizeof(LldaWcreditSparseArgs), int(K), int(chunk), int(max_labels), _ptr(word_off), _ptr(site_doc),
                              _ptr(freq), _ptr(lab_off), _ptr(lab), _ptr(theta_s), _ptr(phi_t), int(D), int(V), int(S), int(NL),
                              int(phi_t.stride(0) if ld_phi is None else ld_phi),
                              int(K if credit_w is None else credit_w.stride(0)) if ld_credit is None else int(ld_credit),
                              _ptr(credit_w), _ptr(tok), _ptr(bad), _ptr(scratch), 0 if scratch is None else int(scratch.numel()))
    _launch(phi_t, lib().llda_credit_words_sparse, "llda_credit_words_sparse", ctypes.byref(a))


LR_MAX_PARTICLES = 16          # LLDA_LR_MAX_PARTICLES
LR_MAX_TOKENS = 4096           # LLDA_LR_MAX_TOKENS
LR_MAX_K = 1024                # llda_left_to_right keeps a particle's counts in registers


def left_to_right(doc_off, word, phi_t, D, V, K, *, particles, alpha, seed, stream_id, max_doc_tokens, mant, expo, tok, bad,
                  ld_phi=None, allowed=None, ld_allowed=None, doc_ids=None, doc_base=0, status=None):
    """llda_left_to_right on the current torch stream: doc_off (int64 [D+1]) / word (int32 [S]) the TOKENS in the text's order; phi_t
    (V, ld_phi) float64 in reference topic order; allowed (D, ld_allowed) uint8 or None; doc_ids int64 [D] or None; mant (float64
    [D]), expo, tok, bad (int64 [D]) the outputs; status int32 [1] or None."""
    a = LldaLeftrightArgs(ctypes.sizeof(LldaLeftrightArgs), int(K), int(particles), int(max_doc_tokens), _ptr(doc_off), _ptr(word),
                          _ptr(phi_t), _ptr(allowed), _ptr(doc_ids), int(D), int(V), int(phi_t.stride(0) if ld_phi is None else ld_phi),
                          int((K if allowed is None else allowed.stride(0)) if ld_allowed is None else ld_allowed), int(doc_base),
                          float(alpha), int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, 0, _ptr(mant), _ptr(expo),
                          _ptr(tok), _ptr(bad), _ptr(status))
    _launch(phi_t, lib().llda_left_to_right, "llda_left_to_right", ctypes.byref(a))


def heldout_loglik_sparse(doc_off, word, freq, lab_off, lab, theta_s, phi_t, D, V, K, NL, max_labels, *, ld_phi=None, mant=None,
                          expo=None, tok=None, bad=None):
    """llda_heldout_loglik_sparse on the current torch stream: the sites as ``heldout_loglik`` takes them, the label sets and the loads
    per slot as ``attribute_sparse`` does; mant (float64 [D]), expo, tok, bad (int64 [D]) the outputs, each may be None."""
    a = LldaHeldoutSparseArgs(ctypes.sizeof(LldaHeldoutSparseArgs), int(K), int(max_labels), 0, _ptr(doc_off), _ptr(word), _ptr(freq),
                              _ptr(lab_off), _ptr(lab), _ptr(theta_s), _ptr(phi_t), int(D), int(V), int(NL),
                              int(phi_t.stride(0) if ld_phi is None else ld_phi), _ptr(mant), _ptr(expo), _ptr(tok), _ptr(bad))
    _launch(phi_t, lib().llda_heldout_loglik_sparse, "llda_heldout_loglik_sparse", ctypes.byref(a))


def left_to_right_sparse(doc_off, word, phi_t, lab_off, lab, D, V, K, NL, max_labels, *, particles, alpha, seed, stream_id, max_doc_tokens,
                         mant, expo, tok, bad, ld_phi=None, doc_ids=None, doc_base=0, status=None):
    """llda_left_to_right_sparse on the current torch stream: the tokens and the outputs as ``left_to_right`` takes them, the label
    sets lab_off (int64 [D+1]) / lab (int32 [NL]) in place of the allowed rows; K up to LLDA_MAX_K."""
    a = LldaLeftrightSparseArgs(ctypes.sizeof(LldaLeftrightSparseArgs), int(K), int(particles), int(max_doc_tokens), _ptr(doc_off),
                                _ptr(word), _ptr(phi_t), _ptr(lab_off), _ptr(lab), _ptr(doc_ids), int(D), int(V),
                                int(phi_t.stride(0) if ld_phi is None else ld_phi), int(NL), int(doc_base), float(alpha),
                                int(seed) & 0xFFFFFFFFFFFFFFFF, int(stream_id) & 0xFFFFFFFF, int(max_labels), _ptr(mant), _ptr(expo),
                                _ptr(tok), _ptr(bad), _ptr(status))
    _launch(phi_t, lib().llda_left_to_right_sparse, "llda_left_to_right_sparse", ctypes.byref(a))


def foldin_sparse(doc_off, word, freq, phi_t, lab_off, lab, D, V, K, NL, max_labels, *, iters, thinning, alpha, c_init, c_loop, seed,
                  stream_id, z, n_dk_s, th_s, ld_phi=None, doc_ids=None, doc_base=0, status=None):
    """llda_foldin_sparse on the current torch stream: doc_off (int64 [D+1]) / word / freq (int32 [S]) the sites; phi_t (V, ld_phi)
    float64 in reference topic order; the label sets lab_off (int64 [D+1]) / lab (int32 [NL]); doc_ids int64 [D] or None; z (int32
    [S], the slot of every site), n_dk_s (int32 [NL]), th_s (float64 [NL]) the outputs; status int32 [1] or None."""
    a = LldaFoldinSparseArgs(ctypes.sizeof(LldaFoldinSparseArgs), int(K), int(max_labels), int(iters), int(thinning),
                             int(stream_id) & 0xFFFFFFFF, _ptr(doc_off), _ptr(word), _ptr(freq), _ptr(phi_t), _ptr(lab_off), _ptr(lab),
                             _ptr(doc_ids), int(D), int(V), int(NL), int(phi_t.stride(0) if ld_phi is None else ld_phi), int(doc_base),
                             float(alpha), float(c_init), float(c_loop), int(seed) & 0xFFFFFFFFFFFFFFFF, _ptr(z), _ptr(n_dk_s),
                             _ptr(th_s), _ptr(status))
    _launch(phi_t, lib().llda_foldin_sparse, "llda_foldin_sparse", ctypes.byref(a))


NEAREST_MAX_N = 16            # LLDA_NEAREST_MAX_N
NEAREST_TILE = 128            # LLDA_NEAREST_TILE: queries and rows of a tile of llda_nearest_rows
NEAREST_KSTEP = 16            # LLDA_NEAREST_KSTEP: columns per step of its k-loop


def nearest_scratch_bytes(Q, D, n, chunks=0):
    """llda_nearest_scratch_bytes: bytes of work space llda_nearest_rows needs (host only)."""
    r = int(lib().llda_nearest_scratch_bytes(int(Q), int(D), int(n), int(chunks)))
    if r < 0:
        check(r, "llda_nearest_scratch_bytes(Q=%d, D=%d, n=%d, chunks=%d)" % (Q, D, n, chunks))
    return r


def nearest_rows(a, b, Q, D, L, n, scratch, *, lda=None, ldb=None, row_base=0, exclude=None, chunks=0, top_idx=None, top_val=None,
                 n_nan=None):
    """llda_nearest_rows on the current torch stream: a (Q, lda) and b (D, ldb) float64 on the device, exclude int64 [Q] or None;
    top_idx (Q, n) int64, top_val (Q, n) float64, n_nan (Q,) int64 the outputs, each may be None; scratch = a uint8 tensor of
    nearest_scratch_bytes(Q, D, n, chunks) bytes."""
    args = LldaNearestArgs(ctypes.sizeof(LldaNearestArgs), int(L), int(n), int(chunks), _ptr(a), _ptr(b), _ptr(exclude), int(Q), int(D),
                           int(a.stride(0) if lda is None else lda), int(b.stride(0) if ldb is None else ldb), int(row_base),
                           _ptr(top_idx), _ptr(top_val), _ptr(n_nan), _ptr(scratch), int(scratch.numel() * scratch.element_size()))
    _launch(scratch, lib().llda_nearest_rows, "llda_nearest_rows", ctypes.byref(args))


LABEL_CHUNK = 4096            # LLDA_LABEL_CHUNK: pairs one workgroup of llda_label_metrics sorts in LDS
LABEL_TEST_CHUNK = 256        # LLDA_LABEL_TEST_CHUNK: the one other value of llda_label_args.chunk
LABEL_MAX_D = 1 << 30         # LLDA_LABEL_MAX_D


def label_scratch_bytes(D, n_labels, chunk=0):
    """llda_label_scratch_bytes: bytes of work space llda_label_metrics needs (host only)."""
    r = int(lib().llda_label_scratch_bytes(int(D), int(n_labels), int(chunk)))
    if r < 0:
        check(r, "llda_label_scratch_bytes(D=%d, n_labels=%d, chunk=%d)" % (D, n_labels, chunk))
    return r


def label_metrics(score, truth, D, K, first, n_labels, scratch, *, ld=None, chunk=0, n_pos=None, n_thr=None, auc_num=None, auc=None,
                  thr_tp=None, thr_fp=None, f1=None, thr=None, flags=None, order=None):
    """llda_label_metrics on the current torch stream: score (D, ld) float64 in reference topic order, truth (D, K) uint8; the
    outputs (n_labels,) int64 / float64 / int32 and order (n_labels, D) int32, each may be None; scratch = a uint8 tensor of
    label_scratch_bytes(D, n_labels, chunk) bytes."""
    a = LldaLabelArgs(ctypes.sizeof(LldaLabelArgs), int(K), int(first), int(n_labels), int(chunk), 0, _ptr(score), _ptr(truth), int(D),
                      int(score.stride(0) if ld is None else ld), _ptr(n_pos), _ptr(n_thr), _ptr(auc_num), _ptr(auc), _ptr(thr_tp),
                      _ptr(thr_fp), _ptr(f1), _ptr(thr), _ptr(flags), _ptr(order), _ptr(scratch),
                      int(scratch.numel() * scratch.element_size()))
    _launch(score, lib().llda_label_metrics, "llda_label_metrics", ctypes.byref(a))


def label_sets(score, thr, truth, D, K, first, at_least_one, *, ld=None, mask=None, n_pred=None, n_hit=None, n_true=None, tp=None,
               fp=None, fn=None):
    """llda_label_sets on the current torch stream: score (D, ld) float64, thr (K,) float64, truth (D, K) uint8 or None; mask
    (D, (K + 31) // 32) int32 bit words, n_pred, n_hit, n_true (D,) int32, tp, fp, fn (K,) int64 ADDED to (zero them); each may be
    None."""
    a = LldaSetsArgs(ctypes.sizeof(LldaSetsArgs), int(K), int(first), 1 if at_least_one else 0, _ptr(score), _ptr(thr), _ptr(truth),
                     int(D), int(score.stride(0) if ld is None else ld), _ptr(mask), _ptr(n_pred), _ptr(n_hit), _ptr(n_true), _ptr(tp),
                     _ptr(fp), _ptr(fn))
    _launch(score, lib().llda_label_sets, "llda_label_sets", ctypes.byref(a))


def loglik(doc_off, word, lab_mask, n_dk, n_kw, n_k, D, V, K, alpha, beta, out_doc):
    _launch(out_doc, lib().llda_loglik, "llda_loglik", _ptr(doc_off), _ptr(word), _ptr(lab_mask), _ptr(n_dk), _ptr(n_kw),
            _ptr(n_k), int(D), int(V), int(K), float(alpha), float(beta), _ptr(out_doc))


READOUT_NEGATIVE, READOUT_NAN, READOUT_NO_LOAD = 1, 2, 4


def readout_phi(n_kw, n_k, den, V, K, beta, out, flags=None, keep=None, share=None):
    """llda_readout_phi: out (K, V) float64 = phi of the counts, or keep*out + share*phi when the two
    coefficients are given."""
    mode = 0 if keep is None else 1
    _launch(out, lib().llda_readout_phi, "llda_readout_phi", _ptr(n_kw), _ptr(n_k), _ptr(den), int(V), int(K), float(beta),
            mode, float(keep or 0.0), float(share or 0.0), _ptr(out), _ptr(flags))


def readout_theta(n_dk, lab_mask, D, K, alpha, out, keep=None, share=None):
    """llda_readout_theta: out (D, K) float64 = theta of the counts, or its running mean (as readout_phi)."""
    mode = 0 if keep is None else 1
    _launch(out, lib().llda_readout_theta, "llda_readout_theta", _ptr(n_dk), _ptr(lab_mask), int(D), int(K), float(alpha),
            mode, float(keep or 0.0), float(share or 0.0), _ptr(out))


def selftest_div(n, seed=1):
    """llda_selftest_div: number of (a, b) pairs (out of >= n) where the kernel's reciprocal-based
    division differs from the hardware IEEE division.  Must be 0."""
    import torch
    bad = torch.zeros((1,), dtype=torch.int64, device="cuda")
    _launch(bad, lib().llda_selftest_div, "llda_selftest_div", int(seed), int(n), _ptr(bad))
    return int(bad.item())


def foldin(*, doc_off, word, init_idx, freq, ph, init_rows, slot_valid, z, n_dk, th, status, D, K, iters, thinning,
           alpha, beta, c_init, c_loop, seed, stream_id, doc_base=0, beta_fallback=False, avg_mode=0, doc_ids=None,
           ph_base=None, doc_stream=None, exact_only=False, n_sites=None):
    """llda_foldin on the current torch stream.  ph, init_rows, slot_valid, n_dk and th are lane-major (layout.lm_topic_pos), z holds
    group-layout positions.  n_sites = None: ``word.numel()`` (the initial assignments by a launch of their own, n_dk zeroed by the
    caller); 0: drawn inside the per-document launch, z and n_dk pure outputs.  status, doc_ids, ph_base, doc_stream may be None."""
    a = LldaFoldinArgs(_ptr(doc_off), _ptr(word), _ptr(init_idx), _ptr(freq), _ptr(ph), _ptr(init_rows),
                       _ptr(slot_valid), _ptr(z), _ptr(n_dk), _ptr(th), _ptr(status), int(D), int(doc_base), int(K),
                       int(iters), int(thinning), 1 if beta_fallback else 0, int(avg_mode), 1 if exact_only else 0, float(alpha),
                       float(beta), float(c_init), float(c_loop), int(seed) & 0xFFFFFFFFFFFFFFFF,
                       int(stream_id) & 0xFFFFFFFF, 0, _ptr(doc_ids), int(word.numel() if n_sites is None else n_sites), _ptr(ph_base), _ptr(doc_stream))
    _launch(z, lib().llda_foldin, "llda_foldin", ctypes.byref(a))
