"""ctypes binding of libpca_hip.so (C ABI declared in include/pca_hip.h).

The shared object is the product: if it is missing or fails to load, everything that
needs it raises -- there is no CPU or PyTorch fallback behind this module.
"""
from __future__ import annotations

import ctypes as C
import os
import threading

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libpca_hip.so")

PCA_F32, PCA_BF16 = 0, 1
K_GEMM_F32, K_MAB1_FWD, K_MAB1_BWD, K_MAB0_FWD, K_MAB0_BWD, K_WGRAD = 1, 2, 3, 4, 5, 6
K_SET_FWD, K_SET_BWD = 7, 8
MODE_F32, MODE_BF16, MODE_FP8 = 0, 1, 2

c_fp = C.c_void_p       # float* (device)
c_vp = C.c_void_p
c_i64p = C.c_void_p


class MabShape(C.Structure):
    _fields_ = [(n, C.c_int32) for n in
                ("B", "nq", "nk", "dq", "dk", "d", "h", "q_shared", "mode",
                 "q_dtype", "k_dtype", "y_dtype")] + [("k_lengths", C.c_void_p), ("ln", C.c_int32)]


class MabParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo",
                                          "ln0_w", "ln0_b", "ln1_w", "ln1_b")]


class MabGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wq", "bq", "wk", "bk", "wv", "bv", "wo", "bo",
                                          "ln0_w", "ln0_b", "ln1_w", "ln1_b")]


class StConfig(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "N", "din", "d", "h", "m", "k", "C", "mode")]


class OptimCfg(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("lr", "beta1", "beta2", "eps", "weight_decay",
                                         "grad_scale", "max_norm")] + [("skip_nonfinite", C.c_int32)]


class OptimState(C.Structure):
    _fields_ = [("skipped", C.c_int32), ("clipped", C.c_int32), ("last_norm", C.c_float),
                ("last_lr", C.c_float), ("norm_sum", C.c_double), ("norm_count", C.c_int32),
                ("reserved", C.c_int32)]


class OptimGroups(C.Structure):
    _fields_ = [("decoupled", C.c_int32), ("n_seg", C.c_int32), ("seg_end", C.c_void_p),
                ("seg_lr_scale", C.c_void_p), ("seg_wd_scale", C.c_void_p), ("avg", C.c_void_p),
                ("avg_weight", C.c_float), ("avg_start", C.c_int32)]


class PcaFrameAug(C.Structure):
    _fields_ = [("jitter", C.c_int32), ("gain_db", C.c_float), ("win_lengths", C.c_void_p),
                ("n_win", C.c_int32), ("norm_mode", C.c_int32), ("seed", C.c_uint64),
                ("draw", C.c_uint64), ("draw_dev", C.c_void_p)]


FRAME_MAX_LEVELS = 4


class PcaFrameLevel(C.Structure):
    _fields_ = [("n_fft", C.c_int32), ("hop", C.c_int32), ("n_bins", C.c_int32), ("Nt", C.c_int32),
                ("offset", C.c_int32), ("farr", C.c_void_p), ("tarr", C.c_void_p),
                ("win_lengths", C.c_void_p)]


class PcaFrameBands(C.Structure):
    _fields_ = [("n_bands", C.c_int32), ("nnz", C.c_int32), ("band_lo", C.c_void_p),
                ("band_off", C.c_void_p), ("weights", C.c_void_p), ("power", C.c_int32),
                ("amin", C.c_float)]


class PcaPcen(C.Structure):
    _fields_ = [("context", C.c_int32), ("s", C.c_float), ("gain", C.c_float), ("bias", C.c_float),
                ("r", C.c_float), ("eps", C.c_float), ("scale", C.c_float)]


class PcaDelta(C.Structure):
    _fields_ = [("axes", C.c_int32), ("width", C.c_int32)]


FRAME_MAX_SPEEDS = 8


class PcaFrameAugEx(C.Structure):
    _fields_ = PcaFrameAug._fields_ + [
        ("n_speed", C.c_int32), ("nwin", C.c_int32), ("num_table", C.c_int32), ("n_bg", C.c_int32),
        ("ratios", C.c_double * FRAME_MAX_SPEEDS), ("tables", C.c_void_p),
        ("bg_waves", C.c_void_p), ("bg_off", C.c_void_p), ("bg_rms", C.c_void_p),
        ("clip_rms", C.c_void_p), ("bg_max_len", C.c_int64), ("mix_prob", C.c_double),
        ("snr_lo_db", C.c_double), ("snr_hi_db", C.c_double)]


POINT_MASK_MAX = 4
MASK_DROP, MASK_FLOOR = 0, 1


class PcaPointMask(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("n_freq", "freq_width", "n_time", "time_width", "mode")]


class PcaPeakSpec(C.Structure):
    _fields_ = [("radius_f", C.c_int32), ("radius_t", C.c_int32), ("rel_floor", C.c_float),
                ("abs_floor", C.c_float), ("refine", C.c_int32)]


class PcaReassignSpec(C.Structure):
    _fields_ = [("axes", C.c_int32), ("rel_floor", C.c_float), ("abs_floor", C.c_float),
                ("max_df", C.c_float), ("max_dt", C.c_float), ("strength", C.c_float)]


class PcaSoftTargets(C.Structure):
    _fields_ = [("labels2", C.c_void_p), ("weight", C.c_void_p), ("smoothing", C.c_float)]


class GemmDesc(C.Structure):
    _fields_ = [("M", C.c_int64), ("N", C.c_int64), ("K", C.c_int64),
                ("sa_m", C.c_int64), ("sa_k", C.c_int64), ("sb_k", C.c_int64),
                ("sb_n", C.c_int64), ("sc_m", C.c_int64),
                ("nb1", C.c_int32), ("nb2", C.c_int32),
                ("sa_b1", C.c_int64), ("sa_b2", C.c_int64), ("sb_b1", C.c_int64),
                ("sb_b2", C.c_int64), ("sc_b1", C.c_int64), ("sc_b2", C.c_int64),
                ("accumulate", C.c_int32), ("split_k", C.c_int32), ("alpha", C.c_float)]


# name -> (restype, argtypes); every symbol include/pca_hip.h declares
SIGNATURES = {
    "pca_abi_version": (C.c_int, []),
    "pca_last_error": (C.c_char_p, []),
    "pca_stft_num_frames": (C.c_int64, [C.c_int64, C.c_int]),
    "pca_stft_logmag": (C.c_int, [c_fp, C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                  C.c_int64, C.c_int64, c_vp]),
    "pca_stft_logmag_batch": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64,
                                        C.c_int, C.c_int, C.c_int, C.c_int, c_fp, C.c_int64,
                                        C.c_int64, c_vp]),
    "pca_stft_logmag_batch_norm": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64,
                                             C.c_int64, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                             C.c_int64, C.c_int64, C.c_double, c_vp]),
    "pca_trim_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int, C.c_int]),
    "pca_trim_bounds": (C.c_int, [c_fp, c_i64p, C.c_int, C.c_int64, C.c_int64, C.c_int, C.c_int,
                                  C.c_double, c_i64p, c_vp, c_vp]),
    "pca_resample": (C.c_int, [c_fp, C.c_int64, C.c_double, c_vp, c_vp, C.c_int, C.c_int, C.c_float, c_fp,
                               C.c_int64, c_vp]),
    "pca_pack_points_2d": (C.c_int, [c_fp, C.c_int64, C.c_int64, c_fp, c_i64p, C.c_int,
                                     C.c_int, c_fp, c_i64p, c_i64p, c_vp]),
    "pca_pack_points_3d": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_fp, c_fp,
                                     c_i64p, C.c_int, C.c_int, C.c_int, c_fp, c_i64p, c_i64p,
                                     c_vp]),
    "pca_pack_points_2d_seq": (C.c_int, [c_fp, C.c_int64, C.c_int64, c_fp, c_i64p, c_vp, c_vp,
                                         C.c_int, C.c_int, c_fp, c_i64p, c_i64p, c_vp]),
    "pca_pack_defer": (C.c_int, [C.c_int]),
    "pca_pack_points_3d_seq": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_fp, c_fp,
                                         c_vp, c_i64p, c_vp, c_vp, C.c_int, C.c_int, C.c_int,
                                         c_fp, c_vp, c_i64p, c_i64p, c_vp]),
    "pca_pack_points_3d_var": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_fp, c_fp,
                                         c_vp, c_i64p, C.c_int, C.c_int, C.c_int, c_fp, c_vp,
                                         c_i64p, c_i64p, c_vp]),
    "pca_mab_saved_bytes": (C.c_size_t, [C.POINTER(MabShape)]),
    "pca_mab_fwd_ws_bytes": (C.c_size_t, [C.POINTER(MabShape)]),
    "pca_mab_bwd_ws_bytes": (C.c_size_t, [C.POINTER(MabShape)]),
    "pca_mab_fwd": (C.c_int, [C.POINTER(MabShape), c_vp, c_vp, C.POINTER(MabParams), c_vp,
                              c_vp, c_vp, c_vp]),
    "pca_mab_bwd": (C.c_int, [C.POINTER(MabShape), c_vp, c_vp, C.POINTER(MabParams), c_vp,
                              c_vp, c_vp, c_vp, C.c_int, C.POINTER(MabGrads), c_vp, c_vp]),
    "pca_pma_attention_ws_bytes": (C.c_size_t, [C.POINTER(MabShape)]),
    "pca_pma_attention": (C.c_int, [C.POINTER(MabShape), c_fp, c_fp, C.POINTER(MabParams), c_fp, c_fp,
                                    c_vp, c_vp]),
    "pca_select_points": (C.c_int, [c_fp, c_fp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_vp,
                                    c_vp]),
    "pca_peak_points": (C.c_int, [c_fp, c_vp, C.c_int, C.c_int, C.c_int, C.c_int, C.POINTER(PcaPeakSpec),
                                  C.c_int, c_fp, c_vp, c_vp, c_vp, c_vp]),
    "pca_linear_fwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int64, C.c_int, C.c_int, c_vp]),
    "pca_linear_bwd": (C.c_int, [c_fp, c_fp, c_fp, c_fp, c_fp, c_fp, C.c_int64, C.c_int,
                                 C.c_int, c_vp, c_vp]),
    "pca_linear_bwd_ws_bytes": (C.c_size_t, [C.c_int64, C.c_int, C.c_int]),
    "pca_cross_entropy": (C.c_int, [c_fp, c_i64p, C.c_int, C.c_int, C.c_float, c_fp, c_fp,
                                    c_fp, c_vp]),
    "pca_cross_entropy_soft": (C.c_int, [c_fp, c_i64p, C.POINTER(PcaSoftTargets), C.c_int, C.c_int,
                                         C.c_float, c_fp, c_fp, c_fp, c_vp]),
    "pca_eval_tally": (C.c_int, [c_fp, c_i64p, C.c_int, C.c_int, c_i64p, C.c_int, c_vp]),
    "pca_clip_aggregate": (C.c_int, [c_fp, C.c_int64, C.c_int, c_i64p, C.c_int, c_i64p, c_fp, c_vp,
                                     c_i64p, c_i64p, C.c_int, c_vp]),
    "pca_eval_metrics": (C.c_int, [c_fp, c_i64p, C.c_int64, C.c_int, C.c_int, c_fp, c_i64p, c_vp,
                                   c_i64p, C.c_int, c_i64p, c_vp, c_vp, c_vp]),
    "pca_eval_metrics_ws_bytes": (C.c_size_t, [C.c_int64]),
    "pca_debug_poison_lds":(C.c_int, [c_vp]),
    "pca_subsample_points": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_fp, c_fp, c_vp,
                                       C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                       C.c_uint64, C.c_uint64, c_vp, c_fp, c_vp, c_vp, c_vp,
                                       c_vp]),
    "pca_importance_points": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_fp, c_fp, c_vp,
                                        C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                        C.c_int, C.c_uint64, C.c_uint64, c_vp, c_fp, c_vp, c_fp,
                                        c_vp, c_vp, c_vp]),
    "pca_pack_points_2d_ss": (C.c_int, [c_fp, c_fp, c_vp, C.c_int, C.c_int, c_fp, c_vp, c_vp,
                                        c_vp]),
    "pca_frame_points": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p, c_i64p,
                                   C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp,
                                   C.POINTER(PcaFrameAug), c_fp, c_i64p, c_vp, c_vp]),
    "pca_frame_points_multires": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p,
                                            c_i64p, C.c_int, C.POINTER(PcaFrameLevel), C.c_int, C.c_int64,
                                            C.POINTER(PcaFrameAug), c_fp, c_i64p, c_vp, c_vp]),
    "pca_frame_points_bands": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p, c_i64p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp,
                                         C.POINTER(PcaFrameAug), C.POINTER(PcaFrameBands), c_fp, c_i64p,
                                         c_vp, c_vp]),
    "pca_frame_points_pcen": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p, c_i64p,
                                        C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp,
                                        C.POINTER(PcaFrameAug), C.POINTER(PcaFrameBands), C.POINTER(PcaPcen),
                                        c_vp, C.c_int64, c_vp, c_fp, c_i64p, c_vp, c_vp]),
    "pca_frame_points_delta": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p, c_i64p,
                                         C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp,
                                         C.POINTER(PcaFrameAug), C.POINTER(PcaFrameBands), C.POINTER(PcaDelta),
                                         c_fp, C.c_int64, c_vp, c_fp, c_i64p, c_vp, c_vp]),
    "pca_frame_points_reassigned": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p,
                                              c_i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                              c_fp, C.POINTER(PcaFrameAug), C.POINTER(PcaReassignSpec),
                                              c_fp, c_i64p, c_vp, c_vp]),
    "pca_clip_rms": (C.c_int, [c_fp, c_i64p, C.c_int, C.c_int64, c_vp, c_vp]),
    "pca_frame_points_ex": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p, c_i64p,
                                      C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp, c_fp,
                                      C.POINTER(PcaFrameAugEx), c_fp, c_i64p, c_vp, c_fp, c_vp]),
    "pca_frame_points_ex_targets": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p,
                                              c_i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                              c_fp, C.POINTER(PcaFrameAugEx), c_fp, c_i64p, c_vp, c_fp,
                                              c_i64p, c_i64p, c_fp, c_vp]),
    "pca_frame_points_masked": (C.c_int, [c_fp, c_i64p, c_i64p, C.c_int, C.c_int64, C.c_int64, c_i64p,
                                          c_i64p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, c_fp,
                                          c_fp, C.POINTER(PcaFrameAugEx), c_fp, c_i64p, c_vp, c_fp,
                                          c_i64p, c_i64p, c_fp, C.POINTER(PcaPointMask), c_vp, c_vp,
                                          c_vp]),
    "pca_baseline_param_count": (C.c_int64, [C.c_int, C.c_int, C.c_int, c_vp, C.c_int, C.c_int]),
    "pca_fb_forward": (C.c_int, [c_fp, C.c_int64, C.c_int64, c_i64p, C.c_int, C.c_int, c_vp,
                                 C.c_int, C.c_int, c_fp, C.c_int64, C.c_int, C.c_int, C.c_uint64,
                                 C.c_uint64, c_vp, c_fp, c_vp, c_vp, c_vp, c_vp]),
    "pca_cnn_temp_forward": (C.c_int, [c_fp, C.c_int64, C.c_int64, C.c_int64, c_i64p, C.c_int,
                                       C.c_int, C.c_int, C.c_int, c_vp, C.c_int, C.c_int, c_fp,
                                       C.c_int64, C.c_int, C.c_int, C.c_uint64, C.c_uint64, c_vp,
                                       c_fp, c_vp, c_vp, c_vp, c_vp]),
    "pca_adam_step": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int64, C.c_float, C.c_float,
                                C.c_float, C.c_float, C.c_float, C.c_float, c_vp, C.c_int, c_vp]),
    "pca_grad_sumsq_partials": (C.c_int64, [C.c_int64]),
    "pca_grad_sumsq": (C.c_int, [c_fp, C.c_int64, c_vp, C.c_int, c_vp]),
    "pca_adam_step_ex": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int64, C.POINTER(OptimCfg), c_vp,
                                   C.c_int, c_fp, C.c_int64, c_vp, c_vp, C.c_int, c_vp]),
    "pca_adam_step_groups": (C.c_int, [c_fp, c_fp, c_fp, c_fp, C.c_int64, C.POINTER(OptimCfg), c_vp,
                                       C.c_int, c_fp, C.c_int64, c_vp, c_vp, C.c_int,
                                       C.POINTER(OptimGroups), c_i64p, c_vp]),
    "pca_st_param_count": (C.c_int64, [C.POINTER(StConfig)]),
    "pca_st_bucket_split": (C.c_int64, [C.POINTER(StConfig)]),
    "pca_st_ws_bytes": (C.c_size_t, [C.POINTER(StConfig), C.c_int]),
    "pca_st_step_reproducible": (C.c_int, [C.POINTER(StConfig), C.c_int]),
    "pca_st_ws_layout": (C.c_int, [C.POINTER(StConfig), C.c_void_p]),
    "pca_st_handoff_counter": (C.c_int, [C.POINTER(StConfig), C.c_void_p, C.POINTER(C.c_void_p)]),
    "pca_st_forward": (C.c_int, [C.POINTER(StConfig), c_fp, c_fp, c_vp, c_fp, c_vp, c_vp]),
    "pca_st_pool_attention_ws_bytes": (C.c_size_t, [C.POINTER(StConfig)]),
    "pca_st_pool_attention": (C.c_int, [C.POINTER(StConfig), c_fp, c_fp, c_vp, c_fp, c_fp, c_fp, c_vp,
                                        c_vp]),
    "pca_st_train_fwd_bwd": (C.c_int, [C.POINTER(StConfig), c_fp, c_fp, c_vp, c_i64p, c_fp,
                                       c_fp, c_fp, c_fp, C.c_float, C.c_int, c_vp, c_vp]),
    "pca_st_train_fwd_bwd_soft": (C.c_int, [C.POINTER(StConfig), c_fp, c_fp, c_vp, c_i64p,
                                            C.POINTER(PcaSoftTargets), c_fp, c_fp, c_fp, c_fp,
                                            C.c_float, C.c_int, c_vp, c_vp]),
    "pca_prof_start": (C.c_int, [C.c_int, C.c_int]),
    "pca_prof_stop": (C.c_int, [C.POINTER(C.c_double), C.POINTER(C.c_int64),
                                C.POINTER(C.c_double), C.POINTER(C.c_double)]),
    "pca_gemm_f32": (C.c_int, [C.POINTER(GemmDesc), c_fp, c_fp, c_fp, c_fp, c_vp]),
    "pca_gemm_bf16": (C.c_int, [C.POINTER(GemmDesc), c_fp, c_fp, c_fp, c_fp, c_vp]),
    "pca_softmax_rows": (C.c_int, [c_fp, C.c_int64, C.c_int, C.c_float, c_vp]),
    "pca_softmax_bwd_rows": (C.c_int, [c_fp, c_fp, C.c_int64, C.c_int, C.c_float, c_vp]),
    "pca_colsum": (C.c_int, [c_fp, C.c_int64, C.c_int, c_fp, C.c_int, c_vp]),
}

# exported for tests and experiments, outside the documented ABI (not in include/pca_hip.h)
DEBUG_SIGNATURES = {
    "pca_debug_tail_plan": (C.c_int, [c_i64p, C.c_int, c_i64p, C.c_int]),
    "pca_debug_mid_nparts": (C.c_int, [C.c_int, C.c_int, C.c_int]),
    "pca_debug_prep_plan": (C.c_int, [c_i64p, C.c_int, c_i64p, C.c_int]),
    "pca_debug_prep_images": (C.c_int, [C.POINTER(C.c_void_p), C.POINTER(C.c_void_p), C.POINTER(C.c_int),
                                        C.POINTER(C.c_int), C.POINTER(C.c_int), C.c_int, c_vp]),
    "pca_debug_merge_factor": (C.c_float, [C.c_float, C.c_float, C.c_int]),
    "pca_debug_set128_shape_ok": (C.c_int, [C.c_int] * 8),
}

_lib = None
_lock = threading.Lock()


class PcaHipError(RuntimeError):
    pass


def lib() -> C.CDLL:
    """Load libpca_hip.so once; raise loudly if it is not there."""
    global _lib
    if _lib is not None:
        return _lib
    with _lock:
        if _lib is not None:
            return _lib
        if not os.path.exists(LIB_PATH):
            raise PcaHipError(
                f"{LIB_PATH} not found: build it with point-cloud-audio_amd/csrc/build.sh "
                "(or __graft_entry__.build()); there is no fallback path")
        handle = C.CDLL(LIB_PATH)
        for name, (res, args) in {**SIGNATURES, **DEBUG_SIGNATURES}.items():
            fn = getattr(handle, name)       # AttributeError if the symbol is missing
            fn.restype = res
            fn.argtypes = args
        _lib = handle
    return _lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = lib().pca_last_error()
        raise PcaHipError(f"{what} failed (rc={rc}): {msg.decode() if msg else ''}")
