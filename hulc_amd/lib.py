"""ctypes binding of libhulc_hip.so (include/hulc_hip.h).  No CPU fallback: a missing library raises."""
from __future__ import annotations

import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libhulc_hip.so")

KIND = {"hulc": 0, "gcbc": 1, "mcil": 2, "mcil_gru": 3}
DTYPE = {"fp32": 0, "bf16": 1, "fp16": 2}


class HulcConfig(C.Structure):
    _fields_ = [("kind", C.c_int32), ("dtype", C.c_int32), ("max_batch", C.c_int32), ("max_seq", C.c_int32),
                ("max_window", C.c_int32), ("use_clip", C.c_int32), ("kl_beta", C.c_float),
                ("kl_balancing_mix", C.c_float), ("dropout_p", C.c_float), ("num_classes", C.c_int32),
                ("gripper_alpha", C.c_float), ("log_scale_min", C.c_float), ("seed", C.c_uint64)]


class HulcBatch(C.Structure):
    _fields_ = [("B", C.c_int32), ("S", C.c_int32), ("is_lang", C.c_int32), ("rgb_static", C.c_void_p),
                ("rgb_gripper", C.c_void_p), ("actions", C.c_void_p), ("robot_obs", C.c_void_p), ("lang", C.c_void_p),
                ("plan_idx", C.c_void_p), ("aux_rows", C.c_void_p), ("n_aux", C.c_int32), ("step", C.c_uint64),
                ("frames_u8", C.c_int32), ("pad_static", C.c_int32), ("pad_gripper", C.c_int32), ("shift_static", C.c_void_p),
                ("shift_gripper", C.c_void_p), ("plan_eps", C.c_void_p), ("actions_absolute", C.c_int32), ("max_rel_pos", C.c_float),
                ("max_rel_orn", C.c_float), ("window_start", C.c_void_p), ("store_frames", C.c_int64), ("window_len", C.c_void_p),
                ("window_len_host", C.c_void_p)]      # HOST (B) int32: the ragged encoder pass


class HulcStoreTables(C.Structure):
    """hulc_store_tables: the per-frame tables next to a frame store (hulc_store_gather)."""
    _fields_ = [("actions", C.c_void_p), ("robot_obs", C.c_void_p), ("lang", C.c_void_p), ("store_frames", C.c_int64), ("lang_rows", C.c_int32), ("absolute", C.c_int32)]


class HulcStageCopy(C.Structure):
    """hulc_stage_copy: one copy of hulc_store_stage (src pinned host or device, dst device)."""
    _fields_ = [("src", C.c_void_p), ("dst", C.c_void_p), ("bytes", C.c_int64)]


class HulcValNoise(C.Structure):
    _fields_ = [("plan_idx_pp", C.c_void_p), ("plan_idx_pr", C.c_void_p), ("u_mix_pp", C.c_void_p), ("u_act_pp", C.c_void_p),
                ("u_mix_pr", C.c_void_p), ("u_act_pr", C.c_void_p)]


class HulcRolloutObs(C.Structure):
    _fields_ = [("rgb_static", C.c_void_p), ("rgb_gripper", C.c_void_p), ("robot_obs_raw", C.c_void_p)]


class HulcRolloutEnvsObs(C.Structure):
    """hulc_rollout_envs_obs: the rows of one batched multi-environment rollout call; `slots` is a HOST int32 array (or NULL = rows 0..n-1)."""
    _fields_ = [("n", C.c_int32), ("slots", C.c_void_p), ("rgb_static", C.c_void_p), ("rgb_gripper", C.c_void_p), ("robot_obs_raw", C.c_void_p)]


class HulcOptim(C.Structure):
    _fields_ = [("kind", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("weight_decay", C.c_float),
                ("momentum", C.c_float), ("dampening", C.c_float), ("nesterov", C.c_int32), ("step", C.c_int64), ("grad_scale", C.c_float)]


DECODER = {"logistic": 0, "deterministic": 1}      # HULC_DECODER_*
CRITERION = {"HuberLoss": 0, "MSELoss": 1}         # HULC_CRIT_*
BODY = {"rnn": 0, "mlp": 1}                        # HULC_BODY_*
OPTIM = {"adam": 0, "adamw": 1, "sgd": 2}
CLIP = {"off": 0, "norm": 1, "value": 2}      # HULC_CLIP_*


class HulcSbertConfig(C.Structure):
    _fields_ = [("layers", C.c_int32), ("hidden", C.c_int32), ("heads", C.c_int32), ("intermediate", C.c_int32), ("vocab", C.c_int32),
                ("max_position", C.c_int32), ("max_sentences", C.c_int32), ("max_tokens", C.c_int32), ("normalize", C.c_int32), ("ln_eps", C.c_float)]


class HulcConvJob(C.Structure):      # hulc_conv_job
    _fields_ = [("input", C.c_void_p), ("w", C.c_void_p), ("bias", C.c_void_p), ("out", C.c_void_p), ("bits", C.c_void_p),
                ("frames", C.c_int32), ("in_side", C.c_int32), ("out_side", C.c_int32)]


class HulcEncTailJob(C.Structure):      # hulc_enc_tail_job
    _fields_ = [("x", C.c_void_p), ("W1", C.c_void_p), ("W2", C.c_void_p), ("b1", C.c_void_p), ("b2", C.c_void_p), ("lng", C.c_void_p), ("lnb", C.c_void_p),
                ("f1", C.c_void_p), ("f2", C.c_void_p), ("lnst", C.c_void_p), ("col0", C.c_int32)]


class HulcEncTailBwdJob(C.Structure):      # hulc_enc_tail_bwd_job
    _fields_ = [("f2", C.c_void_p), ("lnst", C.c_void_p), ("lng", C.c_void_p), ("f1", C.c_void_p), ("W2t", C.c_void_p), ("W1t", C.c_void_p), ("xmask", C.c_void_p),
                ("dlng", C.c_void_p), ("dlnb", C.c_void_p), ("d_f2", C.c_void_p), ("d_f1", C.c_void_p), ("dx_f32", C.c_void_p), ("dx_t", C.c_void_p), ("col0", C.c_int32)]


class HulcTrLayerJob(C.Structure):      # hulc_tr_layer_job
    _fields_ = [(n, C.c_void_p) for n in ("xin", "ln_g", "ln_b", "xf_out", "xt_out", "st_out", "Wqkv", "Wo", "W1", "W2", "bqkv", "bo", "b1", "b2", "n1g", "n1b",
                                          "qkv", "Pat", "ao", "y1", "st1", "x1t", "x1f", "hff", "y2")] + \
               [(n, C.c_uint64) for n in ("seed_att", "seed_o", "seed_h", "seed_y")]


class HulcTrFfnBwdJob(C.Structure):      # hulc_tr_ffn_bwd_job
    _fields_ = [(n, C.c_void_p) for n in ("dx", "y2", "st2", "n2g", "dg2", "db2", "W2t", "W1t", "hff", "dt_c", "dt_a", "part")] + [("seed_y", C.c_uint64)]


class HulcTrAttnBwdJob(C.Structure):      # hulc_tr_attn_bwd_job
    _fields_ = [(n, C.c_void_p) for n in ("parts", "y1", "st1", "n1g", "dg1", "db1", "Wot", "Wint", "qkv", "Pat", "b_d", "b_b", "dy_f", "dx")] + \
               [("seed_o", C.c_uint64), ("seed_att", C.c_uint64)]


class HulcGemmEpiJob(C.Structure):      # hulc_gemm_epi_job: EpiP field for field, behind the operands, the output map and the split
    _fields_ = [("A", C.c_void_p), ("B", C.c_void_p), ("M", C.c_int32), ("N", C.c_int32), ("K", C.c_int32), ("lda", C.c_int64), ("ldb", C.c_int64),
                ("ldc", C.c_int64), ("out_R1", C.c_int32), ("out_s0", C.c_int64), ("nsplit", C.c_int32), ("wfrag", C.c_int32),
                ("out", C.c_void_p), ("out_f32", C.c_int32), ("accumulate", C.c_int32), ("atomic", C.c_int32), ("z_stride", C.c_int64),
                ("bias", C.c_void_p), ("bias2", C.c_void_p), ("res", C.c_void_p), ("res_f32", C.c_int32), ("res_ld", C.c_int64), ("res_rowmod", C.c_int32),
                ("res_late", C.c_int32), ("mask", C.c_void_p), ("mask_tanh", C.c_int32), ("relu", C.c_int32), ("alpha", C.c_float), ("drop_p", C.c_float),
                ("drop_seed", C.c_uint64), ("out2", C.c_void_p), ("out2_lo", C.c_int64), ("out2_hi", C.c_int64), ("out2_mask", C.c_void_p),
                ("out2_relu", C.c_int32), ("generic_only", C.c_int32)]


GEMM_RAN = {"none": 0, "32": 1, "64": 2, "128": 3, "glds": 4, "skinny_router": 5, "skinny_reg": 6, "kchunk": 7, "splitk_64": 8, "splitk_128": 9,
            "dual": 12}      # HULC_GEMM_RAN_* (10 and 11: retired launch forms)

EXPORTS = ["hulc_last_error", "hulc_ctx_create", "hulc_ctx_destroy", "hulc_set_stream", "hulc_workspace_bytes",
           "hulc_bind_params", "hulc_prepare_weights", "hulc_zero_grads", "hulc_flush_grads", "hulc_forward_loss", "hulc_forward_loss_pair", "hulc_backward", "hulc_backward_part",
           "hulc_adam_step", "hulc_optimizer_step", "hulc_comm_unique_id", "hulc_comm_prepare", "hulc_comm_init", "hulc_comm_destroy", "hulc_comm_buckets", "hulc_comm_stats", "hulc_comm_size", "hulc_comm_timeline", "hulc_allreduce_grads", "hulc_backward_allreduce", "hulc_scaler_enable", "hulc_scaler_get", "hulc_scaler_set", "hulc_grad_clip_set", "hulc_grad_norm_get", "hulc_validate", "hulc_store_gather", "hulc_store_stage", "hulc_store_stage_join", "hulc_store_stage_stats", "hulc_clip_gt_encode", "hulc_clip_gt_scores", "hulc_aux_heads_enable", "hulc_decoder_select", "hulc_aux_weights_set", "hulc_aux_losses_get", "hulc_rollout_reset", "hulc_rollout_plan", "hulc_rollout_act", "hulc_rollout_get_goal", "hulc_rollout_set_state", "hulc_rollout_envs_init", "hulc_rollout_envs_reset", "hulc_rollout_envs_plan", "hulc_rollout_envs_act", "hulc_rollout_envs_get_state", "hulc_rollout_envs_set_state", "hulc_sbert_create", "hulc_sbert_destroy", "hulc_sbert_set_stream", "hulc_sbert_bind", "hulc_sbert_encode", "hulc_set_kl_beta", "hulc_set_dropout", "hulc_set_option", "hulc_get_option", "hulc_timers_enable", "hulc_timers_read", "hulc_get_tensor", "hulc_get_plan_idx", "hulc_k_gemm_nt", "hulc_k_cast", "hulc_k_trread_probe", "hulc_k_conv_wgrad", "hulc_k_conv1_wgrad_u8", "hulc_k_conv1_interior_groups", "hulc_k_conv_tile", "hulc_k_camera_split", "hulc_k_conv_pair", "hulc_k_skinny", "hulc_k_attention", "hulc_k_rnn_persist", "hulc_k_rnn_persist_flag_words", "hulc_k_clip_loss", "hulc_k_clip_loss_fp32", "hulc_k_mia_head", "hulc_k_cosine_dist", "hulc_k_spatial_softmax64", "hulc_k_enc_tail_fwd", "hulc_k_enc_tail_bwd", "hulc_k_logistic_loss",
           "hulc_k_plan_kl_sample", "hulc_k_st_softmax_bwd", "hulc_k_plan_gather", "hulc_k_plan_scatter_grad", "hulc_k_normal_kl_sample", "hulc_k_normal_rsample_bwd",
           "hulc_k_layernorm_fwd", "hulc_k_layernorm_bwd", "hulc_k_layernorm_mean", "hulc_k_tr_layer_fwd", "hulc_k_tr_ffn_bwd", "hulc_k_tr_attn_bwd",
           "hulc_k_window_compact", "hulc_k_rows_expand", "hulc_k_rows_reduce", "hulc_k_gemm_epi", "hulc_k_gemm_dual", "hulc_k_gemm_pick", "hulc_k_gemm_wgrad_nsplit",
           "hulc_k_det_head_loss", "hulc_k_det_head_bwd", "hulc_k_det_head_act",
           "hulc_k_conv_wgrad_t", "hulc_k_conv1_wgrad_u8_t", "hulc_k_conv_tile_t", "hulc_k_conv_pair_t", "hulc_k_conv_plan",
           "hulc_decoder_body_select", "hulc_trainable_set", "hulc_trainable_get", "hulc_trainable_steps_set",
           "hulc_ema_enable", "hulc_ema_state_get", "hulc_ema_state_set", "hulc_ema_swap", "hulc_ema_swapped", "hulc_k_ema_update",
           "hulc_k_lin_bwd_stream"]

_lib = None


def load():
    """Load the HIP library; raises RuntimeError (never falls back) when it is absent or unloadable."""
    global _lib
    if _lib is not None:
        return _lib
    # HULC_LIB_PATH: another BUILD of the same library (an older commit's, an experiment's) for same-box A/B runs of whole builds (tools/ab_lib.sh); never a fallback —
    # a path that does not exist is an error like a missing in-tree build
    path = os.environ.get("HULC_LIB_PATH") or LIB_PATH
    if not os.path.exists(path):
        raise RuntimeError(f"hulc_amd: {path} not built — run `python -c 'import __graft_entry__ as g; g.build()'`; "
                           "there is no CPU fallback for the product path")
    # torch ships its own libamdhip64; it must be the HIP runtime of the process.  Loading this library first would pull in
    # /opt/rocm's copy and a later `import torch` then sees no device ("hulc_ctx_create: no HIP device visible").
    import torch  # noqa: F401
    lib = C.CDLL(path)
    lib.hulc_last_error.restype = C.c_char_p
    lib.hulc_workspace_bytes.restype = C.c_int64
    lib.hulc_ctx_create.argtypes = [C.POINTER(HulcConfig), C.POINTER(C.c_void_p)]
    lib.hulc_ctx_destroy.argtypes = [C.c_void_p]
    lib.hulc_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.hulc_workspace_bytes.argtypes = [C.c_void_p]
    lib.hulc_bind_params.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int32,
                                     C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.hulc_prepare_weights.argtypes = [C.c_void_p]
    lib.hulc_zero_grads.argtypes = [C.c_void_p]
    if os.environ.get("HULC_LIB_PATH") and not hasattr(lib, "hulc_flush_grads"):      # an older build under A/B: the entry points it predates stay unbound
        lib.hulc_zero_grads.argtypes = [C.c_void_p]
    else:
        lib.hulc_flush_grads.argtypes = [C.c_void_p]
    lib.hulc_forward_loss.argtypes = [C.c_void_p, C.POINTER(HulcBatch), C.c_float, C.c_float, C.c_void_p, C.c_int32]
    lib.hulc_forward_loss_pair.argtypes = [C.c_void_p, C.POINTER(HulcBatch), C.POINTER(HulcBatch), C.c_float, C.c_float, C.c_void_p, C.c_int32]
    lib.hulc_backward.argtypes = [C.c_void_p]
    lib.hulc_backward_part.argtypes = [C.c_void_p, C.c_int32]
    lib.hulc_adam_step.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_float, C.c_int64, C.c_float]
    lib.hulc_optimizer_step.argtypes = [C.c_void_p, C.POINTER(HulcOptim)]
    lib.hulc_comm_unique_id.argtypes = [C.c_void_p, C.c_int64]
    lib.hulc_comm_prepare.argtypes = [C.c_void_p]
    lib.hulc_comm_init.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.hulc_comm_destroy.argtypes = [C.c_void_p]
    lib.hulc_comm_buckets.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]
    lib.hulc_comm_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_double)]
    if hasattr(lib, "hulc_comm_size") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_comm_size.argtypes = [C.c_void_p, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    lib.hulc_comm_timeline.argtypes = [C.c_void_p, C.POINTER(C.c_double), C.c_int32, C.POINTER(C.c_double)]
    lib.hulc_allreduce_grads.argtypes = [C.c_void_p, C.c_int32]
    lib.hulc_backward_allreduce.argtypes = [C.c_void_p, C.c_int32]
    lib.hulc_scaler_enable.argtypes = [C.c_void_p, C.c_float, C.c_float, C.c_float, C.c_int32]
    lib.hulc_scaler_get.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int64)]
    lib.hulc_scaler_set.argtypes = [C.c_void_p, C.c_float, C.c_int32, C.c_int64]
    if hasattr(lib, "hulc_grad_clip_set") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_grad_clip_set.argtypes = [C.c_void_p, C.c_int32, C.c_float, C.c_int32]
        lib.hulc_grad_norm_get.argtypes = [C.c_void_p, C.POINTER(C.c_float), C.POINTER(C.c_float), C.c_void_p, C.c_int64]
    lib.hulc_clip_gt_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32]
    lib.hulc_clip_gt_scores.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
    if hasattr(lib, "hulc_aux_heads_enable") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_aux_heads_enable.argtypes = [C.c_void_p, C.c_int32, C.c_int32]
        lib.hulc_aux_weights_set.argtypes = [C.c_void_p, C.c_float, C.c_float]
        lib.hulc_aux_losses_get.argtypes = [C.c_void_p, C.c_void_p]
    lib.hulc_validate.argtypes = [C.c_void_p, C.POINTER(HulcBatch), C.POINTER(HulcValNoise), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "hulc_store_gather") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_store_gather.argtypes = [C.c_void_p, C.POINTER(HulcStoreTables), C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "hulc_store_stage") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_store_stage.restype = C.c_int64
        lib.hulc_store_stage.argtypes = [C.c_void_p, C.POINTER(HulcStageCopy), C.c_int32]
        lib.hulc_store_stage_join.argtypes = [C.c_void_p, C.c_int64]
        lib.hulc_store_stage_stats.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.hulc_rollout_reset.argtypes = [C.c_void_p]
    lib.hulc_rollout_plan.argtypes = [C.c_void_p, C.POINTER(HulcRolloutObs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hulc_rollout_act.argtypes = [C.c_void_p, C.POINTER(HulcRolloutObs), C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hulc_rollout_get_goal.argtypes = [C.c_void_p, C.c_void_p]
    lib.hulc_rollout_set_state.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "hulc_rollout_envs_init") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_rollout_envs_init.argtypes = [C.c_void_p, C.c_int32]
        lib.hulc_rollout_envs_reset.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32]
        lib.hulc_rollout_envs_plan.argtypes = [C.c_void_p, C.POINTER(HulcRolloutEnvsObs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_rollout_envs_act.argtypes = [C.c_void_p, C.POINTER(HulcRolloutEnvsObs), C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_rollout_envs_get_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_rollout_envs_set_state.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hulc_sbert_create.argtypes = [C.POINTER(HulcSbertConfig), C.POINTER(C.c_void_p)]
    lib.hulc_sbert_destroy.argtypes = [C.c_void_p]
    lib.hulc_sbert_set_stream.argtypes = [C.c_void_p, C.c_void_p]
    lib.hulc_sbert_bind.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_int32, C.POINTER(C.c_char_p), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]
    lib.hulc_sbert_encode.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    lib.hulc_set_kl_beta.argtypes = [C.c_void_p, C.c_float]
    lib.hulc_set_dropout.argtypes = [C.c_void_p, C.c_float]
    lib.hulc_timers_enable.argtypes = [C.c_void_p, C.c_int32, C.c_char_p]
    lib.hulc_set_option.argtypes = [C.c_void_p, C.c_char_p, C.c_int64]
    lib.hulc_get_option.argtypes = [C.c_void_p, C.c_char_p, C.POINTER(C.c_int64)]
    lib.hulc_k_rnn_persist.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_uint32, C.c_void_p]
    lib.hulc_k_rnn_persist_flag_words.restype = C.c_int32
    lib.hulc_timers_read.argtypes = [C.c_void_p, C.c_char_p, C.c_int64, C.c_int32]
    lib.hulc_get_tensor.argtypes = [C.c_void_p, C.c_char_p, C.c_void_p, C.c_int64, C.POINTER(C.c_int64)]
    lib.hulc_get_plan_idx.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
    lib.hulc_k_gemm_nt.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int64,
                                   C.c_int64, C.c_int64, C.c_void_p, C.c_int32, C.c_void_p]
    lib.hulc_k_conv_wgrad.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p]
    if hasattr(lib, "hulc_k_conv1_wgrad_u8") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_k_conv1_interior_groups.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.hulc_k_conv1_wgrad_u8.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.hulc_k_conv_tile.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32,
                                     C.c_int32, C.c_void_p]
    if hasattr(lib, "hulc_k_conv_pair") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_k_camera_split.argtypes = [C.c_int32, C.c_double, C.c_double, C.POINTER(C.c_int32), C.POINTER(C.c_int32)]
        lib.hulc_k_conv_pair.argtypes = [C.c_int32, C.POINTER(HulcConvJob), C.POINTER(HulcConvJob), C.c_int32, C.c_int32, C.c_void_p]
    lib.hulc_k_skinny.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p]
    lib.hulc_k_trread_probe.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hulc_k_cast.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]
    if hasattr(lib, "hulc_k_clip_loss") or not os.environ.get("HULC_LIB_PATH"):
        for f in (lib.hulc_k_clip_loss, lib.hulc_k_clip_loss_fp32):
            f.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_k_mia_head.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_k_cosine_dist.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    lib.hulc_k_attention.argtypes = [C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_uint64, C.c_void_p]
    if hasattr(lib, "hulc_k_enc_tail_fwd") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_k_spatial_softmax64.argtypes = [C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_k_enc_tail_fwd.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HulcEncTailJob), C.POINTER(HulcEncTailJob), C.c_void_p, C.c_void_p, C.c_int32,
                                            C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        lib.hulc_k_enc_tail_bwd.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.POINTER(HulcEncTailBwdJob), C.POINTER(HulcEncTailBwdJob), C.c_void_p, C.c_void_p]
        lib.hulc_k_logistic_loss.argtypes = [C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_int32,
                                             C.c_float, C.c_float, C.c_int32, C.c_int32, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    if hasattr(lib, "hulc_k_layernorm_bwd") or not os.environ.get("HULC_LIB_PATH"):
        P, I, F, U, Q = C.c_void_p, C.c_int32, C.c_float, C.c_uint64, C.c_int64
        lib.hulc_k_plan_kl_sample.argtypes = [P, P, I, I, I, P, P, P, P, P, P, F, F, U, P, P]
        lib.hulc_k_st_softmax_bwd.argtypes = [I, P, P, P, P, I, I, P, P, P, P]
        lib.hulc_k_plan_gather.argtypes = [I, P, P, I, I, I, I, P, P, P, P, P, I, I, P, I, I, P, P]
        lib.hulc_k_plan_scatter_grad.argtypes = [I, I, P, P, I, I, I, I, I, P, I, P]
        lib.hulc_k_normal_kl_sample.argtypes = [I, P, P, I, I, P, P, P, P, P, P, P, F, F, U, P, P]
        lib.hulc_k_normal_rsample_bwd.argtypes = [I, P, P, P, P, I, I, P, P]
        lib.hulc_k_layernorm_fwd.argtypes = [I, P, Q, I, I, P, P, P, Q, P, Q, P, P]
        lib.hulc_k_layernorm_bwd.argtypes = [I, P, Q, P, Q, P, P, I, I, P, Q, I, P, Q, P, P, F, U, I, F, I, Q, P, P]
        lib.hulc_k_layernorm_mean.argtypes = [I, P, I, I, I, P, P, P, P, P, P]
    if hasattr(lib, "hulc_k_tr_layer_fwd") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_k_tr_layer_fwd.argtypes = [C.c_int32, C.POINTER(HulcTrLayerJob), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_void_p]
        lib.hulc_k_tr_ffn_bwd.argtypes = [C.c_int32, C.POINTER(HulcTrFfnBwdJob), C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float, C.c_void_p]
        lib.hulc_k_tr_attn_bwd.argtypes = [C.c_int32, C.POINTER(HulcTrAttnBwdJob), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_float, C.c_void_p]
    if hasattr(lib, "hulc_k_rows_reduce") or not os.environ.get("HULC_LIB_PATH"):
        P, I, Q = C.c_void_p, C.c_int32, C.c_int64
        lib.hulc_k_window_compact.argtypes = [P, P, P, I, I, I, Q, P, P, P, P, P, P]
        lib.hulc_k_rows_expand.argtypes = [I, P, P, P, I, I, I, P, P]
        lib.hulc_k_rows_reduce.argtypes = [P, P, P, I, I, I, P, P]
    if hasattr(lib, "hulc_k_gemm_epi") or not os.environ.get("HULC_LIB_PATH"):
        I, Q, PI = C.c_int32, C.c_int64, C.POINTER(C.c_int32)
        lib.hulc_k_gemm_epi.argtypes = [I, C.POINTER(HulcGemmEpiJob), I, PI, C.c_void_p]
        lib.hulc_k_gemm_pick.argtypes = [I, I, I, I, Q, Q, PI, PI]
        lib.hulc_k_gemm_wgrad_nsplit.argtypes = [I, I, I, I, PI, PI]
    if hasattr(lib, "hulc_k_gemm_dual") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_k_gemm_dual.argtypes = [C.c_int32, C.POINTER(HulcGemmEpiJob), C.POINTER(C.c_int32), C.c_void_p]
    if hasattr(lib, "hulc_k_lin_bwd_stream") or not os.environ.get("HULC_LIB_PATH"):
        P, I, Q = C.c_void_p, C.c_int32, C.c_int64
        lib.hulc_k_lin_bwd_stream.argtypes = [I, P, P, Q, I, I, I, I, I, P, Q, P, P, P]
    if hasattr(lib, "hulc_decoder_select") or not os.environ.get("HULC_LIB_PATH"):
        P, I, F = C.c_void_p, C.c_int32, C.c_float
        lib.hulc_decoder_select.argtypes = [P, I, I]
        lib.hulc_k_det_head_loss.argtypes = [I, P, P, P, P, P, I, I, I, I, F, P, P, P, P, P]
        lib.hulc_k_det_head_bwd.argtypes = [I, P, P, P, I, I, P, P, P, P, P]
        lib.hulc_k_det_head_act.argtypes = [I, P, P, P, P, I, P, P]
    if hasattr(lib, "hulc_decoder_body_select") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_decoder_body_select.argtypes = [C.c_void_p, C.c_int32]
    if hasattr(lib, "hulc_trainable_set") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_trainable_set.argtypes = [C.c_void_p, C.c_int32, C.c_void_p]
        lib.hulc_trainable_get.argtypes = [C.c_void_p, C.c_int64, C.c_void_p, C.c_void_p]
        lib.hulc_trainable_steps_set.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int64]
    if hasattr(lib, "hulc_ema_enable") or not os.environ.get("HULC_LIB_PATH"):
        lib.hulc_ema_enable.argtypes = [C.c_void_p, C.c_void_p, C.c_float, C.c_int64, C.c_int32]
        lib.hulc_ema_state_get.argtypes = [C.c_void_p, C.POINTER(C.c_int64), C.POINTER(C.c_float)]
        lib.hulc_ema_state_set.argtypes = [C.c_void_p, C.c_int64]
        lib.hulc_ema_swap.argtypes = [C.c_void_p]
        lib.hulc_ema_swapped.argtypes = [C.c_void_p, C.POINTER(C.c_int32)]
        lib.hulc_k_ema_update.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p]
    if hasattr(lib, "hulc_k_conv_plan") or not os.environ.get("HULC_LIB_PATH"):
        P, I, PI = C.c_void_p, C.c_int32, C.POINTER(C.c_int32)
        lib.hulc_k_conv_wgrad_t.argtypes = [I, I, P, P, P, P, I, I, PI, P]
        lib.hulc_k_conv1_wgrad_u8_t.argtypes = [I, P, P, I, P, P, P, I, I, I, I, PI, P]
        lib.hulc_k_conv_tile_t.argtypes = [I, I, P, P, P, P, P, P, I, I, I, I, I, P]
        lib.hulc_k_conv_pair_t.argtypes = [I, I, C.POINTER(HulcConvJob), C.POINTER(HulcConvJob), I, I, PI, P]
        lib.hulc_k_conv_plan.argtypes = [I, I, I, I, I, PI, PI, PI, PI]
    _lib = lib
    return lib


def check(rc: int):
    if rc != 0:
        raise RuntimeError("libhulc_hip: " + load().hulc_last_error().decode("utf-8", "replace"))
