"""ctypes binding of the C ABI declared in ``include/lumina_dit.h`` (+ the diagnostics of ``include/lumina_dit_debug.h``).

The shared library is built in-tree by ``__graft_entry__.build()`` (``make -C lumina-t2x_amd/csrc``).
There is NO fallback: if the library is missing or a symbol cannot be resolved the import of the
product path fails loudly (the oracle under ``oracle/`` is test infrastructure and is never used here).
"""
from __future__ import annotations

import ctypes as C
import os
import re
from typing import Dict, List

_HERE = os.path.dirname(os.path.abspath(__file__))
# LUMINA_DIT_LIB: an alternate build of the same C ABI (A/B measurements of two kernel versions on one box); still no fallback
LIB_PATH = os.environ.get("LUMINA_DIT_LIB") or os.path.join(_HERE, "lib", "liblumina_dit.so")
HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lumina_dit.h")
DEBUG_HEADER_PATH = os.path.join(os.path.dirname(_HERE), "include", "lumina_dit_debug.h")  # options' documentation, the trace entry point, the row kernels' test entry points
LT_OPTION_INHERIT = -2 ** 31

LT_F32, LT_BF16, LT_F16 = 0, 1, 2
LT_VARIANT_NEXT_T2I, LT_VARIANT_NEXT_IMAGENET, LT_VARIANT_FLAG_T2I, LT_VARIANT_NEXT_MOE = 0, 1, 2, 3
LT_VARIANT_NEXT_MOE_TIME, LT_VARIANT_NEXT_MOE_SPACE = 4, 5
LT_SOFTMAX_T2I, LT_SOFTMAX_ANAGRAM = 0, 1
SOFTMAX_RULES = {"t2i": LT_SOFTMAX_T2I, "anagram": LT_SOFTMAX_ANAGRAM}
LT_PROJECT_APG, LT_PROJECT_ZERO_STAR = 1, 2  # the projected forms of lt_sample_ode_cfg_project / lt_forward_cfg_project
PROJECT_FORMS = {"apg": LT_PROJECT_APG, "zero_star": LT_PROJECT_ZERO_STAR}
LT_ODE_EULER, LT_ODE_MIDPOINT, LT_ODE_RK4 = 0, 1, 2
ODE_METHODS = {"euler": LT_ODE_EULER, "midpoint": LT_ODE_MIDPOINT, "rk4": LT_ODE_RK4}
LT_ODE_DOPRI5, LT_ODE_BOSH3, LT_ODE_FEHLBERG2, LT_ODE_ADAPTIVE_HEUN = 3, 4, 5, 6
ODE_ADAPTIVE_METHODS = {"dopri5": LT_ODE_DOPRI5, "bosh3": LT_ODE_BOSH3, "fehlberg2": LT_ODE_FEHLBERG2, "adaptive_heun": LT_ODE_ADAPTIVE_HEUN}
LT_ODE_AB2, LT_ODE_AB3, LT_ODE_ABM2, LT_ODE_ABM3 = 32, 33, 34, 35  # named where a call refuses them; lt_sample_ode_multistep takes the weight table
ODE_MULTISTEP_METHODS = {"ab2": LT_ODE_AB2, "ab3": LT_ODE_AB3, "abm2": LT_ODE_ABM2, "abm3": LT_ODE_ABM3}
LT_CACHE_PROBE, LT_CACHE_RUN, LT_CACHE_REUSE = 0, 1, 2
LT_COMPOSE_MAX = 7  # prompts of a composed-guidance call beside the base prompt (lt_forward_compose / lt_sample_ode_compose)
LT_RK_MAX_SLOPES, LT_RK_WS_BYTES = 7, 8192
LT_SDE_EULER, LT_SDE_HEUN = 0, 1
SDE_METHODS = {"Euler": LT_SDE_EULER, "Heun": LT_SDE_HEUN}
LT_SDE_LAST_NONE, LT_SDE_LAST_MEAN, LT_SDE_LAST_TWEEDIE, LT_SDE_LAST_EULER = 0, 1, 2, 3
SDE_LAST_STEPS = {None: LT_SDE_LAST_NONE, "Mean": LT_SDE_LAST_MEAN, "Tweedie": LT_SDE_LAST_TWEEDIE, "Euler": LT_SDE_LAST_EULER}
LT_SDE_REC = 8  # floats per stage record: t, r, var, D, q, dt, sqrt_dt, hdt (last step: t, r, var, D, h, a, c, 0)
(LT_SDE_OP_EULER, LT_SDE_OP_HEUN_XHAT, LT_SDE_OP_HEUN_K1, LT_SDE_OP_HEUN_OUT, LT_SDE_OP_LAST_MEAN, LT_SDE_OP_LAST_TWEEDIE,
 LT_SDE_OP_LAST_EULER) = range(7)


class LtConfig(C.Structure):
    _fields_ = [
        ("variant", C.c_int32), ("dim", C.c_int32), ("n_layers", C.c_int32), ("n_heads", C.c_int32),
        ("n_kv_heads", C.c_int32), ("ffn_hidden", C.c_int32), ("patch_size", C.c_int32),
        ("in_channels", C.c_int32), ("out_channels", C.c_int32), ("cap_feat_dim", C.c_int32),
        ("adaln_dim", C.c_int32), ("qk_norm", C.c_int32), ("num_classes", C.c_int32),
        ("norm_eps", C.c_float), ("max_batch", C.c_int32), ("max_tokens", C.c_int32),
        ("max_text", C.c_int32), ("rope_table_len", C.c_int32), ("num_experts", C.c_int32),
    ]


class LtStepArgs(C.Structure):
    _fields_ = [
        ("cfg_scale", C.c_float), ("scale_factor", C.c_float), ("scale_watershed", C.c_float),
        ("base_seqlen", C.c_int32), ("proportional_attn", C.c_int32), ("latent_h", C.c_int32),
        ("latent_w", C.c_int32), ("batch", C.c_int32), ("io_dtype", C.c_int32), ("cfg_channels", C.c_int32),
        ("ntk_factor", C.c_float),
    ]


class LtOdeAdaptiveStats(C.Structure):
    _fields_ = [
        ("nfe", C.c_int64), ("accepted", C.c_int32), ("rejected", C.c_int32), ("first_step", C.c_float), ("dt_cap", C.c_int32),
        ("dt_count", C.c_int32), ("dt_host", C.POINTER(C.c_float)),
    ]


class LuminaLibError(RuntimeError):
    pass


def header_text(strip_comments: bool = True) -> str:
    """both headers concatenated (the drop-in boundary, then the debug header)"""
    text = ""
    for path in (HEADER_PATH, DEBUG_HEADER_PATH):
        with open(path) as f:
            text += f.read() + "\n"
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S) if strip_comments else text


def declared_symbols() -> List[str]:
    """Names of every function the two headers declare (used by the ABI-export test)."""
    return sorted(set(re.findall(r"\b(lt_[a-z0-9_]+)\s*\(", header_text())))


_vp, _i32, _i64, _f32 = C.c_void_p, C.c_int32, C.c_int64, C.c_float

# name -> (restype, argtypes); mirrors include/lumina_dit.h + lumina_dit_debug.h one to one
_SIGNATURES: Dict[str, tuple] = {
    "lt_last_error": (C.c_char_p, []),
    "lt_version": (C.c_char_p, []),
    "lt_set_option": (_i32, [C.c_char_p, _i32]),
    "lt_engine_set_option": (_i32, [_vp, C.c_char_p, _i32]),
    "lt_engine_get_option": (_i32, [_vp, C.c_char_p, C.POINTER(_i32)]),
    "lt_create": (_i32, [C.POINTER(LtConfig), C.POINTER(_vp)]),
    "lt_destroy": (None, [_vp]),
    "lt_set_weight": (_i32, [_vp, C.c_char_p, _vp, _i32, C.POINTER(_i64), _i32, _vp]),
    "lt_weights_ready": (_i32, [_vp]),
    "lt_prepare_prompt": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp]),
    "lt_prepare_prompt_regional": (_i32, [_vp, _vp, _i32, _vp, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _vp]),
    "lt_prepare_labels": (_i32, [_vp, _vp, _i32, _vp]),
    "lt_forward": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_packed": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_i32), _vp, C.POINTER(_vp), C.POINTER(LtStepArgs), _vp]),
    "lt_forward_cfg_packed": (_i32, [_vp, _vp, C.POINTER(_i32), _vp, _vp, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_packed": (_i32, [_vp, _vp, C.POINTER(_i32), _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_cfg": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_masked": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_masked_packed": (_i32, [_vp, _vp, C.POINTER(_i32), _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32,
                                           C.POINTER(LtStepArgs), _vp]),
    "lt_set_views": (_i32, [_vp, _vp, C.POINTER(_f32), C.POINTER(_f32), _i32, _i32, _i32, _vp]),
    "lt_sample_views": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_set_windows": (_i32, [_vp, C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "lt_forward_tiled": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_tiled": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_compose": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_compose": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_set_softmax_rule": (_i32, [_vp, _i32]),
    "lt_sample_views_guided": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), C.POINTER(_f32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_sde": (_i32, [_vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, C.POINTER(_f32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_adaptive": (_i32, [_vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _f32, _f32, _f32, _i32, _i32, _i32, C.POINTER(LtStepArgs), _vp,
                                      C.POINTER(LtOdeAdaptiveStats)]),
    "lt_sample_ode_cfg_schedule": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_rule": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), _f32, _f32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_cfg_rule": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_project": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), _i32, _f32, _f32, _f32, _i32, _i32,
                                         C.POINTER(LtStepArgs), _vp]),
    "lt_forward_cfg_project": (_i32, [_vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_multistep": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, C.POINTER(_f32), _i32, C.POINTER(_f32), _f32, _f32, _i32, _i32,
                                       C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_multistep_packed": (_i32, [_vp, _vp, C.POINTER(_i32), _vp, _vp, C.POINTER(_f32), _i32, C.POINTER(_f32), _i32, _i32, _i32,
                                              C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_reuse": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), C.POINTER(_i32), _i32,
                                       C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_multistep_cfg_reuse": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, C.POINTER(_f32), _i32, C.POINTER(_f32), C.POINTER(_i32),
                                                 _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_cfg_reuse": (_i32, [_vp, _vp, _vp, _vp, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_flowedit": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), C.POINTER(_f32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_op_flowedit_mix": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, _i64, _i32, _vp]),
    "lt_op_flowedit_combine": (_i32, [_vp, _vp, _vp, _f32, _f32, _f32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_forward_skip": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), C.POINTER(_i32), _i32, _vp]),
    "lt_forward_cfg_slg": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, C.POINTER(_i32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_slg": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i32), _i32, _i32,
                                     C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cached": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32, C.POINTER(LtStepArgs), _f32, C.POINTER(C.c_double),
                                    C.POINTER(C.c_double), _vp]),
    "lt_forward_cached": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, C.POINTER(LtStepArgs), C.POINTER(C.c_double), _vp]),
    "lt_last_cache_hits": (_i64, [_vp]),
    "lt_debug_cache_read": (_i32, [_vp, _i32, _vp, _i64, _vp]),
    "lt_op_cache_ws_bytes": (_i32, []),
    "lt_op_cache_indicator": (_i32, [_vp, _vp, _i64, _vp, _vp, _vp]),
    "lt_op_cache_residual_store": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "lt_op_cache_residual_apply": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _vp]),
    "lt_forward_perturb": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), C.POINTER(_i32), _i32, C.POINTER(_i32), _i32, _vp]),
    "lt_forward_cfg_pag": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, C.POINTER(_i32), _i32, C.POINTER(_i32), _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_pag": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i32), _i32,
                                     C.POINTER(_i32), _i32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_forward_blur": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(LtStepArgs), C.POINTER(_i32), _i32, C.POINTER(_i32), _i32, _f32, _vp]),
    "lt_forward_cfg_seg": (_i32, [_vp, _vp, _vp, _vp, _f32, _f32, C.POINTER(_i32), _i32, C.POINTER(_i32), _i32, _f32, C.POINTER(LtStepArgs), _vp]),
    "lt_sample_ode_cfg_seg": (_i32, [_vp, _vp, _vp, _vp, C.POINTER(_f32), _i32, _i32, C.POINTER(_f32), C.POINTER(_f32), C.POINTER(_i32), _i32,
                                     C.POINTER(_i32), _i32, _f32, _i32, C.POINTER(LtStepArgs), _vp]),
    "lt_op_query_blur": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_seg_taps": (_i32, [_f32, C.POINTER(_f32), C.POINTER(_i32), C.POINTER(_i32)]),
    "lt_last_nfe": (_i64, [_vp]),
    "lt_last_eval_rows": (_i64, [_vp]),
    "lt_graph_replays": (_i64, [_vp]),
    "lt_moe_routing_record": (_i32, [_vp, _i32]),
    "lt_moe_routing_read": (_i32, [_vp, C.POINTER(_i32), _i32]),
    "lt_moe_routing_force": (_i32, [_vp, C.POINTER(_i32), _i32]),
    "lt_profile_enable": (_i32, [_vp, _i32]),
    "lt_profile_read": (_i32, [_vp, _i32, C.POINTER(C.c_double), C.POINTER(_i64), C.POINTER(C.c_double)]),
    "lt_profile_reset": (_i32, [_vp]),
    "lt_profile_enable_mask": (_i32, [_vp, _i32]),
    "lt_profile_set_budget": (_i32, [_vp, _i32, _i64]),
    "lt_profile_set_window": (_i32, [_vp, _i32, _i64, _i64]),
    "lt_op_gemm_bf16": (_i32, [_vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_pair_layout": (_i32, [_vp, _i64, _i32, _i32, _vp]),
    "lt_op_gemm_bf16_pair": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_gemm_vt": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_gemm_qkv": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_gemm_qkv_fusable": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32]),
    "lt_op_gemm_describe": (_i32, [_i32, _i32, _i32, _i32, _i32, C.c_char_p, _i32]),
    "lt_op_moe_plan": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _vp]),
    "lt_op_gemm_splitk": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "lt_op_gemm_splitk_auto": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "lt_op_gemm_grouped": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_gemm_grouped_tail": (_i32, [_vp, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "lt_op_gemm_grouped_gather": (_i32, [_vp, _i32, _vp, _vp, _vp, _i64, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_pack_w13": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "lt_op_rmsnorm_mod": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lt_op_gated_residual_norm": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _f32, _f32, _i32, _vp]),
    "lt_op_prep_mod": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, C.c_uint32, C.c_uint32, _i32, _vp]),
    "lt_op_qk_norm_rope": (_i32, [_vp, _i32, _i32, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _f32, _vp]),
    "lt_op_v_transpose": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_attention_identity": (_i32, [_vp, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_attention": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lt_op_qkv_attention_small": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _f32, _vp, _vp, _vp]),
    "lt_op_attention_describe": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_char_p, _i32]),
    "lt_op_attention_fused": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_attention_nk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp, _i32, _vp]),
    "lt_op_attention_fused_nk": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp]),
    "lt_op_attention_nk_describe": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_char_p, _i32]),
    "lt_op_attention_trace": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _vp, _vp]),
    "lt_op_views_invert": (_i32, [_vp, _vp, _vp, _i32, _i32, _vp]),
    "lt_op_views_gather": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_views_reduce": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_windows_gather": (_i32, [_vp, C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp]),
    "lt_op_windows_reduce": (_i32, [_vp, C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp]),
    "lt_op_windows_cover": (_i32, [C.POINTER(_i32), _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lt_op_compose_replicate": (_i32, [_vp, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_compose_guidance": (_i32, [_vp, _vp, C.POINTER(_f32), _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_views_guided_gather": (_i32, [_vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _f32, C.POINTER(_f32), _i32, _i32, _i32, _i32, _vp]),
    "lt_op_sde_step": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, C.POINTER(_f32), _i64, _i32, _vp]),
    "lt_op_rk_stage": (_i32, [_vp, C.POINTER(_vp), C.POINTER(_f32), _i32, _f32, _vp, _i64, _i32, _vp]),
    "lt_op_rk_error_norm": (_i32, [_vp, _vp, C.POINTER(_vp), C.POINTER(_f32), _i32, _f32, _f32, _f32, _vp, _vp, _vp, _i64, _i32, _vp]),
    "lt_op_rk_dense": (_i32, [_vp, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _vp, _i64, _i32, _vp]),
    "lt_op_rk_interp": (_i32, [C.POINTER(_vp), _f32, _vp, _i64, _i32, _vp]),
    "lt_op_rms_norm": (_i32, [_vp, _vp, _vp, _f32, _f32, _vp, _vp, _vp, _i64, _i32, _vp]),
    "lt_op_linear_small_m": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_patchify": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_eol_fill": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "lt_op_fill_rows_bf16": (_i32, [_vp, _vp, _i64, _i32, _vp]),
    "lt_op_label_gather": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "lt_op_cast_to_bf16": (_i32, [_vp, _i32, _vp, _i64, _vp]),
    "lt_op_upload_rows": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_mask_to_bias": (_i32, [_vp, _vp, _i32, _i32, _i32, _vp]),
    "lt_op_add_bf16": (_i32, [_vp, _vp, _vp, _i64, _vp]),
    "lt_op_timestep_features": (_i32, [_vp, _i32, _vp, _i32, _i32, _vp]),
    "lt_op_cap_pool_ln": (_i32, [_vp, _i32, _vp, _vp, _vp, _vp, _i32, _i32, _i32, _vp]),
    "lt_op_unpatchify_cfg_dev": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp]),
    "lt_op_guidance_slices": (_i32, []),
    "lt_op_guidance_stats": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _vp]),
    "lt_op_unpatchify_cfg_rule": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp]),
    "lt_op_guidance_project_stats": (_i32, [_vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp]),
    "lt_op_unpatchify_cfg_project": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp,
                                            _vp, _vp]),
    "lt_op_unpatchify_cfg_reuse": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _vp, _i32, _vp]),
    "lt_op_unpatchify_cfg_slg": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _vp, _i32, _vp]),
    "lt_op_unpatchify_cfg": (_i32, [_vp, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _i32, _vp]),
    "lt_op_packed_table": (_i32, [C.POINTER(_i32), _i32, _i32, _i32, C.POINTER(_i32), C.POINTER(_i64), C.POINTER(_i32)]),
    "lt_op_patchify_packed": (_i32, [_vp, _i32, _vp, C.POINTER(_i32), _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_fill_pad_packed": (_i32, [_vp, _vp, C.POINTER(_i32), _vp, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_unpatchify_packed": (_i32, [_vp, _i32, _vp, _i32, C.POINTER(_i32), _vp, _i32, _i32, _i32, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lt_op_region_text_combine": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_ode_combine": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _i64, _vp]),
    "lt_op_ode_combine_masked": (_i32, [_i32, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _f32, _f32, _f32, _i64, _vp]),
    "lt_op_ode_multistep": (_i32, [_vp, C.POINTER(_vp), _i32, C.POINTER(_f32), C.POINTER(_f32), _i32, _vp, _vp, _i64, _i32, _vp]),
    "lt_op_rope_table": (_i32, [_vp, _i32, _i32, _i32, _f32, _f32, _f32, _f32, _i32, _vp, _vp]),
    "lt_op_linear_small_m_ext": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _i32, _i32, _i32, C.c_uint32, C.c_uint32, _vp]),
    "lt_op_moe_route": (_i32, [_vp, _vp, _vp, _i32, _i32, _i32, _i32, _vp, _vp, _i32, _vp]),
    "lt_op_moe_plan_ex": (_i32, [_vp, _vp, _i32, _vp, _vp, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i64, _i64, _i64, _vp]),
    "lt_op_rope_table_2d": (_i32, [_vp, _i32, _i32, _f32, _f32, _vp]),
    "lt_op_rope_table_2d_pair": (_i32, [_vp, _vp, _i32, _i32, _f32, _f32, _vp]),
    "lt_op_proj_gated_residual_norm": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, _i32, _vp]),
    "lt_op_qkv_qstat": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _i32, _f32, _vp, _vp, _vp, _vp]),
    "lt_op_attention_qraw": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_attention_qraw_ex": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp,
                                       _i32, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_attention_qraw_nk": (_i32, [_vp, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _f32, _vp, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp,
                                       _i32, _i32, _i32, _i32, _i32, _i32, _vp, _vp]),
    "lt_op_attention_small": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _vp, _i32, _i32, _vp, _f32,
                                     _f32, _vp, _i32, _i32, _i32, _i32, _i32, _vp]),
    "lt_op_rmsnorm_mod_ex": (_i32, [_vp, _vp, _vp, _vp, _i32, _vp, _i32, _i32, _i32, _f32, _i32, _i32, _vp]),
    "lt_op_gated_residual_norm_ex": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _vp, _vp, _vp, _i32, _i32, _vp, _i32, _i32, _i32, _f32, _f32, _i32, _i32,
                                            _vp, _i32, _vp, _vp, _vp, _vp, _i32, _vp, _vp, _vp, _vp]),
    "lt_op_gemm_ystat": (_i32, [_vp, _vp, _vp, _vp, _i32, _i32, _i32, _i32, C.POINTER(_i32), _vp]),
    "lt_op_gated_residual_norm_describe": (_i32, [_i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _i32, C.c_char_p, _i32]),
    "lt_op_qk_norm_rope_ex": (_i32, [_vp, _i32, _i32, _vp, _vp, _f32, _vp, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp, _f32, _i32, _vp, _vp, _f32,
                                     _vp, _vp, _i32, _i32, _vp]),
    "lt_op_qk_norm_rope_pair": (_i32, [_vp, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _vp, _i32, _vp,
                                       _f32, _i32, _vp, _vp, _f32, _f32, _vp]),
    "lt_op_qkv_post": (_i32, [_vp, _i32, _i32, _i32, _i32, _vp, _vp, _vp, _vp, _f32, _vp, _vp, _vp, _i32, _i32, _i32, _i32, _i32, _i32, _i32, _vp,
                              _i32, _vp, _f32, _i32, _vp, _vp, _f32, _f32, _vp]),
}

_lib = None


def load() -> C.CDLL:
    """Load the HIP extension; raises LuminaLibError (never falls back) when it is unavailable."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise LuminaLibError(
            f"HIP extension not built: {LIB_PATH} is missing. Run `python -c 'import __graft_entry__ as g; g.build()'` "
            "(or `make -C lumina-t2x_amd/csrc`). There is no CPU/PyTorch fallback for the denoising path."
        )
    try:
        lib = C.CDLL(LIB_PATH)
    except OSError as exc:  # missing ROCm runtime, wrong arch, ...
        raise LuminaLibError(f"cannot load {LIB_PATH}: {exc}") from exc
    for name, (res, args) in _SIGNATURES.items():
        try:
            fn = getattr(lib, name)
        except AttributeError as exc:
            raise LuminaLibError(f"{LIB_PATH} does not export {name}") from exc
        fn.restype = res
        fn.argtypes = args
    _lib = lib
    return lib


def check(rc: int, what: str = "") -> None:
    if rc != 0:
        msg = load().lt_last_error()
        raise LuminaLibError(f"{what or 'lumina_dit call'} failed (rc={rc}): {msg.decode() if msg else '?'}")
