"""ctypes binding of libmmtta.so (the C ABI declared in include/mmtta.h).

There is deliberately no fallback: if the library is missing or a call fails, this module raises.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "csrc", "libmmtta.so")

F32, BF16 = 0, 1
CONV_FWD, CONV_DGRAD, CONVT_FWD, CONVT_DGRAD = 0, 1, 2, 3
NORM_INSTANCE, NORM_BATCH, NORM_GROUP = 0, 1, 2


class MmttaError(RuntimeError):
    pass


class Tensor(C.Structure):
    _fields_ = [
        ("ptr", C.c_void_p),
        ("n", C.c_int32), ("c", C.c_int32), ("d", C.c_int32), ("h", C.c_int32), ("w", C.c_int32),
        ("sn", C.c_int64), ("sc", C.c_int64), ("sd", C.c_int64), ("sh", C.c_int64), ("sw", C.c_int64),
        ("dtype", C.c_int32), ("flags", C.c_int32),
    ]


class NormOnLoad(C.Structure):
    _fields_ = [
        ("mean", C.c_void_p), ("rstd", C.c_void_p), ("gamma", C.c_void_p), ("beta", C.c_void_p),
        ("relu", C.c_int32), ("per_item", C.c_int32), ("scale", C.c_void_p), ("shift", C.c_void_p),
    ]


class NormOnLoadAct(NormOnLoad):
    """The whole mmtta_norm_on_load: the 56-byte layout above (all the library reads for ACT_NONE / ACT_RELU) with the
    appended LeakyReLU slope.  norm_on_load() builds this one, so a LEAKY_RELU descriptor is never read past its end."""
    _fields_ = [("negative_slope", C.c_float), ("_pad2", C.c_int32)]


class NormSets(C.Structure):           # mmtta_norm_sets
    _fields_ = [("items_per_set", C.c_int32), ("_pad", C.c_int32), ("affine_stride", C.c_int64), ("stats_stride", C.c_int64)]


class ConvDesc(C.Structure):
    _fields_ = [
        ("op", C.c_int32), ("ksize", C.c_int32), ("stride", C.c_int32), ("cin", C.c_int32), ("cout", C.c_int32),
        ("dtype", C.c_int32),
    ]


class PackItem(C.Structure):
    _fields_ = [("desc", ConvDesc), ("w_master", C.c_void_p), ("packed", C.c_void_p)]


class ParamSets(C.Structure):          # mmtta_param_sets
    _fields_ = [("items_per_set", C.c_int32), ("inner", C.c_int32), ("packed_outer", C.c_int64), ("packed_inner", C.c_int64),
                ("weight_outer", C.c_int64), ("weight_inner", C.c_int64), ("bias_outer", C.c_int64), ("bias_inner", C.c_int64)]


class ConvPlan(C.Structure):
    _fields_ = [
        ("tiles", C.c_int32), ("launches", C.c_int32), ("ksplit", C.c_int32), ("stats_rows", C.c_int32),
        ("config", C.c_int32), ("_pad", C.c_int32), ("workspace_bytes", C.c_int64),
    ]


class PointwiseRoute(C.Structure):     # mmtta_pointwise_route_t
    _fields_ = [("vox_per_row", C.c_int64), ("work_items", C.c_int64), ("grid_x", C.c_int64), ("grid_y", C.c_int32),
                ("family", C.c_int32), ("mode", C.c_int32), ("vec", C.c_int32), ("it", C.c_int32), ("count", C.c_int32),
                ("bf16_a", C.c_int32), ("bf16_b", C.c_int32), ("bf16_o", C.c_int32), ("has_b", C.c_int32),
                ("rows_per_n", C.c_int32), ("rows_per_block", C.c_int32), ("cpl", C.c_int32), ("nvl", C.c_int32),
                ("trips", C.c_int32), ("cb_passes", C.c_int32), ("second_trip", C.c_int32), ("leaky", C.c_int32)]


PW_OPS = ("channel_stats", "norm_bwd_reduce", "norm_bwd_apply", "norm_bwd_small", "combine", "lincomb", "upsample_fwd",
          "upsample_bwd")                                      # MMTTA_PW_OP_*: the index is the code
PW_FAMILIES = ("reduce", "reduce_stream", "elementwise", "combine8", "norm_bwd_apply8", "norm_bwd_small", "lincomb",
               "upsample_fwd", "upsample_bwd")                 # MMTTA_PW_*: the index is the code


class OptimDesc(C.Structure):          # mmtta_optim_desc
    _fields_ = [("kind", C.c_int32), ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float),
                ("weight_decay", C.c_float), ("momentum", C.c_float), ("dampening", C.c_float), ("nesterov", C.c_int32)]


class UpdateTarget(C.Structure):       # mmtta_update_target
    _fields_ = [("optim", OptimDesc), ("w_p", C.c_void_p), ("w_m", C.c_void_p), ("w_v", C.c_void_p), ("b_p", C.c_void_p),
                ("b_m", C.c_void_p), ("b_v", C.c_void_p), ("b_grad", C.c_void_p), ("image", C.c_void_p * 2),
                ("image_outer", C.c_int64 * 2), ("image_inner", C.c_int64 * 2), ("step", C.c_void_p),
                ("w_decay", C.c_int32), ("b_decay", C.c_int32)]


OPTIM_ADAM, OPTIM_ADAMW, OPTIM_SGD = 0, 1, 2


class ConvEpilogue(C.Structure):
    _fields_ = [("add", C.POINTER(Tensor)), ("add_norm", NormOnLoadAct)]


class IntensityRule(C.Structure):      # mmtta_intensity_rule
    _fields_ = [("clip", C.c_int32), ("zscore", C.c_int32), ("masked", C.c_int32), ("min_count", C.c_int32),
                ("lo", C.c_float), ("hi", C.c_float), ("mask_gt", C.c_float), ("eps", C.c_float),
                ("mean", C.c_float), ("std", C.c_float), ("legacy", C.c_int32), ("_pad", C.c_int32)]


class InputNormBranch(C.Structure):    # mmtta_input_norm_branch
    _fields_ = [("dy", C.POINTER(Tensor)), ("weight", C.c_void_p), ("set_stride", C.c_int64), ("ksize", C.c_int32),
                ("stride", C.c_int32)]


class WindowGrid(C.Structure):         # mmtta_window_grid
    _fields_ = [("extent", C.c_int32 * 3), ("count", C.c_int32 * 3)]


class GuardRule(C.Structure):          # mmtta_guard_rule
    _fields_ = [("min_agreement_q16", C.c_uint32), ("max_growth_q16", C.c_uint32), ("max_shrink_q16", C.c_uint32),
                ("min_voxels", C.c_int32), ("scope", C.c_int32), ("reserved", C.c_int32)]


_P = C.POINTER
_SIGNATURES = {
    "mmtta_last_error": (C.c_char_p, []),
    "mmtta_abi_version": (C.c_int, []),
    "mmtta_set_option": (C.c_int, [C.c_int, C.c_int]),
    "mmtta_intensity_scratch_bytes": (C.c_int64, [C.c_int]),
    "mmtta_intensity_normalize": (C.c_int, [_P(Tensor), _P(IntensityRule), _P(Tensor), C.c_void_p, C.c_void_p]),
    "mmtta_copy_strided": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p]),
    "mmtta_conv_packed_bytes": (C.c_int64, [_P(ConvDesc)]),
    "mmtta_conv_pack_weights": (C.c_int, [_P(ConvDesc), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_conv_pack_table_bytes": (C.c_int64, [C.c_int]),
    "mmtta_conv_pack_table_build": (C.c_int, [_P(PackItem), C.c_int, C.c_void_p, _P(C.c_int64)]),
    "mmtta_conv_pack_batched": (C.c_int, [C.c_void_p, C.c_int, C.c_int64, C.c_void_p]),
    "mmtta_conv_plan": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(Tensor), _P(ConvPlan)]),
    "mmtta_conv_run": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), C.c_void_p, C.c_void_p, _P(ConvEpilogue),
                                 _P(Tensor), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p]),
    "mmtta_conv_run_sets": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), C.c_void_p, C.c_void_p, _P(ConvEpilogue),
                                      _P(Tensor), C.c_int, C.c_void_p, C.c_void_p, C.c_int64, _P(ParamSets), C.c_void_p]),
    "mmtta_conv_route": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_stages_raw": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_cls8_pipelined": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_cls8_lean_epilogue": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_thin_lean": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_thin_kernel": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_conv_head_loss_eligible": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(ConvEpilogue), _P(Tensor), _P(Tensor),
                                                C.c_int, C.c_int]),
    "mmtta_conv_head_loss_partials": (C.c_int64, [_P(ConvDesc), _P(Tensor), _P(Tensor)]),
    "mmtta_conv_head_loss_run_sets": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), C.c_void_p, C.c_void_p, _P(ConvEpilogue),
                                                _P(Tensor), _P(Tensor), C.c_int, C.c_int, C.c_void_p, C.c_void_p, _P(ParamSets),
                                                C.c_void_p]),
    "mmtta_conv_wgrad_workspace_bytes": (C.c_int64, [_P(ConvDesc), _P(Tensor), _P(Tensor)]),
    "mmtta_conv_wgrad_workspace_bytes_sets": (C.c_int64, [_P(ConvDesc), _P(Tensor), _P(Tensor), _P(ParamSets)]),
    "mmtta_conv_wgrad_plan_sets": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(Tensor), _P(ParamSets), _P(C.c_int32)]),
    "mmtta_conv_wgrad_sets": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(Tensor), C.c_void_p, C.c_void_p,
                                        C.c_int, C.c_void_p, C.c_int64, _P(ParamSets), C.c_void_p]),
    "mmtta_conv_wgrad_kernel": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(Tensor)]),
    "mmtta_conv_wgrad_stages_raw": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(Tensor)]),
    "mmtta_conv_wgrad": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(Tensor), C.c_void_p, C.c_void_p,
                                   C.c_int, C.c_void_p, C.c_int64, C.c_void_p]),
    "mmtta_norm_stats_finalize": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                            C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                            C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                            C.c_void_p]),
    "mmtta_norm_stats_finalize_sets": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                                 C.c_float, C.c_int, C.c_void_p, C.c_void_p, C.c_float, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                                 C.c_void_p, C.c_void_p, _P(NormSets), C.c_void_p]),
    "mmtta_reduce_rows_per_n": (C.c_int, [_P(Tensor)]),
    "mmtta_channel_stats": (C.c_int, [_P(Tensor), C.c_void_p, C.c_void_p]),
    "mmtta_combine": (C.c_int, [_P(Tensor), _P(NormOnLoad), _P(Tensor), _P(NormOnLoad), _P(Tensor), C.c_void_p]),
    "mmtta_norm_bwd_reduce": (C.c_int, [_P(Tensor), _P(Tensor), _P(NormOnLoad), C.c_void_p, C.c_void_p]),
    "mmtta_norm_bwd_finalize": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                          C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_void_p, C.c_void_p]),
    "mmtta_norm_bwd_finalize_sets": (C.c_int, [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int64,
                                               C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                               C.c_int, C.c_void_p, _P(NormSets), C.c_void_p]),
    "mmtta_norm_bwd_apply": (C.c_int, [_P(Tensor), _P(Tensor), _P(NormOnLoad), C.c_void_p, C.c_void_p, _P(Tensor),
                                       C.c_void_p]),
    "mmtta_norm_bwd_small_ok": (C.c_int, [_P(Tensor), _P(Tensor), _P(NormOnLoad), _P(Tensor)]),
    "mmtta_norm_bwd_small": (C.c_int, [_P(Tensor), _P(Tensor), _P(NormOnLoad), C.c_int64, _P(Tensor), C.c_void_p]),
    "mmtta_upsample2x_fwd": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p]),
    "mmtta_upsample2x_bwd": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_lincomb": (C.c_int, [C.c_int, _P(_P(Tensor)), _P(C.c_float), _P(Tensor), C.c_int, C.c_void_p]),
    "mmtta_pointwise_route": (C.c_int, [C.c_int, _P(_P(Tensor)), C.c_int, _P(NormOnLoad), _P(NormOnLoad), C.c_void_p, C.c_void_p,
                                        _P(PointwiseRoute)]),
    "mmtta_entropy_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_entropy_loss": (C.c_int, [_P(Tensor), C.c_int, _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_entropy_partials_items": (C.c_int64, [_P(Tensor)]),
    "mmtta_entropy_loss_items": (C.c_int, [_P(Tensor), C.c_int, _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_entropy_filtered_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_entropy_filtered_items": (C.c_int, [_P(Tensor), C.c_int, C.c_float, C.c_void_p, C.c_void_p, _P(Tensor), C.c_void_p,
                                               C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_mirror_views": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, _P(C.c_int32), C.c_void_p]),
    "mmtta_memo_partials": (C.c_int64, [_P(Tensor), C.c_int]),
    "mmtta_memo_loss_items": (C.c_int, [_P(Tensor), C.c_int, C.c_int, _P(C.c_int32), _P(Tensor), C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "mmtta_memo_ensemble": (C.c_int, [_P(Tensor), C.c_int, C.c_int, _P(C.c_int32), _P(Tensor), C.c_void_p]),
    "mmtta_affine_views": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_affine_ensemble": (C.c_int, [_P(Tensor), C.c_int, C.c_int, _P(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p,
                                        _P(Tensor), C.c_void_p]),
    "mmtta_consistency_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_consistency_loss_items": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_cotta_update_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "mmtta_cotta_update_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_int64,
                                          C.c_double, C.c_float, C.c_uint64, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_void_p]),
    "mmtta_magnitude_select_class": (C.c_int, [C.c_int64]),
    "mmtta_magnitude_select_chunks": (C.c_int64, [C.c_int64]),
    "mmtta_magnitude_select_scratch_bytes": (C.c_int64, [C.c_int, C.c_int]),
    "mmtta_magnitude_select_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int64, C.c_void_p,
                                              C.c_void_p, C.c_void_p]),
    "mmtta_petal_update_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "mmtta_petal_update_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                          C.c_int, C.c_int64, C.c_int, C.c_int64, C.c_int64, C.c_int64, C.c_double, C.c_void_p,
                                          C.c_void_p, C.c_void_p]),
    "mmtta_intensity_range_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_intensity_range": (C.c_int, [_P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_augment_views": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, _P(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p,
                                      C.c_uint64, C.c_void_p, C.c_void_p]),
    "mmtta_entropy_weighted_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_entropy_weighted_items": (C.c_int, [_P(Tensor), C.c_int, C.c_float, C.c_void_p, _P(Tensor), C.c_void_p, C.c_void_p,
                                               C.c_void_p, C.c_void_p]),
    "mmtta_pseudo_label_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_pseudo_label_loss_items": (C.c_int, [_P(Tensor), C.c_int, _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_fisher_accumulate_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int64, C.c_void_p]),
    "mmtta_fisher_scale": (C.c_int, [C.c_void_p, C.c_int64, C.c_float, C.c_void_p]),
    "mmtta_fisher_penalty_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "mmtta_fisher_penalty_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                            C.c_int64, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_patch_shuffle": (C.c_int, [_P(Tensor), _P(Tensor), _P(C.c_int32), C.c_void_p, C.c_void_p]),
    "mmtta_deyo_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_deyo_loss_items": (C.c_int, [_P(Tensor), _P(Tensor), _P(C.c_int32), C.c_void_p, C.c_int, C.c_float, C.c_float,
                                        C.c_float, C.c_void_p, _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p]),
    "mmtta_lame_refine": (C.c_int, [_P(Tensor), _P(Tensor), C.c_uint32, C.c_int, C.c_int, C.c_float, C.c_float, C.c_int,
                                    _P(Tensor), _P(Tensor), C.c_void_p, C.c_void_p]),
    "mmtta_guard_counts": (C.c_int, [_P(Tensor), _P(Tensor), C.c_float, C.c_void_p, C.c_void_p]),
    "mmtta_guard_select": (C.c_int, [C.c_void_p, _P(GuardRule), _P(Tensor), _P(Tensor), C.c_void_p, C.c_void_p]),
    "mmtta_crf_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_crf_entropy_items": (C.c_int, [_P(Tensor), _P(Tensor), C.c_uint32, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                          _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_nuclear_scratch": (C.c_int64, [_P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int]),
    "mmtta_nuclear_entropy_items": (C.c_int, [_P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float, C.c_float,
                                              _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_input_norm_apply": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p, C.c_void_p, C.c_uint32, C.c_int, C.c_void_p]),
    "mmtta_input_norm_grad_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_input_norm_grad": (C.c_int, [_P(Tensor), _P(InputNormBranch), C.c_int, C.c_void_p, C.c_void_p, C.c_uint32, C.c_int,
                                        C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_double, C.c_double,
                                        C.c_double, C.c_double, C.c_void_p]),
    "mmtta_bias_field_apply": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                         C.c_int, C.c_uint32, C.c_void_p]),
    "mmtta_bias_field_grad_partials": (C.c_int64, [_P(Tensor), C.c_int]),
    "mmtta_bias_field_grad": (C.c_int, [_P(Tensor), _P(InputNormBranch), C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_int, C.c_int, C.c_uint32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
                                        C.c_void_p, C.c_double, C.c_double, C.c_double, C.c_double, C.c_void_p]),
    "mmtta_modality_views": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, _P(C.c_uint32), C.c_void_p]),
    "mmtta_modcons_partials": (C.c_int64, [_P(Tensor), C.c_int]),
    "mmtta_modcons_loss_items": (C.c_int, [_P(Tensor), C.c_int, C.c_int, C.c_float, C.c_float, C.c_int, _P(Tensor), C.c_void_p,
                                           C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_window_views": (C.c_int, [_P(Tensor), _P(Tensor), _P(WindowGrid), _P(C.c_int32), C.c_void_p, C.c_float, C.c_void_p]),
    "mmtta_window_partials": (C.c_int64, [_P(Tensor)]),
    "mmtta_window_entropy_items": (C.c_int, [_P(Tensor), C.c_int, _P(WindowGrid), C.c_void_p, _P(Tensor), C.c_void_p, C.c_void_p,
                                             C.c_void_p]),
    "mmtta_window_blend": (C.c_int, [_P(Tensor), _P(Tensor), _P(WindowGrid), C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_adam_step": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64, C.c_float,
                                  C.c_float, C.c_float, C.c_float, C.c_float, C.c_void_p, C.c_void_p]),
    "mmtta_optim_step": (C.c_int, [_P(OptimDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                   C.c_void_p, C.c_void_p]),
    "mmtta_optim_step_sets": (C.c_int, [_P(OptimDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_int64,
                                        C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "mmtta_optim_step_segments": (C.c_int, [_P(OptimDesc), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int,
                                            C.c_int64, C.c_int, C.c_int64, C.c_void_p, C.c_void_p]),
    "mmtta_fused_update_enabled": (C.c_int, []),
    "mmtta_conv_wgrad_update_sets": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(Tensor), _P(UpdateTarget),
                                               C.c_void_p, C.c_int64, _P(ParamSets), C.c_void_p]),
    "mmtta_conv_wgrad_updates_in_epilogue": (C.c_int, [_P(ConvDesc), _P(Tensor), _P(NormOnLoad), _P(Tensor), _P(ParamSets)]),
    "mmtta_sam_ascent_partials": (C.c_int64, [C.c_int64, C.c_int]),
    "mmtta_sam_ascent_sets": (C.c_int, [C.c_void_p, C.c_void_p, C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.c_int, C.c_int,
                                        C.c_int64, C.c_float, C.c_void_p]),
    "mmtta_mask_dice_counts": (C.c_int, [_P(Tensor), _P(Tensor), C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_dice_ce_scratch_bytes": (C.c_int64, [_P(Tensor)]),
    "mmtta_dice_ce_sums": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_dice_ce_grad": (C.c_int, [_P(Tensor), _P(Tensor), C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_float, C.c_float,
                                     C.c_float, C.c_float, C.c_void_p, _P(Tensor), C.c_void_p]),
    "mmtta_calibration_scratch_bytes": (C.c_int64, [_P(Tensor), C.c_int]),
    "mmtta_calibration_bins": (C.c_int, [_P(Tensor), _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_components_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_components_filter": (C.c_int, [C.c_void_p, C.c_void_p, _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _P(C.c_int64), _P(C.c_int32), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_lesionwise_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_lesionwise_scores": (C.c_int, [C.c_void_p, _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int,
                                          _P(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_lesionwise_hd95_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_lesionwise_hd95": (C.c_int, [C.c_void_p, _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double), C.c_double,
                                        _P(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_mask_fill_nest_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_mask_fill_nest": (C.c_int, [C.c_void_p, _P(Tensor), C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_int32),
                                       _P(C.c_int64), _P(C.c_int32), C.c_int, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_surface_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_surface_distances": (C.c_int, [C.c_void_p, _P(Tensor), _P(C.c_double), C.c_double, C.c_int, C.c_void_p,
                                          C.c_void_p, C.c_void_p, C.c_void_p]),
    "mmtta_surface_dice_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_surface_dice": (C.c_int, [C.c_void_p, _P(Tensor), _P(C.c_double), _P(C.c_double), C.c_int, C.c_void_p, C.c_void_p,
                                     C.c_void_p]),
    "mmtta_lesionwise_nsd_list_slots": (C.c_int, []),
    "mmtta_lesionwise_nsd_scratch_bytes": (C.c_int64, [C.c_int64, C.c_int64, C.c_int64, C.c_int64]),
    "mmtta_lesionwise_nsd": (C.c_int, [C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_int, C.c_int, _P(C.c_double), _P(C.c_double),
                                       C.c_int, _P(C.c_int64), C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]),
}

# mmtta_set_option keys (include/mmtta.h MMTTA_OPT_*)
OPT_IGEMM_PIPELINE, OPT_EPILOGUE_VEC16, OPT_IGEMM_LEAN, OPT_WGRAD_VECTOR_STAGING = 6, 9, 10, 11
OPT_CLASS_FUSED_MIN_WORKGROUPS, OPT_THIN_MFMA, OPT_RAW_STAGING, OPT_HEAD_LOSS_PAIR, OPT_THIN_LEAN = 12, 13, 16, 17, 18
OPT_WGRAD_EPILOGUE_UPDATE, OPT_CLS8_PIPELINE, OPT_CLS8_LEAN_EPILOGUE = 19, 20, 21
# A/B aids read once by load(): (environment variable, option, form).  Form True: the value "1" switches the option off;
# False: the option is set to int(value) whenever the variable is present.  (MMTTA_NO_PIPE and the last six pick between
# kernels with the same results bit for bit.)
_ENV_OPTIONS = (
    ("MMTTA_NO_PIPE", OPT_IGEMM_PIPELINE, True),
    ("MMTTA_NO_EPIVEC", OPT_EPILOGUE_VEC16, True),
    ("MMTTA_WGVEC", OPT_WGRAD_VECTOR_STAGING, False),
    ("MMTTA_THINMFMA", OPT_THIN_MFMA, False),
    ("MMTTA_CLSFUSE", OPT_CLASS_FUSED_MIN_WORKGROUPS, False),
    ("MMTTA_LEAN", OPT_IGEMM_LEAN, False),
    ("MMTTA_RAWSTAGE", OPT_RAW_STAGING, False),
    ("MMTTA_HEADLOSS", OPT_HEAD_LOSS_PAIR, False),
    ("MMTTA_THINLEAN", OPT_THIN_LEAN, False),
    ("MMTTA_EPIUPDATE", OPT_WGRAD_EPILOGUE_UPDATE, False),
    ("MMTTA_CLS8PIPE", OPT_CLS8_PIPELINE, False),
    ("MMTTA_CLS8LEAN", OPT_CLS8_LEAN_EPILOGUE, False),
)

_lib = None


def load() -> C.CDLL:
    """Load libmmtta.so and type every entry point.  Raises if the library is not built."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise MmttaError(
            f"{LIB_PATH} is missing: build it with `python -m multimodal_tta_amd.build` (hipcc, gfx950). "
            "There is no CPU or PyTorch fallback for the adaptation path."
        )
    lib = C.CDLL(LIB_PATH)
    for name, (res, args) in _SIGNATURES.items():
        fn = getattr(lib, name)  # AttributeError if the ABI and the binding drifted apart
        fn.restype = res
        fn.argtypes = args
    if lib.mmtta_abi_version() != 2:
        raise MmttaError("libmmtta.so ABI version mismatch")
    for var, key, off_at_1 in _ENV_OPTIONS:
        if off_at_1:
            if os.environ.get(var, "0") == "1":
                lib.mmtta_set_option(key, 0)
        elif var in os.environ:
            lib.mmtta_set_option(key, int(os.environ[var]))
    _lib = lib
    return lib


def exported_names() -> Sequence[str]:
    return list(_SIGNATURES)


def check(status: int, what: str = "") -> None:
    if status != 0:
        msg = load().mmtta_last_error().decode("utf-8", "replace")
        raise MmttaError(f"{what or 'libmmtta'} failed with status {status}: {msg}")


def stream_ptr() -> int:
    return int(torch.cuda.current_stream().cuda_stream)


def ptr(t: Optional[torch.Tensor]) -> Optional[int]:
    return None if t is None else int(t.data_ptr())


TENSOR_OWNS_PAD = 1   # include/mmtta.h MMTTA_TENSOR_OWNS_PAD


def desc_cl(t: torch.Tensor) -> Tensor:
    """Descriptor of a channels-last activation view: torch shape [N, D, H, W, C], stride(C) == 1.  fp32, or bf16 for the
    forward activations of `bf16` precision (storage type travels in the descriptor; strides are in elements)."""
    if t.dim() != 5 or t.dtype not in (torch.float32, torch.bfloat16) or not t.is_cuda:
        raise MmttaError(f"expected a CUDA float32 / bfloat16 [N,D,H,W,C] view, got {tuple(t.shape)} {t.dtype} {t.device}")
    n, d, h, w, c = t.shape
    sn, sd, sh, sw, sc = t.stride()
    if sc != 1 and c != 1:
        raise MmttaError("activation views must have unit stride along C")
    flags = TENSOR_OWNS_PAD if getattr(t, "_mmtta_owns_pad", False) else 0
    return Tensor(t.data_ptr(), n, c, d, h, w, sn, 1, sd, sh, sw, BF16 if t.dtype == torch.bfloat16 else F32, flags)


def desc_ncdhw(t: torch.Tensor) -> Tensor:
    """Descriptor of a boundary tensor: torch shape [N, C, D, H, W], any strides."""
    if t.dim() != 5 or t.dtype != torch.float32 or not t.is_cuda:
        raise MmttaError(f"expected a CUDA float32 [N,C,D,H,W] tensor, got {tuple(t.shape)} {t.dtype} {t.device}")
    n, c, d, h, w = t.shape
    sn, sc, sd, sh, sw = t.stride()
    return Tensor(t.data_ptr(), n, c, d, h, w, sn, sc, sd, sh, sw, F32, 0)


ACT_NONE, ACT_RELU, ACT_LEAKY_RELU = 0, 1, 2       # mmtta_norm_on_load.relu: the activation code (mmtta.h MMTTA_ACT_*)


def norm_on_load(mean=None, rstd=None, gamma=None, beta=None, relu=False, scale=None, shift=None,
                 per_item=False, act=None, negative_slope=0.0) -> NormOnLoadAct:
    """`act` (an ACT_* code) takes precedence over the older `relu` flag; `negative_slope` is read for ACT_LEAKY_RELU."""
    code = (ACT_RELU if relu else ACT_NONE) if act is None else int(act)
    return NormOnLoadAct(ptr(mean), ptr(rstd), ptr(gamma), ptr(beta), code, 1 if per_item else 0, ptr(scale),
                      ptr(shift), float(negative_slope) if code == ACT_LEAKY_RELU else 0.0, 0)
